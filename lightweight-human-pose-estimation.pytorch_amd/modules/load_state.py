"""Drop-ins for the reference's ``modules.load_state`` (modules/load_state.py).  ``load_state`` (:4-15):
copy every checkpoint tensor whose key AND shape match, keep the net's own value otherwise and
print the reference's warning line.  ``load_from_mobilenet`` (:18-32): the same against a MobileNet
checkpoint saved from a DataParallel wrapper, whose keys read ``module.model.*``."""
import collections


def load_state(net, checkpoint):
    source_state = checkpoint['state_dict']
    target_state = net.state_dict()
    merged = collections.OrderedDict()
    for key, value in target_state.items():
        src = source_state.get(key) if hasattr(source_state, "get") else None
        if src is not None and tuple(src.shape) == tuple(value.shape):
            merged[key] = src
        else:
            merged[key] = value
            print('[WARNING] Not found pre-trained parameters for {}'.format(key))
    net.load_state_dict(merged)


def load_from_mobilenet(net, checkpoint):
    source_state = checkpoint['state_dict']
    target_state = net.state_dict()
    merged = collections.OrderedDict()
    for key, value in target_state.items():
        k = key.replace('model', 'module.model')       # every occurrence, as the reference's str.replace does
        src = source_state.get(k) if hasattr(source_state, "get") else None
        if src is not None and tuple(src.shape) == tuple(value.shape):
            merged[key] = src
        else:
            merged[key] = value
            print('[WARNING] Not found pre-trained parameters for {}'.format(key))
    net.load_state_dict(merged)
