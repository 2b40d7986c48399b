"""Host-side engine over one C-ABI handle: marshals numpy / torch buffers to the library.

PyTorch is used only as a tensor container (device memory, ``data_ptr()``); every computation
is a HIP kernel behind include/lwpose.h.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import MEM_DEVICE, MEM_HOST, check, lib

_ROLE_NBT = 6


def _torch():
    import torch
    return torch


def _triple(values):
    """The three doubles of a ``pad_value`` / ``img_mean`` argument."""
    return (C.c_double * 3)(*[float(v) for v in values])


def _stride(stride):
    stride = int(stride)
    if stride < 1:
        raise ValueError("stride must be at least 1")
    return stride


def _data_or_null(a):
    """The address of a numpy array's data, None (a null pointer) for an empty one."""
    return a.ctypes.data if a.size else None


def _is_dtype(a, dtype):
    """``a`` (numpy array or torch tensor) holds elements of the numpy type ``dtype``."""
    return a.dtype == (dtype if isinstance(a, np.ndarray) else getattr(_torch(), np.dtype(dtype).name))


class Engine(object):
    def __init__(self, device_id=0, nref=1, num_channels=128, num_heatmaps=19, num_pafs=38, dtype=_lib.F32):
        self.h = _lib.Handle(device_id, nref, num_channels, num_heatmaps, num_pafs, dtype)
        self.nref, self.C, self.NH, self.NP = nref, num_channels, num_heatmaps, num_pafs
        self.device_id = device_id
        self._device = None                   # torch.device of the engine's GPU (``_gpu``)
        self._keep = None                     # tensors behind the raw pointers of the last asynchronous call
        self._keep_slot = {}                  # pipeline slot -> (cuda tensor kept alive until the slot is fetched, frames)
        self._overlay_shape = {}              # pipeline slot -> (N, H, W, 3) of the frames pipeline_submit_u8 took
        self._loss_keep = None                # tensors behind the pointers of the last loss call
        self._last_N = None                   # frames of the last serial pose-producing call
        self._skel = None                     # ``skeleton``, read back from the handle on demand
        self._caps = (2048, 128, 4096, 256)   # set_capacity: the library's defaults
        self._tracking_mode = 0
        self._overlay_mode = 0
        self._jpeg_entropy, self._jpeg_subseq = "host", 0
        self._gspec = None                    # ``grad_spec`` of the current train scope
        self.stage_steps = 0                  # adam_step calls so far: the drop-in net reads its stage parameters back when this moves
        self.train_scope = "stages"           # set_train_scope: "stages" | "cpm" | "all"
        self._scope_steps = 0                 # stage_steps when the current scope was set
        self._left_params = {}                # parameters an earlier, wider scope trained and the current one does not cover
        self._coco_n = 0                      # images of the open detection store (coco_open); 0: none, the library reports it
        self._val_store = None

    # ------------------------------------------------------------------ the library boundary
    def _call(self, name, *args):
        """``name(handle, *args)`` of the library; a failure raises what ``check`` makes of the return code and the handle's
        message.  Every entry point that takes the handle goes through here, but for the few that read the return code."""
        check(getattr(lib(), name)(self.h.ptr, *args), self.h.ptr)

    def _timed(self, run_name, time_name, args, iters, n_ms=1, tail=()):
        """``run_name(*args, *tail)``, returning None; or with ``iters`` > 0 its timing twin ``time_name(*args, iters, ms)``,
        returning the ``n_ms`` millisecond figures it wrote (one float, or a tuple)."""
        if not iters:
            self._call(run_name, *args, *tail)
            return None
        ms = (C.c_float * n_ms)()
        self._call(time_name, *args, int(iters), ms)
        return ms[0] if n_ms == 1 else tuple(ms)

    @property
    def _gpu(self):
        if self._device is None:
            torch = _torch()
            self._device = torch.device("cuda", self.device_id)
        return self._device

    def _empty(self, shape, dtype=None):
        """An uninitialised tensor on the engine's GPU; float32 unless ``dtype`` (a torch dtype) says otherwise."""
        torch = _torch()
        return torch.empty(shape, dtype=torch.float32 if dtype is None else dtype, device=self._gpu)

    def _ptr(self, x, dtype=None, what="input", convert=True):
        """(pointer, MEM_HOST or MEM_DEVICE, the contiguous object behind the pointer) of a numpy array, a cpu tensor or a cuda
        tensor: the one place a caller's buffer becomes an address.  The caller keeps the third value alive for as long as the
        library may read the pointer.  ``dtype`` (a numpy type) is the element type the library reads; None leaves the
        elements as they are, for callers that check the type themselves.  Host data is converted to ``dtype``; a cuda tensor
        of another type is converted too, or with ``convert=False`` refused (TypeError).  A cuda tensor on another GPU than
        the engine's is refused (ValueError).  A copy is made only of what is not contiguous or is converted."""
        if getattr(x, "is_cuda", False):
            if x.device.index != self.device_id:
                raise ValueError("%s %s on cuda:%d but the engine lives on cuda:%d"
                                 % (what, "are" if what.endswith("s") else "is", x.device.index, self.device_id))
            if dtype is not None and not _is_dtype(x, dtype):
                if not convert:
                    raise TypeError("%s must be a %s cuda tensor, got %s" % (what, np.dtype(dtype).name, x.dtype))
                x = x.to(getattr(_torch(), np.dtype(dtype).name))
            a = x.detach().contiguous()
            return a.data_ptr(), MEM_DEVICE, a
        a = np.ascontiguousarray(x.detach().numpy() if hasattr(x, "detach") else x, dtype=dtype)
        return a.ctypes.data, MEM_HOST, a

    def _dev32(self, t, what, shape, optional=False):
        """``t`` as a contiguous float32 cuda tensor of ``shape`` on the engine's GPU (the targets, masks and stage tensors of
        the loss and the backward); ``optional``: None stays None."""
        if t is None and optional:
            return None
        if not getattr(t, "is_cuda", False):
            raise TypeError("%s must be a cuda tensor" % what)
        if tuple(t.shape) != shape:
            raise ValueError("%s has shape %s, expected %s" % (what, tuple(t.shape), shape))
        return self._ptr(t, np.float32, what)[2]

    def _stage_shapes(self, N, H, W):
        """Shapes of the 2 (1 + nref) stage outputs for an (N, 3, H, W) input: three stride-2 layers, out = (in - 1) // 2 + 1."""
        for _ in range(3):
            H, W = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        return [(N, self.NP if i % 2 else self.NH, H, W) for i in range(2 * (1 + self.nref))]

    # ------------------------------------------------------------------ stream ordering
    def _order(self, device=None, hand_over=True):
        """Order the library's stream against torch's CURRENT stream on this GPU with events (lwp_set_stream): no host block.
        The reference's net(x) runs on the current stream (demo.py:64-68); this gives device tensors the same semantics —
        inputs written by queued torch work are waited for, and torch work queued after the call sees the device results.
        ``hand_over=False``: results left on the device stay on the library's stream (for its own next call)."""
        st = _torch().cuda.current_stream(self._gpu if device is None else device)
        self._call("lwp_set_stream", C.c_void_p(st.cuda_stream), 1 if hand_over else 2)

    # ------------------------------------------------------------------ weights
    def load_state_dict(self, state_dict):
        """state_dict: key -> torch tensor / numpy array (float32; num_batches_tracked int64)."""
        names, arrs = [], []
        for k, v in state_dict.items():
            a = v.detach().cpu().numpy() if hasattr(v, "detach") else np.asarray(v)
            if a.dtype != np.int64:
                a = np.ascontiguousarray(a, dtype=np.float32)
            names.append(k.encode())
            arrs.append(np.ascontiguousarray(a))
        n = len(names)
        c_names = (C.c_char_p * n)(*names)
        c_ptrs = (C.c_void_p * n)(*[a.ctypes.data for a in arrs])
        shapes = np.ones((n, 4), dtype=np.int64)
        ndims = np.zeros(n, dtype=np.int32)
        for i, a in enumerate(arrs):
            ndims[i] = a.ndim
            shapes[i, :a.ndim] = a.shape
        self._call("lwp_load_weights", c_names, c_ptrs, shapes.ctypes.data, ndims.ctypes.data, n)
        self._left_params = {}                # every parameter has just been replaced
        self._scope_steps = self.stage_steps

    def weights_blob_bytes(self):
        n = C.c_size_t()
        self._call("lwp_weights_blob_bytes", C.byref(n))
        return n.value

    def export_weights(self, device_tensor):
        self._call("lwp_weights_blob_export", device_tensor.data_ptr(), device_tensor.numel() * device_tensor.element_size())

    def import_weights(self, device_tensor):
        self._call("lwp_weights_blob_import", device_tensor.data_ptr(), device_tensor.numel() * device_tensor.element_size())

    # ------------------------------------------------------------------ skeleton (modules/keypoints.py:5-8, group_keypoints' options)
    def set_skeleton(self, limb_kpts, limb_pafs, num_kpt_types=None, pose_entry_size=None, min_paf_score=0.05):
        """Grouping tables for a network trained on another key-point set: limb_kpts / limb_pafs are the L (a, b) key-point
        type pairs and their PAF channel pairs, in grouping order.  num_kpt_types defaults to num_heatmaps - 1,
        pose_entry_size to max(20, K + 2).  ``limb_kpts=None`` restores the COCO default.  Bad tables raise ValueError."""
        if limb_kpts is None:
            self._call("lwp_set_skeleton", 0, 0, None, None, 0, 0.0)
            self._skel = None
            return
        kp = np.ascontiguousarray(np.asarray(limb_kpts, dtype=np.int64).reshape(-1, 2), dtype=np.int32)
        pf = np.ascontiguousarray(np.asarray(limb_pafs, dtype=np.int64).reshape(-1, 2), dtype=np.int32)
        if len(kp) == 0:                       # (an empty table is an error, not the default: that is limb_kpts=None)
            raise ValueError("a skeleton needs 1..320 limbs, got none")
        if len(kp) != len(pf):
            raise ValueError("limb_kpts and limb_pafs must have the same number of limbs (%d != %d)" % (len(kp), len(pf)))
        K = int(self.NH - 1 if num_kpt_types is None else num_kpt_types)
        E = int(max(20, K + 2) if pose_entry_size is None else pose_entry_size)
        self._call("lwp_set_skeleton", K, len(kp), kp.ctypes.data, pf.ctypes.data, E, float(min_paf_score))
        self._skel = None

    @property
    def skeleton(self):
        """dict(num_kpt_types, limb_kpts (L,2), limb_pafs (L,2), pose_entry_size, min_paf_score) of the handle."""
        if self._skel is None:
            K, L, E, mp = C.c_int(), C.c_int(), C.c_int(), C.c_double()
            self._call("lwp_get_skeleton", C.byref(K), C.byref(L), None, None, 0, C.byref(E), C.byref(mp))
            kp = np.zeros((L.value, 2), np.int32)
            pf = np.zeros((L.value, 2), np.int32)
            self._call("lwp_get_skeleton", None, None, kp.ctypes.data, pf.ctypes.data, L.value, None, None)
            self._skel = dict(num_kpt_types=K.value, limb_kpts=kp, limb_pafs=pf, pose_entry_size=E.value, min_paf_score=mp.value)
        return self._skel

    @property
    def post_generic(self):
        """True when the generic grouping kernels run (custom skeleton, or LWP_POST_GENERIC=1 at creation) — debug."""
        rc = lib().lwp_debug_post_generic(self.h.ptr)
        if rc < 0:
            check(rc, self.h.ptr)
        return rc == 1

    def set_capacity(self, max_peaks=2048, max_kpts=128, max_conn=4096, max_entries=256):
        self._call("lwp_set_capacity", max_peaks, max_kpts, max_conn, max_entries)
        self._caps = (max_peaks, max_kpts, max_conn, max_entries)

    @property
    def caps(self):
        return self._caps

    # ------------------------------------------------------------------ network
    def forward(self, x):
        """x: (N,3,H,W) float32 torch tensor (cpu or cuda) or numpy array -> list of 2(1+nref) outputs of the
        same kind (NCHW), like PoseEstimationWithMobileNet.forward (with_mobilenet.py:114-123)."""
        torch = _torch()
        if len(x.shape) != 4 or x.shape[1] != 3:
            raise ValueError("expected input of shape (N, 3, H, W), got %s" % (tuple(x.shape),))
        ptr, mem, a = self._ptr(x, np.float32)
        N, _, H, W = a.shape
        outs = [torch.empty(s, dtype=torch.float32, device=a.device if mem == MEM_DEVICE else "cpu") for s in self._stage_shapes(N, H, W)]
        ptrs = (C.c_void_p * len(outs))(*[o.data_ptr() for o in outs])
        if mem == MEM_DEVICE:
            self._order(a.device)                 # events both ways: the outputs are valid for work queued on torch's current stream
            # (a frame from preprocess_u8(hand_over=False) is in order on the engine's stream; the outputs still need the hand-over)
        self._call("lwp_forward", ptr, mem, N, H, W, ptrs, mem)
        return [o.numpy() for o in outs] if isinstance(x, np.ndarray) else outs

    def synchronize(self):
        self._call("lwp_synchronize")

    # ------------------------------------------------------------------ post-processing pieces
    def upsample(self, maps_nchw, ratio=4):
        """(N,C,h,w) float32 numpy -> (N, h*r, w*r, C) float32 numpy (cv2.resize INTER_CUBIC, demo.py:72,76)."""
        ptr, mem, a = self._ptr(maps_nchw, np.float32, "maps", convert=False)
        if mem == MEM_DEVICE:
            self._order(a.device)
        N, Cc, h, w = a.shape
        out = np.empty((N, h * ratio, w * ratio, Cc), dtype=np.float32)
        self._call("lwp_upsample", ptr, mem, N, Cc, h, w, ratio, out.ctypes.data, MEM_HOST)
        return out

    @staticmethod
    def preprocess_dims(height, width, net_input_height_size, stride):
        """(scaled_h, scaled_w, out_h, out_w, pad [top,left,bottom,right], scale) of demo.py:55-62 for a height x width frame."""
        v = [C.c_int() for _ in range(4)]
        pad = (C.c_int * 4)()
        sc = C.c_double()
        check(lib().lwp_preprocess_dims(height, width, net_input_height_size, stride, *[C.byref(a) for a in v], pad, C.byref(sc)))
        return v[0].value, v[1].value, v[2].value, v[3].value, [int(a) for a in pad], sc.value

    def preprocess_u8(self, img, net_input_height_size, stride, pad_value=(0, 0, 0), img_mean=(128, 128, 128), img_scale=1 / 256,
                      hand_over=True):
        """uint8 HxWx3 frame (numpy or cuda tensor) -> (x: 1x3xH'xW' float32 cuda tensor, scale, pad): the cubic resize,
        normalize and pad_width of demo.py:55-64 in one kernel.  ``hand_over=False`` (infer_fast's internal use): x is only meant
        for this engine's next call — it stays on the engine's stream and that call skips the stream ordering (no events)."""
        ptr, mem, a = self._ptr(img, what="frame")
        if not _is_dtype(a, np.uint8) or len(a.shape) != 3 or a.shape[2] != 3:
            raise TypeError("frame must be HxWx3 uint8")
        H, W = int(a.shape[0]), int(a.shape[1])
        _, _, oh, ow, pad, scale = self.preprocess_dims(H, W, net_input_height_size, stride)
        x = self._empty((1, 3, oh, ow))
        self._order(hand_over=hand_over)          # x is handed to torch's current stream by event; a host frame may be reused on return
        self._call("lwp_preprocess_u8", ptr, mem, H, W, net_input_height_size, stride, _triple(pad_value), _triple(img_mean),
                   float(img_scale), x.data_ptr())
        if not hand_over:
            x._lwp_stream_owner = self            # produced on this engine's stream, not visible to torch's stream
        return x, scale, pad

    def _u8_frames(self, frames, dtypes=(np.uint8,), kinds="uint8"):
        """(pointer, mem flag, N, H, W, the array kept alive) of a uint8 frame batch (N,H,W,3) or one frame (H,W,3), numpy or a
        cuda tensor on this engine's GPU."""
        ptr, mem, a = self._ptr(frames, what="frames")
        if not any(_is_dtype(a, t) for t in dtypes) or len(a.shape) not in (3, 4) or a.shape[-1] != 3:
            raise TypeError("frames must be (N,)HxWx3 %s" % kinds)
        shp = tuple(a.shape) if len(a.shape) == 4 else (1,) + tuple(a.shape)
        return ptr, mem, int(shp[0]), int(shp[1]), int(shp[2]), a

    def preprocess_u8_batch(self, frames, net_input_height_size, stride, pad_value=(0, 0, 0), img_mean=(128, 128, 128), img_scale=1 / 256,
                            hand_over=True):
        """N same-sized uint8 frames (N,H,W,3) or one (H,W,3), numpy or cuda tensor -> (x: N x 3 x H' x W' float32 cuda tensor,
        scale, pad): ``preprocess_u8`` for a batch in ONE launch (demo.py:55-64 per frame, same bits)."""
        ptr, mem, N, H, W, a = self._u8_frames(frames)
        _, _, oh, ow, pad, scale = self.preprocess_dims(H, W, net_input_height_size, stride)
        x = self._empty((N, 3, oh, ow))
        self._order(hand_over=hand_over)
        self._call("lwp_preprocess_u8_batch", ptr, mem, N, H, W, net_input_height_size, stride, _triple(pad_value), _triple(img_mean),
                   float(img_scale), x.data_ptr())
        if not hand_over:
            x._lwp_stream_owner = self
        return x, scale, pad

    @staticmethod
    def scale_dims(height, width, ratio, base_height, stride):
        """(scaled_h, scaled_w, out_h, out_w, pad [top,left,bottom,right]) of val.py:89-91 for a height x width frame."""
        v = [C.c_int() for _ in range(4)]
        pad = (C.c_int * 4)()
        check(lib().lwp_scale_dims(height, width, float(ratio), base_height, stride, *[C.byref(a) for a in v], pad))
        return v[0].value, v[1].value, v[2].value, v[3].value, [int(a) for a in pad]

    def preprocess_scaled_u8(self, imgs, ratio, base_height, stride, pad_value=(0, 0, 0), img_mean=(128, 128, 128), img_scale=1 / 256):
        """N same-sized frames (N,H,W,3) or one (H,W,3), numpy or cuda tensor, uint8 or float32 -> (x: N x 3 x H' x W' float32
        cuda tensor, pad): normalize + cubic resize by ``ratio`` + pad_width of val.py:84-93 in one kernel."""
        ptr, mem, N, H, W, a = self._u8_frames(imgs, (np.uint8, np.float32), "uint8 or float32")
        _, _, oh, ow, pad = self.scale_dims(H, W, ratio, base_height, stride)
        self._order()
        x = self._empty((N, 3, oh, ow))
        self._call("lwp_preprocess_scaled_u8" if _is_dtype(a, np.uint8) else "lwp_preprocess_scaled_f32", ptr, mem, N, H, W, float(ratio),
                   base_height, stride, _triple(pad_value), _triple(img_mean), float(img_scale), x.data_ptr())
        return x, pad

    def multiscale_accumulate(self, accum, maps, up_ratio, pad, n_scales, init=False):
        """accum (H,W,C) or (N,H,W,C) float32 [numpy or cuda tensor, updated in place] += resize(crop(upsample(maps))) / n_scales
        (val.py:96-101).  maps: (C,h,w) or (N,C,h,w) float32 numpy / cuda tensor; the N frames share pad and size.
        init=True: accum is treated as zero (first scale), so it may be uninitialised memory."""
        mp, mm, maps = self._ptr(maps, np.float32, "maps", convert=False)
        shp = tuple(maps.shape)
        ashp = tuple(accum.shape)
        N = shp[0] if len(shp) == 4 else 1
        if len(ashp) not in (3, 4) or (len(ashp) == 4 and ashp[0] != N) or (len(ashp) == 3 and N != 1):
            raise ValueError("accum / maps batch mismatch")
        H, W, Cc = ashp[-3:]
        if Cc != shp[-3]:
            raise ValueError("channel mismatch")
        if getattr(accum, "is_cuda", False):
            if not accum.is_contiguous() or accum.dtype != _torch().float32:
                raise TypeError("accum must be a contiguous float32 tensor")
        elif accum.dtype != np.float32 or not accum.flags.c_contiguous:
            raise TypeError("accum must be a C-contiguous float32 array")
        ap, am, _ = self._ptr(accum, what="accum")     # contiguous, so this is accum itself: updated in place
        if mm == MEM_DEVICE or am == MEM_DEVICE:
            self._order()
        padv = (C.c_int * 4)(*[int(v) for v in pad])
        self._call("lwp_multiscale_accumulate", mp, mm, N, shp[-3], shp[-2], shp[-1], up_ratio, padv, H, W, n_scales, ap, am, 1 if init else 0)
        return accum

    def extract_keypoints(self, heatmap):
        """In-place threshold of ``heatmap`` (2-D float32 view) and key-point list [(x, y, score)]."""
        if not isinstance(heatmap, np.ndarray) or heatmap.ndim != 2 or heatmap.dtype != np.float32:
            raise TypeError("heatmap must be a 2-D float32 numpy array (view)")
        if not heatmap.flags.writeable:
            raise ValueError("heatmap must be writeable (it is thresholded in place)")
        H, W = heatmap.shape
        if heatmap.strides[0] % 4 or heatmap.strides[1] % 4:
            raise ValueError("unsupported strides")
        cap = self.caps[1]
        xs = np.empty(cap, np.int64); ys = np.empty(cap, np.int64); sc = np.empty(cap, np.float32)
        n = C.c_int()
        self._call("lwp_extract_keypoints", heatmap.ctypes.data, H, W, heatmap.strides[0] // 4, heatmap.strides[1] // 4,
                   xs.ctypes.data, ys.ctypes.data, sc.ctypes.data, cap, C.byref(n))
        return xs[:n.value], ys[:n.value], sc[:n.value]

    def group_keypoints(self, kpts, type_counts, pafs, demo):
        """kpts (n,4) float64, type_counts (K,), pafs (H,W,num_pafs) float32 -> (P,E) float64 (K / E: the skeleton's, 18 / 20 by
        default)."""
        pafs = np.ascontiguousarray(pafs, dtype=np.float32)
        H, W, NPc = pafs.shape
        if NPc != self.NP:
            raise ValueError("pafs must have %d channels" % self.NP)
        kp = np.ascontiguousarray(kpts, dtype=np.float64).reshape(-1, 4)
        tc = np.ascontiguousarray(type_counts, dtype=np.int32)
        sk = self.skeleton
        if tc.shape != (sk["num_kpt_types"],):
            raise ValueError("type_counts must have %d entries (the skeleton's key-point types)" % sk["num_kpt_types"])
        cap = self.caps[3]
        ent = np.empty((cap, sk["pose_entry_size"]), np.float64)
        n = C.c_int()
        self._call("lwp_group_keypoints", kp.ctypes.data, tc.ctypes.data, pafs.ctypes.data, MEM_HOST, H, W, 1 if demo else 0,
                   ent.ctypes.data, cap, C.byref(n))
        return ent[:n.value].copy()

    # ------------------------------------------------------------------ fused pipeline
    def _frames_of(self, slot=-1):
        """Frames of the last serial pose-producing call (slot < 0) or of a submitted pipeline slot."""
        if slot < 0:
            if self._last_N is None:
                raise RuntimeError("no poses yet: call infer_poses, infer_poses_async or poses_from_maps first")
            return self._last_N
        if slot not in self._keep_slot:
            raise RuntimeError("slot %r holds nothing: call pipeline_submit or pipeline_submit_u8 for it first" % (slot,))
        return self._keep_slot[slot][1]

    def _result_buffers(self, N):
        """(the four host arrays a pose-producing call fills for N frames, the argument tail that hands them to the library)."""
        sk = self.skeleton
        K, E = sk["num_kpt_types"], sk["pose_entry_size"]
        kcap = K * self.caps[1]
        ecap = self.caps[3]
        counts, kpts, ent, ne = np.zeros((N, K), np.int32), np.zeros((N, kcap, 4), np.float64), np.zeros((N, ecap, E), np.float64), np.zeros(N, np.int32)
        return (counts, kpts, ent, ne), (counts.ctypes.data, kpts.ctypes.data, kcap, ent.ctypes.data, ecap, ne.ctypes.data)

    @staticmethod
    def _unpack(counts, kpts, ent, ne):
        out = []
        for f in range(len(ne)):
            K = int(counts[f].sum())
            out.append((ent[f, :ne[f]].copy(), kpts[f, :K].copy(), counts[f].copy()))
        return out

    def infer_poses(self, x, upsample_ratio=4, demo=True):
        """x: (N,3,H,W) float32 (numpy / cpu tensor / cuda tensor), already normalised and padded.
        Returns per frame (pose_entries (P,E) f64, all_keypoints (n,4) f64, type_counts (K,)); K / E of the skeleton (18 / 20 by
        default)."""
        ptr, mem, t = self._ptr(x, np.float32)
        N, _, H, W = t.shape
        bufs, tail = self._result_buffers(N)
        if mem == MEM_DEVICE and getattr(x, "_lwp_stream_owner", None) is not self:
            self._order(t.device)
        self._call("lwp_infer_poses", ptr, mem, N, H, W, upsample_ratio, 1 if demo else 0, *tail)
        self._last_N = N
        return self._unpack(*bufs)

    def _maps(self, heat, paf, layout):
        """(heat pointer, paf pointer, mem flag, layout code, N, h, w, the two arrays kept alive) of a pair of float32 maps, both
        numpy or both cuda tensors; device maps are ordered behind torch's current stream."""
        lay = {"NCHW": 0, "NHWC": 1}[layout]
        hp, mem, heat = self._ptr(heat, np.float32, "heat", convert=False)
        pp, pmem, paf = self._ptr(paf, np.float32, "paf", convert=False)
        if pmem != mem:
            raise TypeError("heat and paf must both be numpy arrays or both cuda tensors")
        if mem == MEM_DEVICE:
            self._order(heat.device)
        N, hs, ws = (heat.shape[0], heat.shape[2], heat.shape[3]) if lay == 0 else heat.shape[:3]
        return hp, pp, mem, lay, N, hs, ws, (heat, paf)

    def poses_from_maps(self, heat, paf, upsample_ratio=4, demo=True, layout="NCHW"):
        """Post-processing only.  layout "NCHW": the low-res stage outputs (N,19,h,w) / (N,38,h,w); layout "NHWC": full-res
        averaged maps (N,H,W,19) / (N,H,W,38) of the multi-scale path with upsample_ratio=1.  float32 numpy or cuda tensors."""
        hp, pp, mem, lay, N, hs, ws, _ = self._maps(heat, paf, layout)
        bufs, tail = self._result_buffers(N)
        self._call("lwp_poses_from_maps", hp, pp, mem, lay, N, hs, ws, upsample_ratio, 1 if demo else 0, *tail)
        self._last_N = N
        return self._unpack(*bufs)

    def layers(self):
        out = []
        name = C.create_string_buffer(128)
        v = [C.c_int() for _ in range(6)]
        macs = C.c_int64()
        for i in range(lib().lwp_layer_count(self.h.ptr)):
            self._call("lwp_layer_info", i, name, 128, *[C.byref(x) for x in v], C.byref(macs))
            out.append(dict(index=i, name=name.value.decode(), kind=v[0].value, cin=v[1].value, cout=v[2].value,
                            ksize=v[3].value, stride=v[4].value, dilation=v[5].value, macs_per_pixel=macs.value))
        return out

    def debug_layer_output(self, x, layer_index):
        """Output of layer ``layer_index`` (NCHW float32 numpy) for input x (N,3,H,W) numpy."""
        x = np.ascontiguousarray(x, dtype=np.float32)
        N, _, H, W = x.shape
        info = self.layers()[layer_index]
        buf = np.empty(N * info["cout"] * ((H + 1) // 2) * ((W + 1) // 2), np.float32)
        dims = (C.c_int * 4)()
        self._call("lwp_debug_layer_output", x.ctypes.data, N, H, W, layer_index, buf.ctypes.data, buf.size, dims)
        n = dims[0] * dims[1] * dims[2] * dims[3]
        return buf[:n].reshape(dims[0], dims[1], dims[2], dims[3]).copy()

    def frames_per_pass(self, N, H, W):
        """Frames one launch sequence of an (N,3,H,W) call takes (N unless the batch is split inside the call)."""
        n = lib().lwp_debug_frames_per_pass(self.h.ptr, N, H, W)
        if n < 0:
            raise ValueError("bad shape")
        return n

    def post_counts(self, frame=0):
        """(peaks per type before the NMS [K], key-points per type [K], scored connection candidates per limb [L], picked
        connections per limb [L]) of one frame of the last infer_poses / poses_from_maps call (debug; 18 / 19 by default)."""
        sk = self.skeleton
        K, L = sk["num_kpt_types"], len(sk["limb_kpts"])
        arrs = [(C.c_int * n)() for n in (K, K, L, L)]
        self._call("lwp_debug_post_counts_ex", frame, *arrs, K, L)
        return tuple(np.array(list(a), dtype=np.int64) for a in arrs)

    def layer_variant(self, layer_index):
        """Kernel variant the last debug_layer_output / profile_launches pass picked for a layer ("" before any)."""
        name = C.create_string_buffer(96)
        self._call("lwp_debug_layer_variant", layer_index, name, 96)
        return name.value.decode()

    def _as_device_input(self, x):
        """Checks shared by every entry point that hands ``data_ptr()`` of a resident frame batch to the library: float32,
        contiguous, (N,3,H,W), on this engine's GPU; work still queued on torch's current stream is ordered before the
        library's (own, non-blocking) stream by an event — the host does not wait."""
        torch = _torch()
        if not getattr(x, "is_cuda", False):
            raise TypeError("expected a cuda tensor")
        if x.dtype != torch.float32 or x.dim() != 4 or x.shape[1] != 3:
            raise TypeError("expected a float32 (N, 3, H, W) tensor, got %s %s" % (x.dtype, tuple(x.shape)))
        if not x.is_contiguous():
            raise ValueError("input tensor must be contiguous")
        if x.device.index != self.device_id:
            raise ValueError("input is on cuda:%d but the engine lives on cuda:%d" % (x.device.index, self.device_id))
        if getattr(x, "_lwp_stream_owner", None) is not self:     # (a tensor this engine produced on its own stream is in order already)
            self._order(x.device)
        return x

    def infer_poses_async(self, x_cuda, upsample_ratio=4, demo=True):
        x_cuda = self._as_device_input(x_cuda)
        N, _, H, W = x_cuda.shape
        self._keep = x_cuda
        self._call("lwp_infer_poses_async", x_cuda.data_ptr(), N, H, W, upsample_ratio, 1 if demo else 0)
        self._last_N = N

    def fetch_poses(self):
        bufs, tail = self._result_buffers(self._frames_of())
        self._call("lwp_fetch_poses", *tail)
        return self._unpack(*bufs)

    # ------------------------------------------------------------------ pipelined streaming (two slots)
    def pipeline_submit(self, x_cuda, slot, upsample_ratio=4, demo=True):
        x_cuda = self._as_device_input(x_cuda)
        N, _, H, W = x_cuda.shape
        self._keep_slot[slot] = (x_cuda, N)
        self._call("lwp_pipeline_submit", x_cuda.data_ptr(), N, H, W, upsample_ratio, 1 if demo else 0, slot)

    def pipeline_submit_u8(self, frames, slot, net_input_height_size, stride=8, pad_value=(0, 0, 0), img_mean=(128, 128, 128),
                           img_scale=1 / 256, upsample_ratio=4, demo=True):
        """One-call video step (demo.py:55-68 + 91-118): uint8 frames (N,H,W,3) or (H,W,3), numpy or cuda tensor -> upload,
        batched pre-processing, network, grouping and (if ``set_tracking`` is on) the pose tail, all enqueued; returns at once.
        Read the results with ``pipeline_fetch(slot)`` and ``poses(slot)`` (and, with ``set_overlay`` on, ``pipeline_overlay(slot)``).  The tail un-maps with this submit's own stride,
        scale and pad (``preprocess_dims`` of the frame size): ``set_unmap`` is neither used nor changed.  A numpy frame buffer
        may be reused on return; a cuda tensor is kept alive until the slot is fetched."""
        ptr, mem, N, H, W, a = self._u8_frames(frames)
        if mem == MEM_DEVICE:
            self._order(a.device)
        self._call("lwp_pipeline_submit_u8", ptr, mem, N, H, W, net_input_height_size, stride, _triple(pad_value), _triple(img_mean),
                   float(img_scale), upsample_ratio, 1 if demo else 0, slot)
        self._keep_slot[slot] = (a if mem == MEM_DEVICE else None, N)
        self._overlay_shape[slot] = (N, H, W, 3)

    def pipeline_fetch(self, slot):
        bufs, tail = self._result_buffers(self._frames_of(slot))
        self._call("lwp_pipeline_fetch", slot, *tail)
        return self._unpack(*bufs)

    # ------------------------------------------------------------------ pose tail on the device (demo.py:101-118)
    TRACK_OFF, TRACK_ROWS, TRACK_LANES, TRACK_SEQUENCE = 0, 1, 2, 3

    def set_tracking(self, mode, match_threshold=3, similarity_threshold=0.5, smooth=False, sigmas=None):
        """Pose tail behind the grouping kernels: mode 0 off (default), 1 pose rows only, 2 lanes (frame f of a batch continues
        lane f), 3 sequence (the frames of a batch are consecutive frames of lane 0).  ``sigmas``: K float32 values as
        ``Pose.sigmas`` holds them; None = the COCO table (18 types only).  Clears every lane."""
        mode = {"off": 0, "rows": 1, "lanes": 2, "sequence": 3}.get(mode, mode)
        sg, n = None, 0
        if sigmas is not None:
            sg = np.ascontiguousarray(sigmas, dtype=np.float32)
            n = int(sg.size)
        self._call("lwp_set_tracking", int(mode), int(match_threshold), float(similarity_threshold), 1 if smooth else 0,
                   None if sg is None else sg.ctypes.data, n)
        self._tracking_mode = int(mode)

    def set_unmap(self, stride, scale, pad):
        """Geometry of the un-map (demo.py:101-103) for the following pose-producing calls; ``pad`` = [top, left, ...] as
        ``preprocess_dims`` / ``infer_fast`` return it."""
        self._call("lwp_set_unmap", int(stride), float(scale), int(pad[0]), int(pad[1]))

    def reset_tracking(self, lane=-1, next_id=0):
        """Clears a lane (-1: all) and sets the first id it gives out."""
        self._call("lwp_reset_tracking", int(lane), int(next_id))

    def poses(self, slot=-1):
        """Pose rows of the last infer_poses / poses_from_maps / fetch_poses (slot -1) or of a fetched pipeline slot: per frame a
        dict of keypoints (P,K,2) int32, confidence (P,) f64, bbox (P,4) int32, ids (P,) int32 (-1 without tracking), last_id and
        near (similarity decisions the device could round differently from NumPy; 0 on every fixture)."""
        N = self._frames_of(slot)
        K, cap = self.skeleton["num_kpt_types"], self.caps[3]
        n = np.zeros(N, np.int32)
        kp = np.zeros((N, cap, K, 2), np.int32)
        conf = np.zeros((N, cap), np.float64)
        bbox = np.zeros((N, cap, 4), np.int32)
        ids = np.zeros((N, cap), np.int32)
        last = np.zeros(N, np.int32)
        near = np.zeros(N, np.uint32)
        self._call("lwp_get_poses", slot, n.ctypes.data, kp.ctypes.data, conf.ctypes.data, bbox.ctypes.data, ids.ctypes.data,
                   last.ctypes.data, cap)
        self._call("lwp_debug_tracking_near", slot, near.ctypes.data, N)
        return [dict(keypoints=kp[f, :n[f]].copy(), confidence=conf[f, :n[f]].copy(), bbox=bbox[f, :n[f]].copy(),
                     ids=ids[f, :n[f]].copy(), last_id=int(last[f]), near=int(near[f])) for f in range(N)]

    def track_poses_device(self, keypoints, confidence, lane=0):
        """One tracking step of ``lane`` on caller-supplied poses ((P,K,2) int32 key-points, (P,) confidences), on the kernels of
        the pose tail.  Returns dict(keypoints, bbox, ids, last_id, near)."""
        K = self.skeleton["num_kpt_types"]
        kp = np.ascontiguousarray(keypoints, dtype=np.int32).reshape(-1, K, 2)
        conf = np.ascontiguousarray(confidence, dtype=np.float64).reshape(-1)
        n = len(kp)
        if len(conf) != n:
            raise ValueError("%d poses but %d confidences" % (n, len(conf)))
        okp, obb, oid = np.zeros((n, K, 2), np.int32), np.zeros((n, 4), np.int32), np.zeros(n, np.int32)
        last, near = C.c_int(), C.c_uint()
        self._call("lwp_track_poses", int(lane), n, kp.ctypes.data, conf.ctypes.data, okp.ctypes.data, obb.ctypes.data, oid.ctypes.data,
                   C.byref(last), C.byref(near))
        return dict(keypoints=okp, bbox=obb, ids=oid, last_id=last.value, near=near.value)

    # ------------------------------------------------------------------ pose overlay on the device (demo.py:119-124)
    OVERLAY_OFF, OVERLAY_DEVICE, OVERLAY_HOST = 0, 1, 2

    def set_overlay(self, mode, color=None, box_color=None, boxes=True, n_draw_limbs=-1):
        """Skeletons, the 0.6 / 0.4 blend and the boxes of demo.py:119-124 drawn by kernels behind the pose tail of
        ``pipeline_submit_u8``: mode 0 off (default), 1 annotated frames kept on the device, 2 also copied to pinned host memory
        with the slot's results (``pipeline_overlay``).  ``color`` / ``box_color``: 3 bytes in the frame's channel order, None =
        ``Pose.color`` / (0, 255, 0); ``n_draw_limbs``: the first rows of the engine's limb table that are drawn, -1 = all but
        the last two.  Everything but the mode also applies to ``draw_poses``.  The id label (cv2.putText) is not drawn."""
        mode = {"off": 0, "device": 1, "host": 2}.get(mode, mode)

        def rgb(c):
            if c is None:
                return None
            v = [int(x) for x in c]
            if len(v) != 3 or min(v) < 0 or max(v) > 255:
                raise ValueError("a colour is 3 values in 0..255, got %r" % (c,))
            return (C.c_ubyte * 3)(*v)
        self._call("lwp_set_overlay", int(mode), rgb(color), rgb(box_color), 1 if boxes else 0, int(n_draw_limbs))
        self._overlay_mode = int(mode)

    def draw_poses(self, imgs, keypoints, bbox, n_poses=None, device_out=None):
        """The overlay kernels on poses the caller supplies.  ``imgs``: one frame (H,W,3) or a batch (N,H,W,3), uint8, numpy or
        a cuda tensor.  One frame: ``keypoints`` (P,K,2) and ``bbox`` (P,4) int32.  A batch: padded arrays (N,cap,K,2) / (N,cap,4)
        with ``n_poses`` (N,), or a list of N (P_f,K,2) arrays and a list of N (P_f,4) arrays.  Returns the annotated frames as a
        NEW array of the input's shape; ``imgs`` is not modified.  ``device_out``: None = the kind of ``imgs``, True = a cuda
        tensor, False = a numpy array."""
        ptr, mem, N, H, W, a = self._u8_frames(imgs)
        single = len(a.shape) == 3
        K = self.skeleton["num_kpt_types"]
        if single or n_poses is None:
            kl = [keypoints] if single else list(keypoints)
            bl = [bbox] if single else list(bbox)
            if len(kl) != N or len(bl) != N:
                raise ValueError("%d frames but %d key-point arrays and %d box arrays" % (N, len(kl), len(bl)))
            kl = [np.asarray(k, dtype=np.int32).reshape(-1, K, 2) for k in kl]
            bl = [np.asarray(b, dtype=np.int32).reshape(-1, 4) for b in bl]
            for k, b in zip(kl, bl):
                if len(k) != len(b):
                    raise ValueError("%d poses but %d boxes" % (len(k), len(b)))
            n = np.array([len(k) for k in kl], np.int32)
            cap = int(n.max()) if N else 0
            kp = np.full((N, cap, K, 2), -1, np.int32)
            bb = np.zeros((N, cap, 4), np.int32)
            for f in range(N):
                kp[f, :n[f]] = kl[f]
                bb[f, :n[f]] = bl[f]
        else:
            kp = np.ascontiguousarray(keypoints, dtype=np.int32)
            bb = np.ascontiguousarray(bbox, dtype=np.int32)
            n = np.ascontiguousarray(n_poses, dtype=np.int32).reshape(-1)
            if kp.ndim != 4 or kp.shape[0] != N or kp.shape[2:] != (K, 2) or bb.shape != (N, kp.shape[1], 4) or n.shape != (N,):
                raise ValueError("expected keypoints (N,cap,%d,2), bbox (N,cap,4) and n_poses (N,) for %d frames" % (K, N))
            cap = int(kp.shape[1])
        optr, omem, out = self._u8_out(tuple(a.shape), (mem == MEM_DEVICE) if device_out is None else bool(device_out))
        if mem == MEM_DEVICE or omem == MEM_DEVICE:
            self._order()
        self._call("lwp_draw_poses", ptr, mem, N, H, W, n.ctypes.data, kp.ctypes.data, bb.ctypes.data, cap, optr, omem)
        return out

    def _u8_out(self, shape, on_device):
        """(pointer, mem flag, the array) of a new uint8 array of ``shape``: a cuda tensor or a numpy array."""
        return self._ptr(self._empty(shape, _torch().uint8) if on_device else np.empty(shape, np.uint8))

    def pipeline_overlay(self, slot, device=False):
        """The annotated frames (N,H,W,3) uint8 of a fetched slot that was submitted with the overlay on: a numpy array (from the
        pinned copy in mode 2), or with ``device=True`` a cuda tensor.  A new array each time."""
        if slot not in self._overlay_shape:
            raise RuntimeError("slot %r holds no frames: call pipeline_submit_u8 for it first" % (slot,))
        shape = self._overlay_shape[slot]
        ptr, mem, out = self._u8_out(shape, device)
        if device:
            self._order()
        self._call("lwp_get_overlay", slot, ptr, mem, shape[0], shape[1], shape[2])
        return out

    # ------------------------------------------------------------------ training targets and loss (coco.py:48-61,71-159; loss.py)
    def train_targets(self, kpts, n_persons, image_hw, stride=8, sigma=7, paf_thickness=1, time_iters=0):
        """Key-point and PAF target maps rendered on the device.  ``kpts``: (N, Pmax, K, 3) float64 rows (x, y, visibility),
        numpy or a cuda tensor, persons in label order; ``n_persons``: (N,) counts; ``image_hw``: (H, W) of the frames.
        Returns float32 cuda tensors ``keypoint_maps`` (N, K + 1, H // stride, W // stride) and ``paf_maps`` (N, 2L, ...) for
        the engine's skeleton (``set_skeleton``; the default gives coco.py's channel layout).  With ``time_iters`` > 0 the
        kernel is launched that many times back to back and the call returns the milliseconds of all of them (HIP events)."""
        H, W = int(image_hw[0]), int(image_hw[1])
        sk = self.skeleton
        K, L = sk["num_kpt_types"], len(sk["limb_kpts"])
        ptr, mem, a = self._ptr(kpts, np.float64, "kpts")
        if len(a.shape) != 4 or tuple(a.shape[2:]) != (K, 3):
            raise ValueError("expected key-points of shape (N, Pmax, %d, 3), got %s" % (K, tuple(a.shape)))
        N, Pmax = int(a.shape[0]), int(a.shape[1])
        n = np.ascontiguousarray(n_persons, dtype=np.int32).reshape(-1)
        if n.shape != (N,):
            raise ValueError("expected %d person counts, got %s" % (N, n.shape))
        stride = _stride(stride)
        kmaps = self._empty((N, K + 1, H // stride, W // stride))
        pmaps = self._empty((N, 2 * L, H // stride, W // stride))
        self._order()
        args = (ptr if Pmax else None, mem, n.ctypes.data, N, Pmax, H, W, stride, float(sigma), float(paf_thickness),
                kmaps.data_ptr(), pmaps.data_ptr())
        ms = self._timed("lwp_train_targets", "lwp_time_train_targets", args, time_iters)
        return (kmaps, pmaps) if ms is None else ms

    def mask_downsample(self, mask, stride=8):
        """(N, H, W) or (H, W) float32 mask (numpy or cuda tensor) -> the mean of each stride x stride block as a float32 cuda
        tensor (N, H // stride, W // stride): cv2.resize(mask, fx=fy=1/stride, INTER_AREA) of coco.py:48 where H and W are
        multiples of the stride (ValueError otherwise)."""
        ptr, mem, a = self._ptr(mask, np.float32, "mask")
        single = len(a.shape) == 2
        if len(a.shape) not in (2, 3):
            raise ValueError("expected a mask of shape (N, H, W) or (H, W), got %s" % (tuple(a.shape),))
        N = 1 if single else int(a.shape[0])
        H, W = int(a.shape[-2]), int(a.shape[-1])
        stride = _stride(stride)
        out = self._empty((N, H // stride, W // stride))
        self._order()
        self._call("lwp_mask_downsample", ptr, mem, N, H, W, stride, out.data_ptr())
        return out[0] if single else out

    # ------------------------------------------------------------------ training augmentation (datasets/transformations.py)
    def augment_batch(self, samples_or_plan, transforms=None, rng=None, stride=8, time_iters=0):
        """The pixels of a batch of augmented training samples in one kernel launch.  ``samples_or_plan``: a
        ``datasets.transformations.BatchPlan``, or the raw samples with ``transforms`` (and ``rng``) for ``plan_batch``.
        Sources may be NumPy arrays (packed, one upload for the batch) or cuda uint8 / float32 tensors (read in place).
        Returns four cuda tensors: ``image`` (N, 3, cy, cx) float32 = (pixel - 128) / 256, ``mask`` (N, cy, cx) uint8,
        ``mask_small`` (N, cy // stride, cx // stride) float32 (coco.py:48 on the uint8 mask) and ``kpts`` (N, Pmax, 18, 3)
        float64, the transformed key-points as ``train_targets`` takes them (person counts: the plan's ``n_persons``).  Where a
        sample carries ``"segmentations"`` (crowd RLE dicts) instead of a float mask, its mask is rendered on the device from the
        runs (``lwp_augment_batch_crowd``) and read in place; a batch without any takes ``lwp_augment_batch``.  With
        ``time_iters`` > 0 the kernels are launched that many times back to back and the call returns their milliseconds."""
        torch = _torch()
        from ._lib import AugmentPlan
        from .datasets.transformations import BatchPlan, plan_batch
        if not isinstance(samples_or_plan, BatchPlan) and transforms is None:
            raise ValueError("raw samples need the transforms to plan them with")
        plan = samples_or_plan if isinstance(samples_or_plan, BatchPlan) else plan_batch(samples_or_plan, transforms, rng)
        N = len(plan)
        cy, cx = plan.crop_hw
        stride = _stride(stride)
        recs = (AugmentPlan * N)()
        keep = []                                      # the arrays the records point into, alive until the call returns
        for n, g in enumerate(plan.records):
            img, msk = plan.images[n], plan.masks[n]
            on_device = getattr(img, "is_cuda", False)
            if msk is not None and getattr(msk, "is_cuda", False) != on_device:
                raise ValueError("sample %d: the image and its mask must both be host arrays or both cuda tensors" % n)
            if on_device:
                if img.dtype != torch.uint8 or (msk is not None and msk.dtype != torch.float32):
                    raise TypeError("sample %d: cuda sources must be a uint8 image and a float32 mask" % n)
            elif np.asarray(img).dtype != np.uint8:
                raise TypeError("sample %d: the image must be uint8, got %s" % (n, np.asarray(img).dtype))
            r = recs[n]
            r.image, r.mem, img = self._ptr(img, np.uint8, "sample %d: the image" % n)
            r.mask, _, msk = (None, None, None) if msk is None else self._ptr(msk, np.float32, "sample %d: the mask" % n)
            keep.append((img, msk))
            r.rs_scale = float(g["rs_scale"])
            for i in range(6):
                r.m[i] = float(g["minv"][i])
            r.src_h, r.src_w, r.rs_h, r.rs_w, r.area = g["src_h"], g["src_w"], g["rs_h"], g["rs_w"], int(g["area"])
            r.bound_h, r.bound_w, r.should_crop = g["bound_h"], g["bound_w"], int(g["should_crop"])
            r.dst_y0, r.dst_y1, r.dst_x0, r.dst_x1 = g["dst"]
            r.img_y0, r.img_x0 = g["src0"]
            r.flip = int(g["flip"])
            for c in range(3):
                r.warp_pad[c], r.crop_pad[c] = int(g["warp_pad"][c]), int(g["crop_pad"][c])
        image = self._empty((N, 3, cy, cx))
        mask = self._empty((N, cy, cx), torch.uint8)
        small = self._empty((N, cy // stride, cx // stride))
        self._order()
        args = (recs, N, cy, cx, stride, image.data_ptr(), mask.data_ptr(), small.data_ptr())
        ms = None
        if getattr(plan, "crowd_runs", None) is not None:
            if time_iters:
                raise ValueError("a batch with segmentations has no timing twin: time crowd_masks, and augment_batch without them")
            self._call("lwp_augment_batch_crowd", *args[:5], *[a.ctypes.data for a in plan.crowd_runs], *args[5:])
        else:
            ms = self._timed("lwp_augment_batch", "lwp_time_augment_batch", args, time_iters)
        return (image, mask, small, torch.from_numpy(plan.kpts).to(self._gpu)) if ms is None else ms

    def crowd_masks(self, segmentations_per_image, sizes, time_iters=0):
        """``get_mask`` (coco.py:17-21) of all-ones masks for a batch, in one kernel launch.  ``segmentations_per_image``: per
        image a list of uncompressed RLE dicts (possibly empty); ``sizes``: per image (height, width).  Returns a list of
        (H, W) float32 cuda tensors, views of ONE buffer: 1 where no segmentation covers the pixel, 0 where any does.  With
        ``time_iters`` > 0 the kernel is launched that many times back to back and the call returns the milliseconds of all of
        them (HIP events)."""
        from .datasets.coco import pack_crowd_runs
        sizes = [(int(h), int(w)) for h, w in sizes]
        counts, seg_off, image_seg_off = pack_crowd_runs(segmentations_per_image, sizes)
        N = len(sizes)
        heights = np.array([h for h, _ in sizes], dtype=np.int32)
        widths = np.array([w for _, w in sizes], dtype=np.int32)
        out_off = np.zeros(N + 1, dtype=np.int64)
        np.cumsum(heights.astype(np.int64) * widths, out=out_off[1:])
        buf = self._empty((max(int(out_off[-1]), 1),))
        self._order()
        args = (counts.ctypes.data, seg_off.ctypes.data, image_seg_off.ctypes.data, heights.ctypes.data, widths.ctypes.data, N,
                out_off.ctypes.data, buf.data_ptr())
        ms = self._timed("lwp_crowd_masks", "lwp_time_crowd_masks", args, time_iters)
        if ms is not None:
            return ms
        return [buf[int(out_off[n]):int(out_off[n + 1])].view(h, w) for n, (h, w) in enumerate(sizes)]

    # ------------------------------------------------------------------ JPEG files (cv2.imread's place)
    @staticmethod
    def jpeg_info(data):
        """The header of one baseline JPEG file (``bytes``): a dict of lwp_jpeg_header's fields (width, height, components,
        per-component sampling and quantisation table, restart interval, MCU and block counts, the Exif orientation or 0).
        Needs no GPU.  ValueError, naming the reason and the byte offset, for a file outside the scope (include/lwpose.h)."""
        data = bytes(data)
        hd = _lib.JpegHeader()
        check(lib().lwp_jpeg_info(data, len(data), C.byref(hd)))
        n = hd.components
        return {"width": hd.width, "height": hd.height, "components": n, "h_samp": list(hd.h_samp)[:n], "v_samp": list(hd.v_samp)[:n],
                "quant_table": list(hd.quant_table)[:n], "restart_interval": hd.restart_interval, "mcus_x": hd.mcus_x,
                "mcus_y": hd.mcus_y, "orientation": hd.orientation, "blocks_w": list(hd.blocks_w)[:n],
                "blocks_h": list(hd.blocks_h)[:n], "total_blocks": hd.total_blocks}

    @staticmethod
    def debug_jpeg_blocks(data):
        """The host half alone (tests; no GPU): (header dict, coefficients int16 (total_blocks, 64) in natural order and plane
        order, quantisation tables uint16 (4, 64) in natural order)."""
        data = bytes(data)
        hd = Engine.jpeg_info(data)
        coef = np.empty((hd["total_blocks"], 64), dtype=np.int16)
        qt = np.empty((4, 64), dtype=np.uint16)
        check(lib().lwp_debug_jpeg_blocks(data, len(data), coef.ctypes.data, coef.size, qt.ctypes.data))
        return hd, coef, qt

    def set_jpeg_entropy(self, mode, subseq_bytes=0):
        """Where ``decode_jpeg_batch`` decodes the Huffman data: ``"host"`` (the default) or ``"device"`` (the same
        pixels, refusals and messages).  ``subseq_bytes``: the bytes of a scan one lane owns, 0 (the default) or a multiple of 4
        from 4 to 1024.  ValueError for anything else."""
        if mode not in _lib.JPEG_ENTROPY_MODES:
            raise ValueError("entropy mode must be 'host' or 'device', not %r" % (mode,))
        self._call("lwp_set_jpeg_entropy", _lib.JPEG_ENTROPY_MODES[mode], int(subseq_bytes))
        self._jpeg_entropy, self._jpeg_subseq = mode, int(subseq_bytes)

    @staticmethod
    def _jpeg_args(files):
        N = len(files)
        data = (C.c_void_p * N)(*[C.cast(C.c_char_p(f), C.c_void_p) for f in files])
        lens = (C.c_size_t * N)(*[len(f) for f in files])
        return data, lens

    def debug_jpeg_entropy(self, files, subseq_bytes=0, time_iters=0):
        """The device entropy decoder alone (tests): ``[(status, coef or None, qtables or None)]`` per file, status 0 for an
        accepted file, whose coefficients and tables are laid out as ``debug_jpeg_blocks`` returns them; a refused file does not
        fail the call.  With ``time_iters`` > 0: (milliseconds of that many back-to-back runs of the kernels, the most sync rounds
        inside a workgroup, the most across workgroups)."""
        files = [bytes(f) for f in files]
        N = len(files)
        if N == 0:
            return []
        data, lens = self._jpeg_args(files)
        self._order()
        if time_iters:
            ms, rounds = C.c_float(), (C.c_int * 2)()
            self._call("lwp_time_jpeg_entropy_batch", N, data, lens, int(subseq_bytes), int(time_iters), C.byref(ms), rounds)
            return ms.value, rounds[0], rounds[1]
        coefs, qts = [], []
        for f in files:
            hd = _lib.JpegHeader()
            blocks = 0 if lib().lwp_jpeg_info(f, len(f), C.byref(hd)) else hd.total_blocks
            coefs.append(np.zeros((max(blocks, 1), 64), dtype=np.int16))
            qts.append(np.zeros((4, 64), dtype=np.uint16))
        cp = (C.c_void_p * N)(*[c.ctypes.data for c in coefs])
        qp = (C.c_void_p * N)(*[q.ctypes.data for q in qts])
        status = (C.c_int * N)()
        self._call("lwp_debug_jpeg_entropy_batch", N, data, lens, int(subseq_bytes), cp, qp, status)
        return [(int(status[i]), None, None) if status[i] else (0, coefs[i], qts[i]) for i in range(N)]

    @staticmethod
    def debug_jpeg_scan(data):
        """The host pre-pass of the device entropy decoder alone (tests; no GPU): a dict of ``status`` (0 accepted so far,
        1 refused, 2 too long for device mode), ``bytes`` (the un-stuffed scan), ``segments`` (uint32 (n, 4): byte offset, byte
        length, first MCU, MCU count), ``tables`` (the six flattened Huffman tables, uint8 (6, 1488)) and ``qtables`` (uint16
        (4, 64)).  ValueError if the header itself is refused."""
        data = bytes(data)
        hd = Engine.jpeg_info(data)
        n_mcus = hd["mcus_x"] * hd["mcus_y"]
        cap = -(-n_mcus // hd["restart_interval"]) if hd["restart_interval"] else 1
        out = np.zeros(len(data) + 8, dtype=np.uint8)
        segs = np.zeros((cap, 4), dtype=np.uint32)
        tables = np.zeros((6, 1488), dtype=np.uint8)
        qt = np.zeros((4, 64), dtype=np.uint16)
        nb, ns, status = C.c_size_t(), C.c_size_t(), C.c_int()
        check(lib().lwp_debug_jpeg_scan(data, len(data), out.ctypes.data, out.size, C.byref(nb), segs.ctypes.data, cap, C.byref(ns),
                                        tables.ctypes.data, qt.ctypes.data, C.byref(status)))
        return {"status": status.value, "bytes": out[:nb.value].tobytes(), "segments": segs[:ns.value].copy(), "tables": tables, "qtables": qt}

    def decode_jpeg_batch(self, files, time_iters=0, entropy=None):
        """``cv2.imread(.., IMREAD_COLOR)`` of a batch of baseline JPEG files (a list of ``bytes``), decoded in ONE device call:
        the Huffman data on the host, inverse DCT, up-sampling, colour conversion and the BGR store on the GPU, files of different
        sizes and samplings mixed.  Returns a list of cuda uint8 (H, W, 3) tensors, views of one allocation.  ValueError with the
        file's index for one outside the scope; nothing is written then.  The Exif orientation is not applied.  With
        ``time_iters`` > 0 each of the two kernels is launched that many times back to back and the call returns their
        milliseconds (stage A, stage B).  ``entropy``: ``"host"`` or ``"device"`` for this call, None for the engine's setting
        (``set_jpeg_entropy``; the host unless set)."""
        if entropy is not None and entropy != self._jpeg_entropy:
            if entropy not in _lib.JPEG_ENTROPY_MODES:
                raise ValueError("entropy mode must be 'host' or 'device', not %r" % (entropy,))
            self._call("lwp_set_jpeg_entropy", _lib.JPEG_ENTROPY_MODES[entropy], self._jpeg_subseq)
            try:
                return self.decode_jpeg_batch(files, time_iters)
            finally:
                self._call("lwp_set_jpeg_entropy", _lib.JPEG_ENTROPY_MODES[self._jpeg_entropy], self._jpeg_subseq)
        files = [bytes(f) for f in files]
        N = len(files)
        if N == 0:
            return []
        sizes = []
        for i, f in enumerate(files):
            hd = _lib.JpegHeader()
            rc = lib().lwp_jpeg_info(f, len(f), C.byref(hd))
            if rc:
                raise ValueError("image %d: %s" % (i, lib().lwp_last_error(None).decode("utf-8", "replace")))
            sizes.append((hd.height, hd.width))
        off = np.zeros(N + 1, dtype=np.int64)           # every image starts on a 16-byte boundary of the allocation
        for i, (h, w) in enumerate(sizes):
            off[i + 1] = (off[i] + h * w * 3 + 15) // 16 * 16
        buf = self._empty((int(off[-1]),), _torch().uint8)
        data, lens = self._jpeg_args(files)
        outs = (C.c_void_p * N)(*[buf.data_ptr() + int(off[i]) for i in range(N)])
        self._order()
        ms = self._timed("lwp_jpeg_decode_batch", "lwp_time_jpeg_decode_batch", (N, data, lens, outs), time_iters, n_ms=2)
        if ms is not None:
            return ms
        return [buf[int(off[i]):int(off[i]) + h * w * 3].view(h, w, 3) for i, (h, w) in enumerate(sizes)]

    # ------------------------------------------------------------------ JPEG files, written (cv2.imwrite's place)
    @staticmethod
    def _jpeg_encode_options(quality, subsampling, restart_interval):
        if isinstance(quality, bool) or not isinstance(quality, (int, np.integer)) or not 1 <= quality <= 100:
            raise ValueError("quality must be an integer from 1 to 100, not %r" % (quality,))
        if subsampling not in _lib.JPEG_SUBSAMPLINGS:
            raise ValueError("subsampling must be '4:4:4', '4:2:2' or '4:2:0', not %r" % (subsampling,))
        if (isinstance(restart_interval, bool) or not isinstance(restart_interval, (int, np.integer))
                or not 0 <= restart_interval <= 65535):
            raise ValueError("restart_interval must be an integer from 0 to 65535 MCUs, not %r" % (restart_interval,))
        return int(quality), _lib.JPEG_SUBSAMPLINGS[subsampling], int(restart_interval)

    @staticmethod
    def jpeg_encode_bound(height, width, subsampling="4:2:0", restart_interval=0):
        """Bytes that hold the file ``encode_jpeg_batch`` writes of a height x width frame, whatever its pixels.  Needs no GPU."""
        _, sub, ri = Engine._jpeg_encode_options(75, subsampling, restart_interval)
        n = C.c_size_t()
        check(lib().lwp_jpeg_encode_bound(int(height), int(width), sub, ri, C.byref(n)))
        return n.value

    @staticmethod
    def debug_jpeg_encode_header(height, width, quality=75, subsampling="4:2:0", restart_interval=0):
        """The header bytes alone (tests; no GPU): SOI up to and including SOS, in Pillow's layout."""
        q, sub, ri = Engine._jpeg_encode_options(quality, subsampling, restart_interval)
        out = np.empty(640, dtype=np.uint8)
        n = C.c_size_t()
        check(lib().lwp_debug_jpeg_encode_header(int(height), int(width), q, sub, ri, out.ctypes.data, out.size, C.byref(n)))
        return out[:n.value].tobytes()

    def _jpeg_frames(self, frames):
        """(N, frame pointers, MEM_HOST or MEM_DEVICE, heights, widths, the objects behind the pointers) of a list of (H, W, 3)
        uint8 arrays or cuda tensors, or of one (N, H, W, 3) batch.  Cuda tensors are read in place; a mix of host and device
        frames, another type or another shape is a ValueError."""
        if hasattr(frames, "ndim") and not isinstance(frames, (list, tuple)):
            if frames.ndim != 4:
                raise ValueError("a batch of frames must be (N, H, W, 3), not %s" % (tuple(frames.shape),))
            frames = [frames[i] for i in range(frames.shape[0])]
        frames = list(frames)
        if not frames:
            return 0, None, MEM_HOST, None, None, []
        keep, mems = [], set()
        for i, f in enumerate(frames):
            if not hasattr(f, "shape") or len(f.shape) != 3 or f.shape[2] != 3:
                raise ValueError("frame %d must be (H, W, 3), not %s" % (i, tuple(getattr(f, "shape", ()))))
            if not hasattr(f, "dtype") or not _is_dtype(f, np.uint8):
                raise ValueError("frame %d must be uint8, not %s" % (i, f.dtype))
            if f.shape[0] < 1 or f.shape[1] < 1 or f.shape[0] > 65535 or f.shape[1] > 65535:
                raise ValueError("frame %d: %d x %d: height and width must be 1..65535" % (i, f.shape[0], f.shape[1]))
            ptr, mem, a = self._ptr(f, np.uint8, "frames", convert=False)
            keep.append((ptr, a))
            mems.add(mem)
        if len(mems) != 1:
            raise ValueError("frames must all be host arrays or all be cuda tensors")
        N = len(keep)
        ptrs = (C.c_void_p * N)(*[p for p, _ in keep])
        heights = (C.c_int * N)(*[int(f.shape[0]) for f in frames])
        widths = (C.c_int * N)(*[int(f.shape[1]) for f in frames])
        return N, ptrs, mems.pop(), heights, widths, keep

    def encode_jpeg_batch(self, frames, quality=75, subsampling="4:2:0", restart_interval=0, time_iters=0):
        """``cv2.imencode('.jpg', ..)`` of a batch of BGR frames in ONE device call: colour conversion, down-sampling, forward
        DCT, quantisation, Huffman coding and byte stuffing all run on the GPU, and only the compressed bytes come back.
        ``frames``: a list of (H, W, 3) uint8 arrays (uploaded in one copy) or cuda tensors (read in place), sizes mixed, or one
        (N, H, W, 3) batch.  ``quality`` 1..100, ``subsampling`` '4:4:4' | '4:2:2' | '4:2:0', ``restart_interval`` in MCUs
        (0: none); anything else is a ValueError.  Returns a list of ``bytes``: baseline JFIF files, byte for byte what Pillow
        (libjpeg-turbo) writes of the same pixels with these settings; cv2 itself is not pinned.  With ``time_iters`` > 0 each
        of the six stages is launched that many times back to back and the call returns their milliseconds."""
        q, sub, ri = self._jpeg_encode_options(quality, subsampling, restart_interval)
        N, ptrs, mem, heights, widths, keep = self._jpeg_frames(frames)
        if N == 0:
            return []
        self._order()
        if time_iters:
            ms = (C.c_float * 6)()
            self._call("lwp_time_jpeg_encode_batch", N, ptrs, mem, heights, widths, q, sub, ri, int(time_iters), ms)
            return tuple(ms)
        bounds = [self.jpeg_encode_bound(heights[i], widths[i], subsampling, ri) for i in range(N)]
        off = np.zeros(N + 1, dtype=np.int64)
        np.cumsum(bounds, out=off[1:])
        buf = np.empty(int(off[-1]), dtype=np.uint8)     # untouched pages cost nothing: files take a fraction of the bound
        outs = (C.c_void_p * N)(*[buf.ctypes.data + int(off[i]) for i in range(N)])
        caps = (C.c_size_t * N)(*bounds)
        lens = (C.c_size_t * N)()
        self._call("lwp_jpeg_encode_batch", N, ptrs, mem, heights, widths, q, sub, ri, outs, caps, lens)
        del keep
        return [buf[int(off[i]):int(off[i]) + lens[i]].tobytes() for i in range(N)]

    def debug_jpeg_encode_blocks(self, frames, quality=75, subsampling="4:2:0"):
        """The first stage alone (tests): ``[(coefficients int16 (total_blocks, 64))]`` per frame in the decoder's layout
        (natural order, plane order, MCU-padded grids), and the quantisation tables uint16 (4, 64) of the batch."""
        q, sub, _ = self._jpeg_encode_options(quality, subsampling, 0)
        N, ptrs, mem, heights, widths, keep = self._jpeg_frames(frames)
        coefs = []
        for i in range(N):
            hd = self.jpeg_info(self.debug_jpeg_encode_header(heights[i], widths[i], q, subsampling))
            coefs.append(np.zeros((hd["total_blocks"], 64), dtype=np.int16))
        qt = np.zeros((4, 64), dtype=np.uint16)
        if N:
            self._order()
            cp = (C.c_void_p * N)(*[c.ctypes.data for c in coefs])
            self._call("lwp_debug_jpeg_encode_blocks", N, ptrs, mem, heights, widths, q, sub, cp, qt.ctypes.data)
        return coefs, qt

    @staticmethod
    def _jpeg_scan_args(coefs, sizes, subsampling, restart_interval):
        """The checks of ``debug_jpeg_encode_scan`` that need no device: (contiguous int16 arrays, heights, widths, the
        library's subsampling number, the restart interval).  A coefficient array of another type than int16 (nothing is
        converted: a wrapped value would be coded as if it were meant) or another shape than (total_blocks, 64) of its size,
        or another number of sizes than of arrays, is a ValueError."""
        _, sub, ri = Engine._jpeg_encode_options(75, subsampling, restart_interval)
        coefs, sizes = list(coefs), list(sizes)
        if len(sizes) != len(coefs):
            raise ValueError("%d sizes for %d coefficient arrays" % (len(sizes), len(coefs)))
        arrs, heights, widths = [], [], []
        for i, (c, hw) in enumerate(zip(coefs, sizes)):
            if len(tuple(hw)) != 2:
                raise ValueError("size %d must be (H, W), not %r" % (i, hw))
            H, W = int(hw[0]), int(hw[1])
            if H < 1 or W < 1 or H > 65535 or W > 65535:
                raise ValueError("size %d: %d x %d: height and width must be 1..65535" % (i, H, W))
            if not isinstance(c, np.ndarray) or c.dtype != np.int16:
                raise ValueError("coefficients %d must be an int16 array, not %s" % (i, getattr(c, "dtype", type(c).__name__)))
            blocks = Engine.jpeg_info(Engine.debug_jpeg_encode_header(H, W, 75, subsampling))["total_blocks"]
            if c.shape != (blocks, 64):
                raise ValueError("coefficients %d must be (%d, 64) for %d x %d at %s, not %s" % (i, blocks, H, W, subsampling, c.shape))
            arrs.append(np.ascontiguousarray(c))
            heights.append(H)
            widths.append(W)
        return arrs, heights, widths, sub, ri

    def debug_jpeg_encode_scan(self, coefs, sizes, subsampling="4:2:0", restart_interval=0):
        """The stages behind the first alone (tests): the entropy-coded, stuffed scans (``bytes``, RSTn markers included, no
        header and no EOI) of the caller's coefficients.  ``coefs``: int16 arrays (total_blocks, 64) in the layout
        ``debug_jpeg_encode_blocks`` returns; ``sizes``: their (H, W).  A DC outside -1024..1023 or an AC term outside
        -1023..1023 is a ValueError that names the image."""
        arrs, heights, widths, sub, ri = self._jpeg_scan_args(coefs, sizes, subsampling, restart_interval)
        N = len(arrs)
        if N == 0:
            return []
        bounds = [self.jpeg_encode_bound(heights[i], widths[i], subsampling, ri) for i in range(N)]
        off = np.zeros(N + 1, dtype=np.int64)
        np.cumsum(bounds, out=off[1:])
        buf = np.zeros(int(off[-1]), dtype=np.uint8)
        cp = (C.c_void_p * N)(*[a.ctypes.data for a in arrs])
        outs = (C.c_void_p * N)(*[buf.ctypes.data + int(off[i]) for i in range(N)])
        caps = (C.c_size_t * N)(*bounds)
        lens = (C.c_size_t * N)()
        self._order()
        self._call("lwp_debug_jpeg_encode_scan", N, cp, (C.c_int * N)(*heights), (C.c_int * N)(*widths), sub, ri, outs, caps, lens)
        return [buf[int(off[i]):int(off[i]) + lens[i]].tobytes() for i in range(N)]

    def stage_losses(self, outs, keypoint_maps, paf_maps, mask, batch_size=None, time_iters=0):
        """train.py:92-97's per-stage sums: ``outs`` is the list net(x) returned (cuda tensors; an entry may be None),
        ``keypoint_maps`` / ``paf_maps`` the targets, ``mask`` one (N, h, w) cuda tensor broadcast over the channels.
        Returns 2 * (nref + 1) Python floats, loss[i] = sum(((outs[i] - target) * mask)**2 / 2 / batch_size) in float64;
        two calls on the same inputs return the same bits.  Tensors are read as contiguous NCHW float32: a strided view is
        copied first (``Engine.forward`` returns contiguous tensors, which are read in place).  With ``time_iters`` > 0 the
        kernels are launched that many times back to back and the call returns the milliseconds of all of them (HIP events)."""
        args, n = self._loss_args(outs, keypoint_maps, paf_maps, mask, batch_size)
        losses = (C.c_double * max(n, 1))()
        ms = self._timed("lwp_stage_losses", "lwp_time_stage_losses", args, time_iters, tail=(losses,))
        return [float(losses[i]) for i in range(n)] if ms is None else ms

    def _loss_args(self, outs, keypoint_maps, paf_maps, mask, batch_size):
        """The leading arguments of lwp_stage_losses / lwp_stage_losses_log and the number of stage tensors; the contiguous
        tensors behind the pointers are kept on the engine until the next loss call."""
        ref = next((o for o in outs if o is not None), None)
        if ref is None:
            raise ValueError("no stage tensor given")
        N, _, hs, ws = (int(v) for v in ref.shape)
        keep = [self._dev32(o, "outs[%d]" % i, (N, self.NP if i % 2 else self.NH, hs, ws), True) for i, o in enumerate(outs)]
        km = self._dev32(keypoint_maps, "keypoint_maps", (N, self.NH, hs, ws), True)
        pm = self._dev32(paf_maps, "paf_maps", (N, self.NP, hs, ws), True)
        m = self._dev32(mask, "mask", (N, hs, ws), True)
        if m is None:
            raise ValueError("mask is None")
        ptrs = (C.c_void_p * max(len(keep), 1))(*[None if o is None else o.data_ptr() for o in keep])
        self._loss_keep = (keep, km, pm, m, ptrs)
        self._order()
        return (ptrs, len(keep), None if km is None else km.data_ptr(), None if pm is None else pm.data_ptr(), m.data_ptr(),
                N, hs, ws, int(N if batch_size is None else batch_size)), len(keep)

    def log_stage_losses(self, outs, keypoint_maps, paf_maps, mask, batch_size=None, divisor=1.0):
        """``stage_losses`` without the read: the same launches, and behind them, on the device, ``log[i] += loss[i] / divisor``
        in float64 (train.py:96-97's total_losses with divisor = batches_per_iter).  Returns None and does not wait for the
        GPU; ``read_loss_log`` fetches the running sums.  ``divisor`` must be finite and > 0 (ValueError)."""
        args, _ = self._loss_args(outs, keypoint_maps, paf_maps, mask, batch_size)
        self._call("lwp_stage_losses_log", *args, float(divisor))

    def read_loss_log(self, reset=True):
        """(the 2 * (nref + 1) running sums of ``log_stage_losses`` as Python floats, the number of adds since the last reset).
        Waits for the engine's stream: the one wait of a logged training loop.  ``reset`` zeroes both behind the read."""
        S = 2 * (self.nref + 1)
        sums, adds = (C.c_double * S)(), C.c_int64()
        self._call("lwp_loss_log_read", sums, C.byref(adds), 1 if reset else 0)
        return [float(sums[i]) for i in range(S)], int(adds.value)

    # ------------------------------------------------------------------ stage backward (train.py:99-103, fp32 engines)
    def train_forward(self, x):
        """``forward`` for a float32 cuda tensor (N, 3, H, W) that also keeps what ``stage_backward`` needs: every stage
        layer's output from cpm.conv on (from the cpm's input on in train scope "cpm", from model.0 on in scope "all").  Returns the same list of stage outputs, bit for bit."""
        x = self._as_device_input(x)
        N, _, H, W = (int(v) for v in x.shape)
        outs = [self._empty(s) for s in self._stage_shapes(N, H, W)]
        ptrs = (C.c_void_p * len(outs))(*[o.data_ptr() for o in outs])
        self._order(x.device)
        self._call("lwp_train_forward", x.data_ptr(), N, H, W, ptrs)
        return outs

    def set_backward_precision(self, precision="fp32", grad_scale=1.0):
        """The operand type of the dense-conv gradients' two MFMA products: ``"fp32"`` (the default: the f32 kernels and their
        bits), ``"bf16"`` or ``"fp16"`` (include/lwpose.h, "backward precision").  dZ is multiplied by ``grad_scale``, a
        power of two in [1, 2^24] (1 with "fp32"), in front of its rounding and the f32 accumulator by its inverse.  Everything
        else, the engine included, stays fp32; the setting may change between any two calls.  ValueError for anything else."""
        if precision not in _lib.BACKWARD_PRECISIONS:
            raise ValueError("backward precision must be 'fp32', 'bf16' or 'fp16', not %r" % (precision,))
        self._call("lwp_set_backward_precision", _lib.BACKWARD_PRECISIONS[precision], float(grad_scale))

    @property
    def backward_precision(self):
        """(name, grad_scale) as the handle holds them."""
        dt, sc = C.c_int(), C.c_double()
        self._call("lwp_get_backward_precision", C.byref(dt), C.byref(sc))
        return [k for k, v in _lib.BACKWARD_PRECISIONS.items() if v == dt.value][0], sc.value

    def set_train_scope(self, scope):
        """"stages" (the default): ``train_forward`` / ``stage_backward`` / ``adam_step`` cover initial_stage.* and
        refinement_stages.*; "cpm": the cpm (cpm.align, cpm.trunk, cpm.conv) as well, its ten parameters in front of the stage
        ones in every flat array, the backbone frozen; "all": the backbone model.* too (its 69 parameters in front of the cpm's;
        BatchNorm at its running statistics, which never move).  Raises RuntimeError once the optimiser has taken a step
        (``load_adam_state(None)`` first, or set the scope before the first step).  The retained forward is invalidated.
        Parameters the old scope has trained and the new one does not cover stay readable through ``trained_params``."""
        name = _lib.train_scope_name(scope)
        if name == self.train_scope:
            self._call("lwp_set_train_scope", _lib.train_scope(name))
            return
        old = self.stage_params() if self.stage_steps != self._scope_steps else {}
        self._call("lwp_set_train_scope", _lib.train_scope(name))
        self.train_scope = name
        self._gspec = None
        self._scope_steps = self.stage_steps
        covered = set(k for k, _, _ in self.grad_spec()[0])
        self._left_params.update((k, v.clone()) for k, v in old.items() if k not in covered)
        for k in covered:
            self._left_params.pop(k, None)

    def grad_spec(self):
        """([(state-dict key, shape, float offset)], total floats) of the flat gradient array, in the engine's train scope."""
        if self._gspec is None:
            self._gspec = _lib.train_grad_spec(self.train_scope, self.nref, self.C, self.NH, self.NP)
        return self._gspec

    def grad_views(self, flat):
        """dict key -> view of ``flat`` (the array ``stage_backward`` fills) with that parameter's shape."""
        return dict((k, flat[off:off + int(np.prod(shape))].view(shape)) for k, shape, off in self.grad_spec()[0])

    def _backward_args(self, keypoint_maps, paf_maps, mask, batch_size, loss_scale, flat, want_features):
        if not getattr(mask, "is_cuda", False) or mask.dim() != 3:
            raise ValueError("mask must be an (N, h, w) cuda tensor")
        N, hs, ws = (int(v) for v in mask.shape)
        km = self._dev32(keypoint_maps, "keypoint_maps", (N, self.NH, hs, ws))
        pm = self._dev32(paf_maps, "paf_maps", (N, self.NP, hs, ws))
        m = self._dev32(mask, "mask", (N, hs, ws))
        dfeat = self._empty((N, self.C, hs, ws)) if want_features else None
        self._keep = (km, pm, m)
        return (km.data_ptr(), pm.data_ptr(), m.data_ptr(), N, hs, ws, int(N if batch_size is None else batch_size),
                float(loss_scale)), flat, dfeat

    def stage_backward(self, keypoint_maps, paf_maps, mask, batch_size=None, loss_scale=1.0, into=None, want_features=True, want_backbone=False):
        """Gradients of L = loss_scale * sum of the per-stage masked L2 losses (train.py:99-102) of the last ``train_forward``:
        returns (grads, d_features).  ``grads`` maps every initial_stage.* / refinement_stages.* state-dict key that has a
        gradient to a cuda tensor of the parameter's shape, all views of one flat array (``flat_of(grads)``); ``d_features`` is dL / d backbone_features (N, num_channels, h, w).  ``into``: a flat array from an
        earlier call (``Engine.flat_of(grads)``) to add to, like loss.backward() accumulates over train.py:96's batches.
        The refinement BatchNorms stay at their running statistics: the reference network in eval() mode.
        In train scope "cpm" the dict holds the cpm.* keys too, and ``want_backbone=True`` returns a third value: the gradient
        at the cpm's input (N, 512, h, w).  Train scope "all" adds the model.* keys; there is no gradient at the image."""
        torch = _torch()
        total = self.grad_spec()[1]
        if into is not None and (not into.is_cuda or into.dtype != torch.float32 or into.numel() != total or not into.is_contiguous()):
            raise ValueError("into must be the contiguous float32 cuda array of %d gradients an earlier call returned" % total)
        flat = into if into is not None else self._empty(total)
        args, flat, dfeat = self._backward_args(keypoint_maps, paf_maps, mask, batch_size, loss_scale, flat, want_features)
        args += (1 if into is not None else 0, flat.data_ptr(), None if dfeat is None else dfeat.data_ptr())
        self._order()
        if want_backbone:
            dback = self._empty((int(mask.shape[0]), 512) + tuple(int(v) for v in mask.shape[1:]))
            self._call("lwp_train_backward", *args, dback.data_ptr())
            return self.grad_views(flat), dfeat, dback
        self._call("lwp_stage_backward", *args)
        return self.grad_views(flat), dfeat

    def flat_of(self, grads):
        """The flat array behind a dict ``stage_backward`` returned (to pass as ``into=``)."""
        flat = getattr(next(iter(grads.values())), "_base", None)
        if flat is None or flat.dim() != 1 or flat.numel() != self.grad_spec()[1]:
            raise ValueError("not a gradient dict of this engine's stage_backward")
        return flat

    def profile_stage_backward(self, keypoint_maps, paf_maps, mask, batch_size=None, loss_scale=1.0, reps=3):
        """Device milliseconds and launch counts of one backward by kernel class (HIP events around every launch)."""
        args, flat, dfeat = self._backward_args(keypoint_maps, paf_maps, mask, batch_size, loss_scale, self._empty(self.grad_spec()[1]), True)
        ms, n = (C.c_float * 4)(), (C.c_int * 4)()
        self._order()
        self._call("lwp_profile_stage_backward", *args, flat.data_ptr(), dfeat.data_ptr(), int(reps), ms, n)
        names = ("elementwise", "dgrad", "wgrad", "reduce")
        return dict((names[i], dict(ms=float(ms[i]), launches=int(n[i]))) for i in range(4))

    def cpm_activations(self):
        """Train scope "cpm": the retained cpm tensors of the last ``train_forward`` as NCHW float32 numpy, by the oracle's tap
        names: "model.11" (the cpm's input), "cpm.align", "cpm.trunk.j.dw", "cpm.trunk.j" (pointwise output after ELU, in front
        of the residual add for j = 2), "cpm.sum" and "cpm" (tests)."""
        layers = self.layers()
        by = dict((i["name"], i["index"]) for i in layers)
        out = {"model.11": self.train_activation(by["cpm.align"] - 1), "cpm.align": self.train_activation(by["cpm.align"]),
               "cpm": self.train_activation(by["cpm.conv"])}
        for j in range(3):
            pw = by["cpm.trunk.%d.pw" % j]
            dw = by.get("cpm.trunk.%d.dw" % j)
            out["cpm.trunk.%d.dw" % j] = self.train_activation(dw) if dw is not None else self.train_activation(pw, _lib.KEPT_DEPTHWISE)
            out["cpm.trunk.%d" % j] = self.train_activation(pw, _lib.KEPT_NO_RESIDUAL if j == 2 else _lib.KEPT_OUTPUT)
        out["cpm.sum"] = self.train_activation(by["cpm.trunk.2.pw"])
        return out

    def train_activation(self, layer_index, which=_lib.KEPT_OUTPUT):
        """Retained output of a layer from the last ``train_forward`` as NCHW float32 numpy (tests): a stage layer or cpm.conv,
        in train scope "cpm" also a cpm layer or the backbone's last layer, in scope "all" any layer.  ``which``: ``_lib.KEPT_DEPTHWISE`` for the retained
        depthwise copy of a fused cpm trunk or backbone block (``cin`` channels), ``_lib.KEPT_NO_RESIDUAL`` for the block's output in
        front of its residual add."""
        info = self.layers()[layer_index]
        channels = info["cin"] if which == _lib.KEPT_DEPTHWISE else info["cout"]
        cap = 1 << 16
        dims = (C.c_int * 4)()
        while True:
            buf = np.empty(cap, np.float32)
            rc = lib().lwp_debug_train_copy(self.h.ptr, layer_index, which, buf.ctypes.data, buf.size, dims)
            if rc == _lib.LWP_ERR_ARG and lib().lwp_last_error(self.h.ptr) == b"dst too small" and cap < (1 << 31):
                cap *= 8
                continue
            check(rc, self.h.ptr)
            break
        n = dims[0] * dims[1] * dims[2] * dims[3]
        assert dims[1] == channels
        return buf[:n].reshape(dims[0], dims[1], dims[2], dims[3]).copy()

    def backbone_activations(self):
        """Train scope "all": the retained backbone tensors of the last ``train_forward`` as NCHW float32 numpy, by the oracle's
        tap names: "model.0", "model.i.dw" (a fused block's retained depthwise copy) and "model.i", i = 1..11 (tests)."""
        by = dict((i["name"], i["index"]) for i in self.layers())
        out = {"model.0": self.train_activation(by["model.0"])}
        for i in range(1, 12):
            pw = by["model.%d.pw" % i]
            dw = by.get("model.%d.dw" % i)
            out["model.%d.dw" % i] = self.train_activation(dw) if dw is not None else self.train_activation(pw, _lib.KEPT_DEPTHWISE)
            out["model.%d" % i] = self.train_activation(pw)
        return out

    def debug_dw_grad(self, dz, x, w, stride, dil, max_chunk=0):
        """The backbone's depthwise gradient kernels alone (tests): ``dz`` (N, C, Ho, Wo), ``x`` (N, C, H, W), ``w`` (C, 1, 3, 3)
        float32 cuda tensors -> (dx (N, C, H, W), G (C, 1, 3, 3), g (C,), pixel ranges taken)."""
        torch = _torch()
        N, Cn, H, W = (int(v) for v in x.shape)
        nhwc = lambda t: t.detach().to(torch.float32).permute(0, 2, 3, 1).contiguous()
        dzn, xn = nhwc(dz), nhwc(x)
        wt = w.detach().to(torch.float32).reshape(Cn, 9).t().contiguous()
        dx = torch.empty_like(xn)
        G = torch.empty((Cn, 1, 3, 3), dtype=torch.float32, device=xn.device)
        g = torch.empty(Cn, dtype=torch.float32, device=xn.device)
        splits = C.c_int()
        self._order()
        torch.cuda.synchronize()
        self._call("lwp_debug_dw_grad_sd", dzn.data_ptr(), xn.data_ptr(), wt.data_ptr(), N, H, W, Cn, int(stride), int(dil), int(max_chunk),
                   dx.data_ptr(), G.data_ptr(), g.data_ptr(), C.byref(splits))
        return dx.permute(0, 3, 1, 2).contiguous(), G, g, splits.value

    def debug_stem_wgrad(self, dz, x, max_chunk=0):
        """The stem's weight gradient kernel alone (tests): ``dz`` (N, 32, Ho, Wo), ``x`` (N, 3, H, W) -> (G (32, 3, 3, 3), g (32,), ranges)."""
        torch = _torch()
        N, _, H, W = (int(v) for v in x.shape)
        dzn = dz.detach().to(torch.float32).permute(0, 2, 3, 1).contiguous()
        xc = x.detach().to(torch.float32).contiguous()
        G = torch.empty((32, 3, 3, 3), dtype=torch.float32, device=xc.device)
        g = torch.empty(32, dtype=torch.float32, device=xc.device)
        splits = C.c_int()
        self._order()
        torch.cuda.synchronize()
        self._call("lwp_debug_stem_wgrad", dzn.data_ptr(), xc.data_ptr(), N, H, W, int(max_chunk), G.data_ptr(), g.data_ptr(), C.byref(splits))
        return G, g, splits.value

    # ------------------------------------------------------------------ the stage and cpm gradient kernels alone (tests)
    # NCHW float32 cuda tensors in and out; the kernels see NHWC rows.  `fill` is what the rows hold outside the tensor's window
    # (padding channels, GUARD_ROWS rows behind the last pixel); the rows come back whole so that a test can look there.
    GUARD_ROWS = 3

    @staticmethod
    def _rows(t, ld=None, off=0, fill=0.0, guard=0):
        torch = _torch()
        N, Cn, H, W = (int(v) for v in t.shape)
        rows = torch.full((N * H * W + guard, Cn if ld is None else int(ld)), float(fill), dtype=torch.float32, device=t.device)
        rows[:N * H * W, off:off + Cn] = t.detach().to(torch.float32).permute(0, 2, 3, 1).reshape(N * H * W, Cn)
        return rows

    @staticmethod
    def _nchw(rows, shape, off=0):
        N, Cn, H, W = (int(v) for v in shape)
        return rows[:N * H * W, off:off + Cn].reshape(N, H, W, Cn).permute(0, 3, 1, 2).contiguous()

    def debug_conv_grad(self, dz, x, w, dil=1, pad="graph", max_chunk=0, acc_from=None, no_bias=False, accumulate=False,
                        dx0=None, dw0=None, db0=None, windows=None, fill=0.0):
        """dgrad, wgrad and its reduction of a dense conv alone: ``dz`` (N, cout, H, W), ``x`` (N, cin, H, W), ``w`` (cout, cin, ks,
        ks); ``dx0`` / ``dw0`` / ``db0`` are what dx / dw / db hold before the call (default zeros); ``acc_from`` defaults to cin
        (overwrite); ``windows`` = ((dz_ld, dz_off), (x_ld, x_off), (dx_ld, dx_off)) puts the three tensors in wider rows.
        -> (dx (N, cin, H, W), dw, db, pixel ranges taken, the dx rows whole)."""
        torch = _torch()
        N, cin, H, W = (int(v) for v in x.shape)
        cout, ks = int(w.shape[0]), int(w.shape[2])
        (zl, zo), (xl, xo), (dl, do) = windows if windows is not None else ((cout, 0), (cin, 0), (cin, 0))
        dzr, xr = self._rows(dz, zl, zo, fill), self._rows(x, xl, xo, fill)
        dxr = self._rows(dx0 if dx0 is not None else torch.zeros_like(x), dl, do, fill, self.GUARD_ROWS)
        wc = w.detach().to(torch.float32).contiguous()
        dw = (dw0 if dw0 is not None else torch.zeros_like(wc)).detach().to(torch.float32).clone().contiguous()
        db = (db0 if db0 is not None else torch.zeros(cout, device=x.device)).detach().to(torch.float32).clone().contiguous()
        splits = C.c_int()
        self._order()
        torch.cuda.synchronize()
        self._call("lwp_debug_conv_grad", dzr.data_ptr(), int(zl), int(zo), xr.data_ptr(), int(xl), int(xo), wc.data_ptr(), N, H, W, cout, cin,
                   ks, int(dil), _lib.PAD_MODES[pad], int(max_chunk), cin if acc_from is None else int(acc_from),
                   int(bool(no_bias)), int(bool(accumulate)), dxr.data_ptr(), int(dl), int(do), dw.data_ptr(), db.data_ptr(), C.byref(splits))
        return self._nchw(dxr, x.shape, do), dw, db, splits.value, dxr

    def debug_cpm_dw_grad(self, dz, x, w, beta=False, accumulate=False, max_chunk=0, dx0=None, dw0=None, ld=None, fill=0.0):
        """The cpm's depthwise gradient kernels alone (stride 1, dilation 1): ``dz``, ``x`` (N, C, H, W), ``w`` (C, 1, 3, 3); ``ld``: the
        row stride of all three windows (default C).  -> (dx, dw (C, 1, 3, 3), pixel ranges taken, the dx rows whole)."""
        torch = _torch()
        N, Cn, H, W = (int(v) for v in x.shape)
        ld = Cn if ld is None else int(ld)
        dzr, xr = self._rows(dz, ld, 0, fill), self._rows(x, ld, 0, fill)
        dxr = self._rows(dx0 if dx0 is not None else torch.zeros_like(x), ld, 0, fill, self.GUARD_ROWS)
        wt = w.detach().to(torch.float32).reshape(Cn, 9).t().contiguous()
        dw = (dw0 if dw0 is not None else torch.zeros((Cn, 1, 3, 3), device=x.device)).detach().to(torch.float32).clone().contiguous()
        splits = C.c_int()
        self._order()
        torch.cuda.synchronize()
        self._call("lwp_debug_dw_grad", dzr.data_ptr(), ld, xr.data_ptr(), ld, wt.data_ptr(), N, H, W, Cn, int(bool(beta)),
                   int(bool(accumulate)), int(max_chunk), dxr.data_ptr(), ld, dw.data_ptr(), C.byref(splits))
        return self._nchw(dxr, x.shape), dw, splits.value, dxr

    def debug_loss_grad(self, outs, keypoint_maps, paf_maps, mask, scale, ld=None, off=0, fill=0.0):
        """``loss_grad_kernel`` alone: ``outs`` alternate (N, CH, h, w) and (N, CP, h, w) tensors, ``mask`` (N, h, w), ``scale`` the
        float32 factor loss_scale / batch.  -> ([gradient like outs[s]], [its rows whole])."""
        torch = _torch()
        N, CH, hh, ww = (int(v) for v in keypoint_maps.shape)
        CP = int(paf_maps.shape[1])
        ld = off + max(CH, CP) if ld is None else int(ld)
        S = len(outs)
        src = [self._rows(o, ld, off, fill) for o in outs]
        dst = [self._rows(torch.zeros_like(o), ld, off, fill, self.GUARD_ROWS) for o in outs]
        vp = C.c_void_p
        a = (vp * S)(*[t.data_ptr() + 4 * off for t in src])
        b = (vp * S)(*[t.data_ptr() + 4 * off for t in dst])
        km, pm, mk = (t.detach().to(torch.float32).contiguous() for t in (keypoint_maps, paf_maps, mask))
        self._order()
        torch.cuda.synchronize()
        self._call("lwp_debug_loss_grad", a, b, S, ld, km.data_ptr(), pm.data_ptr(), mk.data_ptr(), N, CH, CP, hh * ww, float(scale))
        return [self._nchw(d, o.shape, off) for d, o in zip(dst, outs)], dst

    def _debug_rows_op(self, name, g, others, ld, fill, *tail):
        """``name(g rows, ld, [other rows, ld]..., pixels, channels, *tail)`` on NHWC rows of width ``ld``; a None among
        ``others`` is passed as a null pointer.  -> (result like g, its rows whole)."""
        torch = _torch()
        N, Cn, H, W = (int(v) for v in g.shape)
        ld = Cn if ld is None else int(ld)
        gr = self._rows(g, ld, 0, fill, self.GUARD_ROWS)
        rs = [self._rows(o, ld, 0, fill) if o is not None else None for o in others]
        self._order()
        torch.cuda.synchronize()
        args = [gr.data_ptr(), ld]
        for r in rs:
            args += [None if r is None else r.data_ptr(), ld]
        self._call(name, *args, N * H * W, Cn, *tail)
        return self._nchw(gr, g.shape), gr

    def debug_relu_mask(self, g, y, res=None, ld=None, fill=0.0):
        """g where y > res (``res`` None: y > 0), else 0; all (N, C, H, W).  -> (result, its rows whole)."""
        return self._debug_rows_op("lwp_debug_relu_mask", g, [y, res], ld, fill)

    def debug_grad_add(self, dst, src, beta, ld=None, fill=0.0):
        """(beta ? dst : 0) + src.  -> (result, its rows whole)."""
        return self._debug_rows_op("lwp_debug_grad_add", dst, [src], ld, fill, int(bool(beta)))

    def debug_elu_grad(self, g, y, ld=None, fill=0.0):
        """g * (y > 0 ? 1 : y + 1), y the ELU's output.  -> (result, its rows whole)."""
        return self._debug_rows_op("lwp_debug_elu_grad", g, [y], ld, fill)

    def debug_pw_fold(self, w, gamma, var):
        """``pw_fold_kernel`` alone: ``w`` (cout, cin), ``gamma`` and ``var`` (cout,) -> the folded (cout, cin) matrix."""
        torch = _torch()
        w, gamma, var = (t.detach().to(torch.float32).contiguous() for t in (w, gamma, var))
        out = torch.empty_like(w)
        self._order()
        torch.cuda.synchronize()
        self._call("lwp_debug_pw_fold", w.data_ptr(), gamma.data_ptr(), var.data_ptr(), out.data_ptr(), int(w.shape[0]), int(w.shape[1]))
        return out

    def debug_bn_chain(self, G, g, W, b, gamma, mean, var, into, accumulate=False):
        """``bn_chain_kernel`` alone: ``G`` and ``W`` (cout, K), the others (cout,); ``into`` = (dW, db or None, dgamma, dbeta), contiguous
        float32 cuda arrays written in place (they may be views into wider arrays)."""
        torch = _torch()
        ins = [t.detach().to(torch.float32).contiguous() for t in (G, g, W, b, gamma, mean, var)]
        for t in into:
            if t is not None and (t.dtype != torch.float32 or not t.is_contiguous() or not t.is_cuda):
                raise ValueError("outputs must be contiguous float32 cuda arrays")
        self._order()
        torch.cuda.synchronize()
        self._call("lwp_debug_bn_chain", *[t.data_ptr() for t in ins], *[None if t is None else t.data_ptr() for t in into],
                   int(ins[0].shape[0]), int(ins[0].shape[1]), int(bool(accumulate)))

    def backward_splits(self, layer_index, depthwise=False):
        """Pixel ranges the last ``stage_backward`` split this layer's weight gradient into (0: none ran); ``depthwise``: those
        of the layer's depthwise weight gradient (a depthwise layer or a fused block of the cpm trunk, train scope "cpm")."""
        n = (lib().lwp_debug_backward_dw_splits if depthwise else lib().lwp_debug_backward_splits)(self.h.ptr, layer_index)
        if n < 0:
            raise ValueError("bad layer index")
        return n

    # ------------------------------------------------------------------ stage fine-tuning step (train.py:41-55, :106; fp32 engines)
    def _flat32(self, flat, what):
        torch = _torch()
        total = self.grad_spec()[1]
        if not getattr(flat, "is_cuda", False) or flat.dtype != torch.float32 or flat.numel() != total or not flat.is_contiguous():
            raise ValueError("%s must be a contiguous float32 cuda array of %d values in the gradient-spec layout" % (what, total))
        return flat

    def adam_groups(self):
        """[(state-dict key, learning-rate multiplier, weight decay on)] per gradient-spec entry (train.py:41-55)."""
        return _lib.train_adam_groups(self.train_scope, self.nref, self.C, self.NH, self.NP)

    def adam_step(self, flat, base_lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=5e-4):
        """One step of the reference's Adam (its parameter groups included) on the stage parameters from the flat gradient array
        ``stage_backward`` filled (``flat_of(grads)``), then the device-side refold and repack of the stage layers: the engine
        is afterwards as if ``load_state_dict`` had been called with the new values, with no host copy and no synchronise.
        The retained ``train_forward`` is invalidated."""
        flat = self._flat32(flat, "flat")
        self._order()
        self._call("lwp_stage_adam_step", flat.data_ptr(), float(base_lr), float(betas[0]), float(betas[1]), float(eps), float(weight_decay))
        self.stage_steps += 1

    def stage_params(self):
        """dict state-dict key -> current raw stage parameter (float32 cuda tensors, views of one flat array in the
        gradient-spec layout: ``flat_of`` gives it)."""
        flat = self._empty(self.grad_spec()[1])
        self._order()
        self._call("lwp_stage_params_get", flat.data_ptr())
        return self.grad_views(flat)

    def trained_params(self):
        """``stage_params`` plus what an earlier, wider train scope trained and the current one no longer covers (the cpm.*
        parameters after "cpm" -> "stages", the model.* ones after "all" -> "cpm"): every parameter whose value on the device may differ from what was loaded."""
        out = dict(self._left_params)
        out.update(self.stage_params())
        return out

    def adam_state(self):
        """dict(step, exp_avg, exp_avg_sq): the step count and the two flat float32 cuda arrays (gradient-spec layout)."""
        m, v = self._empty(self.grad_spec()[1]), self._empty(self.grad_spec()[1])
        step = C.c_int64()
        self._order()
        self._call("lwp_stage_adam_state_get", m.data_ptr(), v.data_ptr(), C.byref(step))
        return dict(step=int(step.value), exp_avg=m, exp_avg_sq=v)

    def load_adam_state(self, state):
        """Restores what ``adam_state`` returned (arrays on the host or the device); ``None`` discards the state."""
        if state is None:
            self._call("lwp_stage_adam_reset")
            return
        torch = _torch()
        m = self._flat32(torch.as_tensor(state["exp_avg"]).to(self._gpu, torch.float32).contiguous(), "exp_avg")
        v = self._flat32(torch.as_tensor(state["exp_avg_sq"]).to(self._gpu, torch.float32).contiguous(), "exp_avg_sq")
        self._order()
        self._call("lwp_stage_adam_state_set", m.data_ptr(), v.data_ptr(), int(state["step"]))

    def time_adam_step(self, flat, base_lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=5e-4, iters=20):
        """(ms of ``iters`` Adam-kernel launches, ms of ``iters`` repack launches) on scratch copies (HIP events)."""
        flat = self._flat32(flat, "flat")
        ms = (C.c_float * 2)()
        self._order()
        self._call("lwp_time_stage_adam_step", flat.data_ptr(), float(base_lr), float(betas[0]), float(betas[1]), float(eps),
                   float(weight_decay), int(iters), ms)
        return float(ms[0]), float(ms[1])

    # ------------------------------------------------------------------ measurement
    def time_pipeline(self, x_cuda, iters, what=1, upsample_ratio=4, demo=True):
        """milliseconds for ``iters`` back-to-back passes (HIP events on the engine's stream)."""
        x_cuda = self._as_device_input(x_cuda)
        N, _, H, W = x_cuda.shape
        ms = C.c_float()
        self._call("lwp_time_pipeline", x_cuda.data_ptr(), N, H, W, upsample_ratio, 1 if demo else 0, what, iters, C.byref(ms))
        self._last_N = N
        return ms.value

    def time_layer(self, layer_index, N, H, W, iters=50):
        ms = C.c_float()
        self._call("lwp_debug_time_layer", layer_index, N, H, W, iters, C.byref(ms))
        return ms.value

    def profile_launches(self, x_cuda, reps=5, upsample_ratio=4, demo=True):
        """[(name, class, ms)] per launch in issue order (HIP events around every launch)."""
        x_cuda = self._as_device_input(x_cuda)
        N, _, H, W = x_cuda.shape
        cap = 256
        ms = (C.c_float * cap)()
        kc = (C.c_int * cap)()
        n = C.c_int()
        self._call("lwp_profile_launches", x_cuda.data_ptr(), N, H, W, upsample_ratio, 1 if demo else 0, reps, ms, kc, cap, C.byref(n))
        layers = self.layers()
        post = ["find_peaks", "nms", "score_pairs", "match", "assemble", "tail_rows", "tail_track"]
        out, npost = [], 0
        for i in range(n.value):
            li = (kc[i] >> 8) - 1                      # first layer the launch covers (a fused head pair is one launch), -1: post kernel
            if li >= 0:
                name = layers[li]["name"]
            else:
                name = post[npost] if npost < len(post) else "launch%d" % i
                npost += 1
            out.append((name, kc[i] & 0xff, ms[i]))
        return out

    def profile_classes(self, x_cuda, reps=5, upsample_ratio=4, demo=True):
        x_cuda = self._as_device_input(x_cuda)
        N, _, H, W = x_cuda.shape
        ms = (C.c_float * 6)()
        ln = (C.c_int * 6)()
        self._call("lwp_profile_classes", x_cuda.data_ptr(), N, H, W, upsample_ratio, 1 if demo else 0, reps, ms, ln)
        names = ["stem", "depthwise", "pointwise_1x1", "dense_3x3", "post", "other"]
        return {n: {"ms": ms[i], "launches": ln[i]} for i, n in enumerate(names)}


    # ------------------------------------------------------------------ COCO key-point evaluation (val.py:17-27)
    @staticmethod
    def _coco_args(packed):
        """n_images, the detection pointers and the ground-truth pointers of ``coco_pack``'s arrays, which ``packed`` keeps alive:
        what lwp_coco_eval takes.  An empty array is passed as a null pointer."""
        gt = Engine._coco_gt_args(packed)
        return gt[:1] + (packed["dt_off"].ctypes.data, _data_or_null(packed["dt_kp"]), _data_or_null(packed["dt_score"])) + gt[1:]

    @staticmethod
    def _coco_gt_args(packed):
        """n_images and the ground-truth pointers of ``_coco_args``: what lwp_coco_open takes."""
        return (int(packed["n_images"]), packed["gt_off"].ctypes.data) + tuple(
            _data_or_null(packed[k]) for k in ("gt_kp", "gt_area", "gt_bbox", "gt_iscrowd", "gt_ignore"))

    def coco_eval(self, gt, detections=None):
        """COCOeval(gt, loadRes(detections), 'keypoints') evaluate() + accumulate() on the GPU with COCOeval's default
        parameters.  ``gt``: a COCO ground-truth dict ('images', 'annotations', 'categories') with ``detections`` the list of
        result dicts (``val.coco_detections``), or the arrays ``coco_pack`` made of the two.  Returns a dict: ``precision``
        (10, 101, 3) and ``scores`` (10, 101, 3) indexed [IoU threshold, recall threshold, area range], ``recall`` (10, 3),
        ``npig`` (3,) and ``stats``, the ten numbers of summarize().  Two calls on the same input return the same bits."""
        packed = gt if detections is None and "dt_off" in gt else coco_pack(gt, detections)
        return self._coco_result("lwp_coco_eval", *self._coco_args(packed))

    def _coco_result(self, name, *args):
        """``name(*args, precision, recall, scores, npig)`` and the dict ``coco_eval`` returns of the four arrays it filled."""
        precision = np.empty((10, 101, 3), dtype=np.float64)
        scores = np.empty((10, 101, 3), dtype=np.float64)
        recall = np.empty((10, 3), dtype=np.float64)
        npig = np.zeros(3, dtype=np.int64)
        self._call(name, *args, precision.ctypes.data, recall.ctypes.data, scores.ctypes.data, npig.ctypes.data)
        return {"precision": precision, "recall": recall, "scores": scores, "npig": npig, "stats": coco_stats(precision, recall)}

    def debug_coco_oks(self, gt, detections=None, image=0):
        """The per-image half of ``coco_eval`` for image number ``image`` (position in ascending image-id order): ``order``, the
        indices within the image of its up to 20 selected detections by rank; ``oks`` (len(order), G), columns in the ground
        truths' input order; ``matched`` / ``ignored`` (3, 10, 20) bool by [area range, IoU threshold, rank]; ``npig`` (3,)."""
        packed = gt if detections is None and "dt_off" in gt else coco_pack(gt, detections)
        image = int(image)
        if not 0 <= image < int(packed["n_images"]):
            raise ValueError("image %d out of range" % image)
        G = int(packed["gt_off"][image + 1] - packed["gt_off"][image])
        n_sel, order, npig = C.c_int(), (C.c_int * 20)(), (C.c_int * 3)()
        oks = np.zeros((20, max(G, 1)), dtype=np.float64)
        matched, ignored = np.zeros((30, 20), dtype=np.uint8), np.zeros((30, 20), dtype=np.uint8)
        self._call("lwp_debug_coco_oks", *self._coco_args(packed), image, C.byref(n_sel), order, oks.ctypes.data, oks.size,
                   matched.ctypes.data, ignored.ctypes.data, npig)
        n = n_sel.value
        return {"order": [order[r] for r in range(n)], "oks": oks.reshape(-1)[:n * G].reshape(n, G).copy(),
                "matched": matched.reshape(3, 10, 20).astype(bool), "ignored": ignored.reshape(3, 10, 20).astype(bool),
                "npig": np.array([npig[a] for a in range(3)], dtype=np.int64)}

    # ------------------------------------------------------------------ device-resident validation (val.py:113-160)
    def coco_open(self, gt_or_packed, row_cap=None):
        """Upload a data set's ground truth once and open a detection store of ``row_cap`` rows on the device (default: 32 an
        image).  ``gt_or_packed``: a COCO ground-truth dict, or what ``coco_pack_gt`` / ``coco_pack`` made of one.  A second
        call replaces the store.  Returns the packed ground truth (``image_ids`` gives an image's index)."""
        g = gt_or_packed if "gt_off" in gt_or_packed else coco_pack_gt(gt_or_packed)
        n = int(g["n_images"])
        row_cap = 32 * n if row_cap is None else int(row_cap)
        self._call("lwp_coco_open", *self._coco_gt_args(g), row_cap)
        self._coco_n = n
        self._val_store = None                # (val.evaluate(store=True) notes here which labels the store belongs to)
        return g

    def coco_release(self):
        self._val_store = None
        self._call("lwp_coco_release")

    def coco_reset(self):
        """Forget the detections and the status, keep the ground truth: the next validation of the same data set."""
        self._call("lwp_coco_reset")

    def coco_add_maps(self, heat, paf, image_index, upsample_ratio=4, demo=False, layout="NCHW"):
        """``poses_from_maps`` for cuda tensors whose poses go into the detection store instead of to the host: grouping and the
        append kernel are enqueued and the call returns; nothing is synchronised or fetched.  ``image_index``: per frame its
        image's position in the ground truth's ascending id order."""
        if not getattr(heat, "is_cuda", False) or not getattr(paf, "is_cuda", False):
            raise TypeError("coco_add_maps takes cuda tensors (the maps stay on the device)")
        hp, pp, _, lay, N, hs, ws, _ = self._maps(heat, paf, layout)
        idx = np.ascontiguousarray(np.atleast_1d(image_index), dtype=np.int32)
        if idx.shape != (N,):
            raise ValueError("image_index must hold one index per frame (%d), got %s" % (N, idx.shape))
        self._call("lwp_coco_add_maps", hp, pp, lay, N, hs, ws, upsample_ratio, 1 if demo else 0, idx.ctypes.data)

    def coco_add_rows(self, image_index, keypoints, scores):
        """Append ready-made detections of one image: ``keypoints`` (n, 17, 3) or (n, 51), ``scores`` (n,); enqueue only."""
        kp = np.ascontiguousarray(keypoints, dtype=np.float64).reshape(-1, 17, 3)
        sc = np.ascontiguousarray(scores, dtype=np.float64).reshape(-1)
        if len(kp) != len(sc):
            raise ValueError("%d key-point rows but %d scores" % (len(kp), len(sc)))
        self._call("lwp_coco_add_rows", int(image_index), len(sc), _data_or_null(kp), _data_or_null(sc))

    def coco_counts(self):
        """(rows in the store, rows per image (n_images,) int32) after everything queued so far; raises the store's status."""
        total = C.c_int64()
        per = np.zeros(self._coco_n, dtype=np.int32)
        self._call("lwp_coco_counts", C.byref(total), per.ctypes.data)
        return int(total.value), per

    def coco_rows(self):
        """The store's rows in the evaluation's order (images ascending, within an image as added): ``image`` (n,) int32,
        ``keypoints`` (n, 17, 3) and ``score`` (n,) float64.  Two library calls, one synchronise each: ``coco_counts`` sizes
        the arrays (sizing them by the store's capacity instead would copy every unused row back), lwp_coco_rows fills them."""
        n, _ = self.coco_counts()
        img = np.zeros(n, dtype=np.int32)
        kp = np.zeros((n, 17, 3), dtype=np.float64)
        sc = np.zeros(n, dtype=np.float64)
        self._call("lwp_coco_rows", img.ctypes.data, kp.ctypes.data, sc.ctypes.data, n)
        return {"image": img, "keypoints": kp, "score": sc}

    def coco_finish(self):
        """``coco_eval`` on the store's rows against the resident ground truth: the same dict, bit for bit what ``coco_eval``
        returns for the same rows.  The store stays as it is."""
        return self._coco_result("lwp_coco_finish")

    def debug_coco_rows(self, frames, image_index):
        """The append kernel alone: ``frames`` is a list of (pose_entries (P, 20), all_keypoints (n, 4)) as ``poses_from_maps``
        returns them, loaded into the serial result block and appended as images ``image_index``."""
        N = len(frames)
        ne = np.array([len(f[0]) for f in frames], dtype=np.int32)
        nk = np.array([len(f[1]) for f in frames], dtype=np.int32)
        ent = np.ascontiguousarray(np.concatenate([np.asarray(f[0], dtype=np.float64).reshape(-1, 20) for f in frames]))
        kpt = np.ascontiguousarray(np.concatenate([np.asarray(f[1], dtype=np.float64).reshape(-1, 4) for f in frames]))
        idx = np.ascontiguousarray(image_index, dtype=np.int32)
        self._call("lwp_debug_coco_rows", N, _data_or_null(ent), ne.ctypes.data, _data_or_null(kpt), nk.ctypes.data, idx.ctypes.data)


def coco_pack(gt, detections):
    """The arrays ``lwp_coco_eval`` takes, from a COCO ground-truth dict and a list of result dicts, as COCO() / loadRes() /
    COCOeval._prepare() arrange them: the images of ``gt`` in ascending id order, each with its annotations and detections in
    input order; ``gt_ignore`` = iscrowd or num_keypoints == 0.  ValueError: a detection whose image_id is not in ``gt``
    (loadRes asserts this), a non-positive annotation id (COCOeval reads a match to id 0 as no match), more than one category."""
    g, index, cat = _coco_gt(gt)
    n = g["n_images"]
    per_dt = [[] for _ in range(n)]
    for d in detections:
        if int(d["image_id"]) not in index:
            raise ValueError("detection for image %r, which the ground truth does not list" % (d["image_id"],))
        if cat is not None and int(d.get("category_id", cat)) != cat:
            continue
        per_dt[index[int(d["image_id"])]].append(d)
    dts = [d for lst in per_dt for d in lst]
    return {"n_images": n, "image_ids": g["image_ids"],
            "dt_off": np.cumsum([0] + [len(v) for v in per_dt], dtype=np.int64), "dt_kp": _coco_kp(dts),
            "dt_score": np.array([d["score"] for d in dts], dtype=np.float64),
            "gt_off": g["gt_off"], "gt_kp": g["gt_kp"], "gt_area": g["gt_area"], "gt_bbox": g["gt_bbox"],
            "gt_iscrowd": g["gt_iscrowd"], "gt_ignore": g["gt_ignore"]}


def _coco_kp(rows):
    a = np.array([r["keypoints"] for r in rows], dtype=np.float64).reshape(-1, 17, 3) if rows else np.zeros((0, 17, 3))
    return np.ascontiguousarray(a)


def _coco_gt(gt):
    """(the ground-truth arrays, image id -> position, the one category id or None): the half of ``coco_pack`` that does not
    change while a data set is validated again and again."""
    cats = sorted({int(c["id"]) for c in gt["categories"]}) if gt.get("categories") else \
        sorted({int(a["category_id"]) for a in gt.get("annotations", []) if "category_id" in a})
    if len(cats) > 1:
        raise ValueError("COCO evaluation supports one category, the ground truth has %d" % len(cats))
    cat = cats[0] if cats else None
    img_ids = sorted({int(im["id"]) for im in gt["images"]})
    index = {v: i for i, v in enumerate(img_ids)}
    n = len(img_ids)
    if n < 1:
        raise ValueError("the ground truth lists no image")
    per_gt = [[] for _ in range(n)]
    for a in gt.get("annotations", []):
        if int(a["id"]) <= 0:
            raise ValueError("annotation id %r is not positive" % (a["id"],))
        if cat is not None and int(a.get("category_id", cat)) != cat:
            continue
        if int(a["image_id"]) in index:
            per_gt[index[int(a["image_id"])]].append(a)
    gts = [a for lst in per_gt for a in lst]
    crowd = np.array([1 if a.get("iscrowd", 0) else 0 for a in gts], dtype=np.int32)
    nokp = np.array([1 if a["num_keypoints"] == 0 else 0 for a in gts], dtype=np.int32)
    return ({"n_images": n, "image_ids": img_ids,
             "gt_off": np.cumsum([0] + [len(v) for v in per_gt], dtype=np.int64), "gt_kp": _coco_kp(gts),
             "gt_area": np.array([a["area"] for a in gts], dtype=np.float64),
             "gt_bbox": np.ascontiguousarray(np.array([a["bbox"] for a in gts], dtype=np.float64).reshape(-1, 4)),
             "gt_iscrowd": crowd, "gt_ignore": (crowd | nokp).astype(np.int32)}, index, cat)


def coco_pack_gt(gt):
    """The ground-truth half of ``coco_pack``: ``n_images``, ``image_ids`` (ascending) and the ``gt_*`` arrays, the same
    values under the same keys.  This is what ``Engine.coco_open`` uploads once per data set."""
    return _coco_gt(gt)[0]


def coco_stats(precision, recall):
    """COCOeval._summarizeKps on accumulate()'s arrays (precision (10, 101, 3), recall (10, 3); ranges all, medium, large): AP,
    AP50, AP75, AP medium, AP large, then the same five of AR.  Each is the mean over the entries > -1, or -1 without any."""
    def mean(s):
        s = s[s > -1]
        return -1.0 if s.size == 0 else float(np.mean(s))
    out = []
    for s in (precision, recall):
        out += [mean(s[..., 0]), mean(s[0, ..., 0]), mean(s[5, ..., 0]), mean(s[..., 1]), mean(s[..., 2])]
    return np.array(out, dtype=np.float64)


_default = {}


def default_engine(device_id=None):
    """Shared engine for the free functions (extract_keypoints / group_keypoints / up-sampling)."""
    if device_id is None:
        device_id = 0
    if device_id not in _default:
        _default[device_id] = Engine(device_id)
    return _default[device_id]
