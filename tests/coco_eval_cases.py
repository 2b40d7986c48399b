"""COCO key-point evaluation: the oracle and the cases of test_coco_eval_host.py / test_gpu_coco_eval.py.

``CocoEvalRef`` is a plain NumPy restatement of pycocotools' cocoeval.py for iouType 'keypoints' (computeOks, evaluateImg,
accumulate, summarize, and loadRes's detection area), with the original's loop structure.  pycocotools itself is not
available where this project is built, so the restatement is UNPINNED against it; test_coco_eval_host.py pins it to
closed-form cases instead.

The case builders assert, on the CPU, the conditions under which the discrete results (selected order, matches, ignore
flags, counts, hence precision / recall / scores) cannot depend on the last bits of exp():
  * every OKS entry lies at least 1e-9 from each of the ten IoU thresholds;
  * within a detection's row, two entries >= 0.5 differ by more than 1e-9 or come from duplicated ground-truth rows;
  * the data set's ten stats are not all in {-1, 0, 1}.
"""
import copy
from collections import defaultdict

import numpy as np

SCAN_CHUNK = 256      # kEvalScanChunk of csrc/lwp_internal.h: detections one step of the accumulate kernel's scans covers


# ------------------------------------------------------------------------------------------------ the restatement
class Params(object):
    def __init__(self):
        self.iouThrs = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)
        self.recThrs = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)
        self.maxDets = [20]
        self.areaRng = [[0 ** 2, 1e5 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]]
        self.areaRngLbl = ['all', 'medium', 'large']
        self.kpt_oks_sigmas = np.array([.26, .25, .25, .35, .35, .79, .79, .72, .72, .62, .62, 1.07, 1.07, .87, .87, .89, .89]) / 10.0


class CocoEvalRef(object):
    """COCOeval(COCO(gt), COCO(gt).loadRes(results), 'keypoints') for dicts already in memory."""

    def __init__(self, gt, results):
        self.params = p = Params()
        p.imgIds = sorted({im['id'] for im in gt['images']})
        p.catIds = sorted({c['id'] for c in gt['categories']})
        assert set(d['image_id'] for d in results) <= set(p.imgIds), 'Results do not correspond to current coco set'
        gts = copy.deepcopy(gt['annotations'])
        dts = copy.deepcopy(results)
        for id, ann in enumerate(dts):                 # loadRes, the 'keypoints' branch
            s = ann['keypoints']
            x = s[0::3]
            y = s[1::3]
            x0, x1, y0, y1 = np.min(x), np.max(x), np.min(y), np.max(y)
            ann['area'] = (x1 - x0) * (y1 - y0)
            ann['id'] = id + 1
            ann['bbox'] = [x0, y0, x1 - x0, y1 - y0]
        for g in gts:                                  # _prepare
            g['ignore'] = g['ignore'] if 'ignore' in g else 0
            g['ignore'] = 'iscrowd' in g and g['iscrowd']
            g['ignore'] = (g['num_keypoints'] == 0) or g['ignore']
        self._gts = defaultdict(list)
        self._dts = defaultdict(list)
        for g in gts:
            if g['category_id'] in p.catIds and g['image_id'] in p.imgIds:
                self._gts[g['image_id'], g['category_id']].append(g)
        for d in dts:
            if d['category_id'] in p.catIds:
                self._dts[d['image_id'], d['category_id']].append(d)

    def evaluate(self):
        p = self.params
        self.ious = {(imgId, catId): self.computeOks(imgId, catId) for imgId in p.imgIds for catId in p.catIds}
        maxDet = p.maxDets[-1]
        self.evalImgs = [self.evaluateImg(imgId, catId, areaRng, maxDet)
                         for catId in p.catIds for areaRng in p.areaRng for imgId in p.imgIds]

    def computeOks(self, imgId, catId):
        p = self.params
        gts = self._gts[imgId, catId]
        dts = self._dts[imgId, catId]
        inds = np.argsort([-d['score'] for d in dts], kind='mergesort')
        dts = [dts[i] for i in inds]
        if len(dts) > p.maxDets[-1]:
            dts = dts[0:p.maxDets[-1]]
        if len(gts) == 0 or len(dts) == 0:
            return []
        ious = np.zeros((len(dts), len(gts)))
        sigmas = p.kpt_oks_sigmas
        vars = (sigmas * 2) ** 2
        k = len(sigmas)
        for j, gt in enumerate(gts):
            g = np.array(gt['keypoints'])
            xg = g[0::3]; yg = g[1::3]; vg = g[2::3]
            k1 = np.count_nonzero(vg > 0)
            bb = gt['bbox']
            x0 = bb[0] - bb[2]; x1 = bb[0] + bb[2] * 2
            y0 = bb[1] - bb[3]; y1 = bb[1] + bb[3] * 2
            for i, dt in enumerate(dts):
                d = np.array(dt['keypoints'])
                xd = d[0::3]; yd = d[1::3]
                if k1 > 0:
                    dx = xd - xg
                    dy = yd - yg
                else:
                    z = np.zeros((k))
                    dx = np.max((z, x0 - xd), axis=0) + np.max((z, xd - x1), axis=0)
                    dy = np.max((z, y0 - yd), axis=0) + np.max((z, yd - y1), axis=0)
                e = (dx ** 2 + dy ** 2) / vars / (gt['area'] + np.spacing(1)) / 2
                if k1 > 0:
                    e = e[vg > 0]
                ious[i, j] = np.sum(np.exp(-e)) / e.shape[0]
        return ious

    def evaluateImg(self, imgId, catId, aRng, maxDet):
        p = self.params
        gt = self._gts[imgId, catId]
        dt = self._dts[imgId, catId]
        if len(gt) == 0 and len(dt) == 0:
            return None
        for g in gt:
            if g['ignore'] or (g['area'] < aRng[0] or g['area'] > aRng[1]):
                g['_ignore'] = 1
            else:
                g['_ignore'] = 0
        gtind = np.argsort([g['_ignore'] for g in gt], kind='mergesort')
        gt = [gt[i] for i in gtind]
        dtind = np.argsort([-d['score'] for d in dt], kind='mergesort')
        dt = [dt[i] for i in dtind[0:maxDet]]
        iscrowd = [int(o['iscrowd']) for o in gt]
        ious = self.ious[imgId, catId][:, gtind] if len(self.ious[imgId, catId]) > 0 else self.ious[imgId, catId]
        T = len(p.iouThrs)
        G = len(gt)
        D = len(dt)
        gtm = np.zeros((T, G))
        dtm = np.zeros((T, D))
        gtIg = np.array([g['_ignore'] for g in gt])
        dtIg = np.zeros((T, D))
        if not len(ious) == 0:
            for tind, t in enumerate(p.iouThrs):
                for dind, d in enumerate(dt):
                    iou = min([t, 1 - 1e-10])
                    m = -1
                    for gind, g in enumerate(gt):
                        if gtm[tind, gind] > 0 and not iscrowd[gind]:
                            continue
                        if m > -1 and gtIg[m] == 0 and gtIg[gind] == 1:
                            break
                        if ious[dind, gind] < iou:
                            continue
                        iou = ious[dind, gind]
                        m = gind
                    if m == -1:
                        continue
                    dtIg[tind, dind] = gtIg[m]
                    dtm[tind, dind] = gt[m]['id']
                    gtm[tind, m] = d['id']
        a = np.array([d['area'] < aRng[0] or d['area'] > aRng[1] for d in dt]).reshape((1, len(dt)))
        dtIg = np.logical_or(dtIg, np.logical_and(dtm == 0, np.repeat(a, T, 0)))
        return {'image_id': imgId, 'aRng': aRng, 'dtIds': [d['id'] for d in dt], 'dtMatches': dtm,
                'dtScores': [d['score'] for d in dt], 'gtIgnore': gtIg, 'dtIgnore': dtIg}

    def accumulate(self):
        p = self.params
        T = len(p.iouThrs); R = len(p.recThrs); K = len(p.catIds); A = len(p.areaRng); M = len(p.maxDets)
        precision = -np.ones((T, R, K, A, M))
        recall = -np.ones((T, K, A, M))
        scores = -np.ones((T, R, K, A, M))
        I0 = len(p.imgIds)
        A0 = len(p.areaRng)
        self.npig = np.zeros(A, dtype=np.int64)
        for k in range(K):
            Nk = k * A0 * I0
            for a in range(A):
                Na = a * I0
                for m, maxDet in enumerate(p.maxDets):
                    E = [self.evalImgs[Nk + Na + i] for i in range(I0)]
                    E = [e for e in E if e is not None]
                    if len(E) == 0:
                        continue
                    dtScores = np.concatenate([e['dtScores'][0:maxDet] for e in E])
                    inds = np.argsort(-dtScores, kind='mergesort')
                    dtScoresSorted = dtScores[inds]
                    dtm = np.concatenate([e['dtMatches'][:, 0:maxDet] for e in E], axis=1)[:, inds]
                    dtIg = np.concatenate([e['dtIgnore'][:, 0:maxDet] for e in E], axis=1)[:, inds]
                    gtIg = np.concatenate([e['gtIgnore'] for e in E])
                    npig = np.count_nonzero(gtIg == 0)
                    self.npig[a] = npig
                    if npig == 0:
                        continue
                    tps = np.logical_and(dtm, np.logical_not(dtIg))
                    fps = np.logical_and(np.logical_not(dtm), np.logical_not(dtIg))
                    tp_sum = np.cumsum(tps, axis=1).astype(dtype=float)
                    fp_sum = np.cumsum(fps, axis=1).astype(dtype=float)
                    for t, (tp, fp) in enumerate(zip(tp_sum, fp_sum)):
                        tp = np.array(tp)
                        fp = np.array(fp)
                        nd = len(tp)
                        rc = tp / npig
                        pr = tp / (fp + tp + np.spacing(1))
                        q = np.zeros((R,))
                        ss = np.zeros((R,))
                        if nd:
                            recall[t, k, a, m] = rc[-1]
                        else:
                            recall[t, k, a, m] = 0
                        pr = pr.tolist(); q = q.tolist()
                        for i in range(nd - 1, 0, -1):
                            if pr[i] > pr[i - 1]:
                                pr[i - 1] = pr[i]
                        inds = np.searchsorted(rc, p.recThrs, side='left')
                        try:
                            for ri, pi in enumerate(inds):
                                q[ri] = pr[pi]
                                ss[ri] = dtScoresSorted[pi]
                        except IndexError:
                            pass
                        precision[t, :, k, a, m] = np.array(q)
                        scores[t, :, k, a, m] = np.array(ss)
        self.eval = {'precision': precision, 'recall': recall, 'scores': scores}

    def summarize(self):
        lines = []

        def _summarize(ap=1, iouThr=None, areaRng='all', maxDets=100):
            p = self.params
            iStr = ' {:<18} {} @[ IoU={:<9} | area={:>6s} | maxDets={:>3d} ] = {:0.3f}'
            titleStr = 'Average Precision' if ap == 1 else 'Average Recall'
            typeStr = '(AP)' if ap == 1 else '(AR)'
            iouStr = '{:0.2f}:{:0.2f}'.format(p.iouThrs[0], p.iouThrs[-1]) if iouThr is None else '{:0.2f}'.format(iouThr)
            aind = [i for i, aRng in enumerate(p.areaRngLbl) if aRng == areaRng]
            mind = [i for i, mDet in enumerate(p.maxDets) if mDet == maxDets]
            if ap == 1:
                s = self.eval['precision']
                if iouThr is not None:
                    t = np.where(iouThr == p.iouThrs)[0]
                    s = s[t]
                s = s[:, :, :, aind, mind]
            else:
                s = self.eval['recall']
                if iouThr is not None:
                    t = np.where(iouThr == p.iouThrs)[0]
                    s = s[t]
                s = s[:, :, aind, mind]
            if len(s[s > -1]) == 0:
                mean_s = -1
            else:
                mean_s = np.mean(s[s > -1])
            lines.append(iStr.format(titleStr, typeStr, iouStr, areaRng, maxDets, mean_s))
            return mean_s
        stats = np.zeros((10,))
        stats[0] = _summarize(1, maxDets=20)
        stats[1] = _summarize(1, maxDets=20, iouThr=.5)
        stats[2] = _summarize(1, maxDets=20, iouThr=.75)
        stats[3] = _summarize(1, maxDets=20, areaRng='medium')
        stats[4] = _summarize(1, maxDets=20, areaRng='large')
        stats[5] = _summarize(0, maxDets=20)
        stats[6] = _summarize(0, maxDets=20, iouThr=.5)
        stats[7] = _summarize(0, maxDets=20, iouThr=.75)
        stats[8] = _summarize(0, maxDets=20, areaRng='medium')
        stats[9] = _summarize(0, maxDets=20, areaRng='large')
        self.stats = stats
        self.lines = lines


def reference(gt, results):
    """The evaluated, accumulated and summarised restatement of one data set."""
    ref = CocoEvalRef(gt, results)
    ref.evaluate()
    ref.accumulate()
    ref.summarize()
    return ref


def image_reference(ref, index):
    """What Engine.debug_coco_oks returns for image number ``index`` (ascending id), read off the restatement."""
    p = ref.params
    img, cat = p.imgIds[index], p.catIds[0]
    dts = ref._dts[img, cat]
    order = [int(i) for i in np.argsort([-d['score'] for d in dts], kind='mergesort')[:20]]
    G = len(ref._gts[img, cat])
    ious = ref.ious[img, cat]
    oks = np.asarray(ious, dtype=np.float64).reshape(len(order), G) if len(ious) else np.zeros((len(order), G))
    matched, ignored = np.zeros((3, 10, 20), dtype=bool), np.zeros((3, 10, 20), dtype=bool)
    npig = np.zeros(3, dtype=np.int64)
    for a in range(3):
        e = ref.evalImgs[a * len(p.imgIds) + index]
        if e is None:
            continue
        matched[a, :, :len(order)] = e['dtMatches'] != 0
        ignored[a, :, :len(order)] = e['dtIgnore']
        npig[a] = np.count_nonzero(e['gtIgnore'] == 0)
    return {"order": order, "oks": oks, "matched": matched, "ignored": ignored, "npig": npig}


# ------------------------------------------------------------------------------------------------ data sets
_TEMPLATE = np.random.RandomState(17).uniform(0.0, 1.0, size=(17, 2))      # a fixed "pose" in the unit square


def pose(cx, cy, size):
    """17 (x, y) around a centre."""
    return np.array([cx, cy]) + (_TEMPLATE - 0.5) * size


def far_pose():
    return pose(900.0, 700.0, 60.0)


def gt_ann(ann_id, image_id, xy, area, visible=None, iscrowd=0, bbox=None):
    """A person annotation: ``visible`` is the list of visible key-point indices (default all); hidden ones are (0, 0, 0)."""
    vis = np.zeros(17, dtype=bool)
    vis[list(range(17)) if visible is None else list(visible)] = True
    kp = []
    for k in range(17):
        kp += [float(xy[k][0]), float(xy[k][1]), 2] if vis[k] else [0, 0, 0]
    if bbox is None:
        x0, y0 = np.min(xy, axis=0)
        x1, y1 = np.max(xy, axis=0)
        bbox = [float(x0), float(y0), float(x1 - x0), float(y1 - y0)]
    return {"id": ann_id, "image_id": image_id, "category_id": 1, "keypoints": kp, "num_keypoints": int(vis.sum()),
            "area": float(area), "bbox": bbox, "iscrowd": iscrowd}


def det(image_id, xy, score, missing=()):
    kp = []
    for k in range(17):
        kp += [0.0, 0.0, 0.0] if k in missing else [float(xy[k][0]), float(xy[k][1]), 1.0]
    return {"image_id": image_id, "category_id": 1, "keypoints": kp, "score": float(score)}


def dataset(image_ids, anns):
    return {"images": [{"id": i} for i in image_ids], "annotations": anns, "categories": [{"id": 1, "name": "person"}]}


class Builder(object):
    """Seeded images of jittered people.  Scores have two decimals, so ties abound, within and across images."""

    def __init__(self, seed):
        self.rng = np.random.RandomState(seed)
        self.anns, self.dets, self.image_ids = [], [], []
        self.next_ann = 1

    def person(self, image_id, area=None, **kw):
        r = self.rng
        size = r.uniform(30.0, 160.0)
        xy = pose(r.uniform(80, 560), r.uniform(80, 400), size)
        a = gt_ann(self.next_ann, image_id, xy, 0.55 * size * size if area is None else area, **kw)
        self.next_ann += 1
        self.anns.append(a)
        return xy, a["area"]

    def jittered(self, image_id, xy, area, score=None, missing=()):
        r = self.rng
        noise = r.normal(size=(17, 2)) * r.uniform(0.0, 0.12) * np.sqrt(area)
        self.dets.append(det(image_id, xy + noise, round(r.uniform(0.05, 0.95), 2) if score is None else score, missing))

    def clutter(self, image_id):
        r = self.rng
        self.dets.append(det(image_id, pose(r.uniform(0, 640), r.uniform(0, 480), r.uniform(20, 200)), round(r.uniform(0.05, 0.6), 2)))

    def image(self, image_id, n_gt, n_det, crowd=(), no_kp=(), partly=(), areas=None, duplicate_last=False):
        """One image: n_gt people (indices in ``crowd`` are crowds, in ``no_kp`` without a visible key-point, in ``partly``
        with six hidden ones), n_det detections: jittered copies of the people in turn, every fourth one clutter."""
        self.image_ids.append(image_id)
        people = []
        for g in range(n_gt):
            kw = {}
            if g in crowd:
                kw["iscrowd"] = 1
            if g in no_kp:
                kw["visible"] = []
            elif g in partly:
                kw["visible"] = [0, 1, 2, 5, 6, 7, 8, 11, 12, 13, 16]
            people.append(self.person(image_id, None if areas is None else areas[g % len(areas)], **kw))
        if duplicate_last and people:
            dup = copy.deepcopy(self.anns[-1])
            dup["id"] = self.next_ann
            self.next_ann += 1
            self.anns.append(dup)
        for d in range(n_det):
            if not people or d % 4 == 3:
                self.clutter(image_id)
            else:
                xy, area = people[d % len(people)]
                self.jittered(image_id, xy, area, missing=(3, 9) if d % 5 == 2 else ())

    def done(self):
        # the files list images, annotations and detections in no particular order: the evaluation sorts the images by id
        order = list(reversed(self.image_ids))
        return dataset(order, list(self.anns)), list(self.dets)


def case_mixed():
    """Every per-image shape of the issue's table in one data set."""
    b = Builder(101)
    b.image(50, 1, 0)                                  # GT but no detection
    b.image(7, 0, 3)                                   # detections but no GT
    b.image(21, 0, 0)                                  # neither: does not count
    b.image(3, 1, 1)                                   # D = 1, G = 1 ...
    # ... replaced by an identical detection: OKS exactly 1
    b.dets[-1] = det(3, np.array(b.anns[-1]["keypoints"]).reshape(17, 3)[:, :2], 0.9)
    b.image(12, 33, 20, crowd=(4,), partly=(1, 7, 20))
    b.image(13, 65, 21, crowd=(0, 30), no_kp=(5, 6), partly=(2,))
    b.image(99, 129, 45, crowd=(3, 77), no_kp=(10,), partly=(11, 12), duplicate_last=True)      # G = 130 with the duplicate
    b.image(40, 4, 6, areas=[1024.0, 9216.0])          # areas on the edges of the ranges count on both sides
    b.image(41, 3, 5, partly=(0, 1, 2))
    return b.done()


def case_total(seed, total, small=False):
    """A data set of exactly ``total`` detections, at most 20 an image (so all are selected); ``small``: every person below
    32^2, so medium and large hold no counted ground truth and stay at -1."""
    b = Builder(seed)
    image_id = 1000
    left = total
    while left > 0:
        n = int(min(left, b.rng.randint(1, 9)))
        b.image(image_id, int(b.rng.randint(1, 5)), n, areas=[500.0, 800.0] if small else None)
        image_id -= 7                                  # descending: the file order is not the id order
        left -= n
    return b.done()


def case_nd1():
    """One selected detection in the data set; two small people, so AP is a fraction and medium / large stay at -1."""
    b = Builder(5)
    b.image(8, 2, 1, areas=[500.0])
    return b.done()


# name -> builder; SCAN_CHUNK is the accumulate kernel's scan step (one detection per thread, then a carry)
CASES = {
    "mixed": case_mixed,
    "nd1": case_nd1,
    "nd_chunk_minus_1": lambda: case_total(31, SCAN_CHUNK - 1),
    "nd_chunk": lambda: case_total(32, SCAN_CHUNK),
    "nd_chunk_plus_1": lambda: case_total(33, SCAN_CHUNK + 1, small=True),
    "nd_beyond_two_chunks": lambda: case_total(34, 2 * SCAN_CHUNK + 77),
}


def check_conditions(ref):
    """The builder's conditions (module docstring); returns the smallest distance of an OKS entry from a threshold."""
    thr = ref.params.iouThrs
    worst = np.inf
    for (img, cat), ious in ref.ious.items():
        if len(ious) == 0:
            continue
        worst = min(worst, float(np.min(np.abs(ious[:, :, None] - thr[None, None, :]))))
        gts = ref._gts[img, cat]
        key = [(tuple(g['keypoints']), g['area'], tuple(g['bbox'])) for g in gts]
        for row in ious:
            big = [j for j in range(len(row)) if row[j] >= 0.5]
            for x in range(len(big)):
                for y in range(x + 1, len(big)):
                    assert abs(row[big[x]] - row[big[y]]) > 1e-9 or key[big[x]] == key[big[y]], (img, big[x], big[y])
    assert worst >= 1e-9, worst
    assert not set(np.round(ref.stats, 15).tolist()) <= {-1.0, 0.0, 1.0}, ref.stats
    return worst


_built = {}


def case(name):
    """(gt, detections, evaluated restatement) of a case: built and checked once, shared and left unchanged."""
    if name not in _built:
        gt, dets = CASES[name]()
        ref = reference(gt, dets)
        check_conditions(ref)
        _built[name] = (gt, dets, ref)
    return _built[name]
