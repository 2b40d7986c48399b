"""Shared by tests/test_overlay_host.py (CPU) and tests/test_gpu_overlay.py: an independent NumPy reference of the pose overlay
(demo.py:119-124 with the package's stand-in rasteriser) and the frames and poses of its cases.

``render`` is written from the arithmetic the C header states, not from ``Pose.draw``: the host test holds the two against each
other.  Frames are seeded noise, so the blend shows in every channel of every painted pixel."""
import numpy as np

COCO_LIMBS = [[1, 2], [1, 5], [2, 3], [3, 4], [5, 6], [6, 7], [1, 8], [8, 9], [9, 10], [1, 11], [11, 12], [12, 13], [1, 0], [0, 14],
              [14, 16], [0, 15], [15, 17], [2, 16], [5, 17]]
COLOR, BOX_COLOR = (0, 224, 255), (0, 255, 0)
INT32_MAX, INT32_MIN = 2 ** 31 - 1, -2 ** 31


def noise_frames(n, h, w, seed):
    return np.random.RandomState(seed).randint(0, 256, (n, h, w, 3)).astype(np.uint8)


def painted_mask(h, w, keypoints, limbs):
    """Boolean (h, w): the pixels the skeletons of ``keypoints`` (P,K,2) paint.  Per limb the steps are evaluated as float64
    vectors (s / steps, * (b - a), + a: three separately rounded operations, as NumPy's scalars do them) and only the steps whose
    radius-1 stamp can touch the frame are kept: the in-frame step range, which makes far-outside end points affordable."""
    mask = np.zeros((h, w), bool)

    def stamps(cx, cy, r):
        for oy in range(-r, r + 1):
            for ox in range(-r, r + 1):
                if ox * ox + oy * oy > r * r:
                    continue
                x, y = cx + ox, cy + oy
                ok = (x >= 0) & (x < w) & (y >= 0) & (y < h)
                mask[y[ok], x[ok]] = True

    for kp in (np.asarray(keypoints, dtype=np.int64) if len(keypoints) else []):
        for a, b in limbs:
            (ax, ay), (bx, by) = (int(v) for v in kp[a]), (int(v) for v in kp[b])
            if ax != -1:
                stamps(np.array([ax]), np.array([ay]), 3)
            if bx != -1:
                stamps(np.array([bx]), np.array([by]), 3)
            if ax == -1 or bx == -1:
                continue
            steps = max(abs(bx - ax), abs(by - ay), 1)
            for s0 in range(0, steps + 1, 1 << 20):
                t = np.arange(s0, min(s0 + (1 << 20), steps + 1), dtype=np.float64) / float(steps)
                cx = np.trunc(float(ax) + float(bx - ax) * t).astype(np.int64)
                cy = np.trunc(float(ay) + float(by - ay) * t).astype(np.int64)
                near = (cx >= -1) & (cx <= w) & (cy >= -1) & (cy <= h)
                stamps(cx[near], cy[near], 1)
    return mask


def render(frame, keypoints, bbox, limbs, color=COLOR, box_color=BOX_COLOR, boxes=True):
    """The annotated frame: (6 src + 4 colour + 5) // 10 on painted pixels, src elsewhere, then the box outlines."""
    h, w = frame.shape[:2]
    out = frame.copy()
    m = painted_mask(h, w, keypoints, limbs)
    out[m] = ((6 * frame[m].astype(np.int64) + 4 * np.asarray(color, np.int64) + 5) // 10).astype(np.uint8)
    if boxes:
        for x, y, bw, bh in np.asarray(bbox, dtype=np.int64).reshape(-1, 4).tolist():
            x0, x1, y0, y1 = min(x, x + bw), max(x, x + bw), min(y, y + bh), max(y, y + bh)
            xs = slice(max(x0, 0), max(min(x1, w - 1) + 1, 0))        # (a stop below 0 would count from the end)
            ys = slice(max(y0, 0), max(min(y1, h - 1) + 1, 0))
            for yy in (y0, y1):
                if 0 <= yy < h:
                    out[yy, xs] = box_color
            for xx in (x0, x1):
                if 0 <= xx < w:
                    out[ys, xx] = box_color
    return out


def bbox_of(keypoints):
    """(P,4) int32 boxes as the pose tail computes them: over key-points with x != -1, (0,0,0,0) if none."""
    out = np.zeros((len(keypoints), 4), np.int32)
    for i, kp in enumerate(np.asarray(keypoints, dtype=np.int64)):
        pts = kp[kp[:, 0] != -1]
        if len(pts):
            lo, hi = pts.min(axis=0), pts.max(axis=0)
            out[i] = (lo[0], lo[1], hi[0] - lo[0] + 1, hi[1] - lo[1] + 1)
    return out


def pose(K=18, **pts):
    """(K,2) int32 of -1 with the key-point types named k<type>=(x, y) filled in."""
    kp = np.full((K, 2), -1, np.int32)
    for name, xy in pts.items():
        kp[int(name[1:])] = xy
    return kp


def edge_poses(h, w):
    """Five COCO poses for an h x w frame.  With types 0, 1, 2, 5, 8, 11 absent the limbs (3,4), (6,7), (9,10), (12,13), (14,16)
    and (15,17) are six independent segments per pose."""
    r, b = w - 1, h - 1
    return np.stack([
        # horizontal, vertical, 45 degrees, steep upwards, shallow right-to-left, zero length
        pose(k3=(5, 10), k4=(w - 10, 10), k6=(w - 8, 3), k7=(w - 8, h - 4), k9=(4, 2), k10=(4 + h - 6, h - 4),
             k12=(w // 2 + 3, h - 2), k13=(w // 2, 1), k14=(w - 3, h // 2 + 3), k16=(6, h // 2), k15=(w // 2, h // 2), k17=(w // 2, h // 2)),
        # one end missing; the four corners (border rows and columns); a limb crossing pose 0's 45-degree one
        pose(k3=(12, 15), k6=(0, 0), k7=(r, b), k9=(0, b), k10=(r, 0), k12=(4 + h - 6, 2), k13=(4, h - 4)),
        # negative coordinates other than -1; y == -1 with x present (present); x == -1 with y present (missing)
        pose(k3=(-2, 5), k4=(10, -7), k6=(7, -1), k7=(20, 12), k9=(-1, 10), k10=(15, 20)),
        # both ends outside, crossing the frame; both outside on the same side, left and right: box wholly outside
        pose(k12=(-10, -5), k13=(w + 8, h + 6), k14=(-20, 5), k16=(-6, h + 9), k15=(w + 5, -3), k17=(w + 30, 20)),
        # nothing found: box (0,0,0,0) paints pixel (0,0)
        pose(),
    ])


def batch_poses(n, h, w):
    """Per frame the pose arrays of a batch of n: frame 0 has none, frame 1 one, the last frame all five (n == 1: all five)."""
    all5 = edge_poses(h, w)
    return [all5][:n] if n == 1 else [all5[:0], all5[1:2], all5][:n]


EDGE_SHAPES = [(24, 40), (37, 53), (64, 96)]


def long_limb_poses():
    """200 x 320: a limb of 305 steps and one of 130."""
    return np.stack([pose(k3=(5, 10), k4=(310, 190), k6=(10, 150), k7=(100, 20))])


def crowd256():
    """16 x 16 with 256 poses (the tail's capacity): seeded key-points spread over a 216 x 216 area around the frame, four in
    five missing, so that the poses leave part of the small frame unpainted."""
    rs = np.random.RandomState(256)
    kp = rs.randint(-100, 116, (256, 18, 2)).astype(np.int32)
    kp[rs.rand(256, 18) < 0.8] = -1
    return kp


def far_poses():
    """24 x 40, end points at +-2^20: a segment through the frame, one that ends inside it, one that stays far away."""
    M = 1 << 20
    return np.stack([pose(k3=(-M, -M // 2), k4=(M, M // 2 + 7), k6=(M, 5), k7=(10, 12), k9=(M, M), k10=(M + 5, M - 9))])


def saturated_poses():
    """24 x 40, rows saturated at int32: the diagonal x == y through the frame's corner, and a vertical far to the right."""
    return np.stack([pose(k3=(INT32_MIN, INT32_MIN), k4=(INT32_MAX, INT32_MAX), k6=(INT32_MAX, INT32_MAX), k7=(INT32_MAX, INT32_MIN))])
