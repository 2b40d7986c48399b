"""Shared by test_crowd_mask_host.py and test_gpu_crowd_mask.py: a NumPy restatement of pycocotools' uncompressed-RLE decode
(maskApi.c rleDecode, and datasets/coco.py:17-21 around it) that keeps the original's loop over the runs, an encoder that builds
RLE dicts from boolean grids, and the named case table.  pycocotools is not a dependency: the restatement is pinned to
closed-form cases in test_crowd_mask_host.py and is otherwise UNPINNED against pycocotools itself.  Nothing here needs a GPU.

The launch of the crowd-mask kernel has one form at every size (a grid over the tiles of the batch's largest image, no loop
over tiles), so the table holds no case for a second trip of a loop; the two forms it does have, run ends staged in LDS or
searched in global memory, are the "lds_*" cases."""
import numpy as np

LDS_RUNS = 4096       # kCrowdRunsLds of csrc/lwp_internal.h: run ends of one image that a workgroup stages in LDS


# ---------------------------------------------------------------------------------------------- the restatement
def rle_decode(counts, h, w):
    """maskApi.c rleDecode: the buffer starts as zeros, the value starts at 0 and flips after every run, runs follow one
    another in memory; the buffer is an h x w image in column-major order.  Returns uint8 (h, w)."""
    M = np.zeros(h * w, dtype=np.uint8)
    p, v = 0, 0
    for c in counts:
        for _ in range(int(c)):
            M[p] = v
            p += 1
        v = 1 - v
    return M.reshape((h, w), order="F")


def get_mask_ref(segmentations, mask, decode=rle_decode, only_last=False):
    """coco.py:17-21 with the decode above.  ``decode`` and ``only_last`` exist for the mutation checks."""
    segmentations = list(segmentations)
    for segmentation in (segmentations[-1:] if only_last else segmentations):
        h, w = segmentation["size"]
        mask[decode(segmentation["counts"], h, w) > 0.5] = 0
    return mask


def search_decode(counts, h, w, side="right", row_major=False):
    """The decode as the kernel states it: the run of position p is the first j with e(j) > p (an upper-bound search over the
    running sums), the pixel is covered when j is odd, nothing is covered past the last end.  ``side="left"`` (a lower-bound
    search) and ``row_major`` (position y * w + x) are the mutants."""
    ends = np.cumsum(np.asarray(counts, dtype=np.int64))
    y, x = np.mgrid[0:h, 0:w]
    p = y * w + x if row_major else x * h + y
    j = np.searchsorted(ends, p, side=side)
    return ((j < len(ends)) & (j % 2 == 1)).astype(np.uint8)


def rle_encode(grid):
    """Boolean (h, w) grid -> {"counts", "size"}: column-major runs that start with zeros (a leading 0 when the first pixel is
    set), as maskApi.c rleEncode makes them."""
    grid = np.asarray(grid).astype(bool)
    flat = grid.reshape(-1, order="F")
    counts, v, run = [], False, 0
    for b in flat:
        if b != v:
            counts.append(run)
            v, run = b, 0
        run += 1
    counts.append(run)
    return {"counts": [int(c) for c in counts], "size": [int(grid.shape[0]), int(grid.shape[1])]}


def rle(counts, h, w):
    return {"counts": list(counts), "size": [h, w]}


# ---------------------------------------------------------------------------------------------- the cases
def blob_grid(h, w, seed, n=4):
    g = np.random.default_rng(seed)
    grid = np.zeros((h, w), dtype=bool)
    for _ in range(n):
        y0, x0 = int(g.integers(0, h)), int(g.integers(0, w))
        y1, x1 = y0 + int(g.integers(1, max(h // 2, 2))), x0 + int(g.integers(1, max(w // 2, 2)))
        grid[y0:y1, x0:x1] = True
    grid ^= g.random((h, w)) < 0.05                    # speckle: many short runs as well
    return grid


def one(h, w, *segs):
    return [(h, w)], [list(segs)]


def _three_overlapping():
    h, w = 9, 11
    grids = [np.zeros((h, w), dtype=bool) for _ in range(3)]
    grids[0][1:6, 2:7] = True
    grids[1][4:9, 5:11] = True
    grids[2][0:5, 0:4] = True
    return one(h, w, *[rle_encode(g) for g in grids])


def _empty_between():
    return [(6, 9), (5, 7), (8, 4)], [[rle_encode(blob_grid(6, 9, 1))], [], [rle_encode(blob_grid(8, 4, 2)), rle(list(range(5)), 8, 4)]]


def _mixed_sizes():
    sizes = [(3, 70), (41, 5), (1, 1), (33, 65), (12, 12)]
    return sizes, [[rle_encode(blob_grid(h, w, 10 + i))] for i, (h, w) in enumerate(sizes)]


def _checker(n_runs, h=65):
    """n_runs runs of one pixel in an image of odd height: a checkerboard down to where the runs stop, zeros (mask 1) after."""
    w = -(-(n_runs + 3) // h)
    return one(h, w, rle([1] * n_runs, h, w))


def _two_segments(total):
    """Two segmentations of one image whose run ends together number ``total``: the table is per image, not per segmentation."""
    h, a = 65, total // 2
    w = -(-(total + 3) // h)
    return one(h, w, rle([1] * a, h, w), rle([2] + [1] * (total - a - 1), h, w))


CASES = {
    # column-major against row-major at the smallest sizes
    "1x1_set": lambda: one(1, 1, rle([0, 1], 1, 1)),
    "1x1_clear": lambda: one(1, 1, rle([1], 1, 1)),
    "1xW": lambda: one(1, 7, rle([2, 3, 1, 1], 1, 7)),
    "Hx1": lambda: one(7, 1, rle([0, 6, 1], 7, 1)),
    "5x3": lambda: one(5, 3, rle_encode(np.tril(np.ones((5, 3), dtype=bool), -1))),
    "3x5": lambda: one(3, 5, rle_encode(np.tril(np.ones((3, 5), dtype=bool), -1))),
    # ragged against any tile; more than one workgroup along x and along y
    "37x53": lambda: one(37, 53, rle_encode(blob_grid(37, 53, 3))),
    "45x131": lambda: one(45, 131, rle_encode(blob_grid(45, 131, 4, n=7))),
    # zero-length runs
    "leading_zero": lambda: one(4, 3, rle([0, 5, 7], 4, 3)),
    "zero_runs_start": lambda: one(4, 3, rle([0, 0, 0, 5, 2, 1], 4, 3)),
    "zero_runs_middle": lambda: one(4, 3, rle([3, 2, 0, 0, 4, 1], 4, 3), rle([2, 3, 0, 4, 1], 4, 3)),
    "zero_runs_end": lambda: one(4, 3, rle([5, 7, 0], 4, 3), rle([4, 5, 0, 0, 0], 4, 3)),
    "only_zero_runs": lambda: one(4, 3, rle([0, 0, 0], 4, 3)),
    # runs against the columns
    "column_boundary": lambda: one(6, 4, rle([6, 6, 12], 6, 4)),
    "spans_columns": lambda: one(5, 6, rle([3, 17, 10], 5, 6)),
    "all_ones": lambda: one(7, 9, rle([0, 63], 7, 9)),
    "all_zeros": lambda: one(7, 9, rle([63], 7, 9)),
    "no_runs": lambda: one(7, 9, rle([], 7, 9)),
    "short_tail": lambda: one(6, 5, rle([4, 5, 3, 2], 6, 5)),
    # the union, the batch
    "three_overlapping": _three_overlapping,
    "empty_between": _empty_between,
    "mixed_sizes": _mixed_sizes,
    # both forms of the run table
    "lds_exact": lambda: _checker(LDS_RUNS),
    "lds_plus_one": lambda: _checker(LDS_RUNS + 1),
    "lds_two_segments_exact": lambda: _two_segments(LDS_RUNS),
    "lds_two_segments_plus_one": lambda: _two_segments(LDS_RUNS + 1),
}

_EXPECTED = {}


def case(name):
    """(sizes, segmentations per image, expected float32 masks) of a named case; the expectation is computed once."""
    sizes, segs = CASES[name]()
    if name not in _EXPECTED:
        _EXPECTED[name] = [get_mask_ref(s, np.ones(hw, dtype=np.float32)) for hw, s in zip(sizes, segs)]
    return sizes, segs, _EXPECTED[name]
