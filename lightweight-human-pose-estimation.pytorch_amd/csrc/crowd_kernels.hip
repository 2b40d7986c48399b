// Crowd masks on the device (datasets/coco.py:17-21, get_mask): the float32 loss mask of every image of a batch, 1 where no
// crowd segmentation covers the pixel and 0 where any does, rendered from the run ends of the uncompressed RLEs.
// An RLE walks the image column by column (pixel (y, x) is position x * h + y) in runs that alternate between zeros and ones and
// start with zeros; run j covers positions [e(j - 1), e(j)) with e the running sum of the counts, which the host computes.
// A thread owns kCrowdStrip rows of one column, which are kCrowdStrip consecutive positions: one upper-bound search for the
// first, a forward walk for the rest.  Lanes run along x, so each row a wave stores is 256 contiguous bytes of the row-major mask.
#include "lwp_internal.h"

namespace lwp {

// bit r: position p + r lies in an odd run of the n run ends at e.  The run of a position is the first j with e[j] > position:
// equal neighbouring ends (zero-length runs) are stepped over and cannot flip the parity; past the last end everything is zero.
__device__ inline unsigned crowd_strip(const unsigned* e, int n, unsigned p, int rows) {
    int j = 0, hi = n;
    while (j < hi) {
        const int mid = (j + hi) >> 1;
        if (e[mid] > p) hi = mid; else j = mid + 1;
    }
    unsigned bits = 0;
    for (int r = 0; r < rows && j < n; ++r) {
        while (j < n && e[j] <= p + r) ++j;
        if (j < n) bits |= (unsigned)(j & 1) << r;
    }
    return bits;
}

__global__ void __launch_bounds__(256) crowd_mask_kernel(const unsigned* __restrict__ ends, const unsigned* __restrict__ seg_off,
                                                         const CrowdImage* __restrict__ images, float* __restrict__ masks) {
    __shared__ unsigned lds[kCrowdRunsLds];
    const CrowdImage im = images[blockIdx.z];
    // the grid covers the largest image of the batch: a workgroup outside this one leaves as a whole, before the barrier
    if ((int)blockIdx.x * 64 >= im.w || (int)blockIdx.y * 4 * kCrowdStrip >= im.h) return;
    const unsigned r0 = seg_off[im.seg0], nr = seg_off[im.seg0 + im.n_seg] - r0;
    const bool staged = nr <= (unsigned)kCrowdRunsLds;
    if (staged) {
        for (unsigned i = threadIdx.x; i < nr; i += 256) lds[i] = ends[r0 + i];
        __syncthreads();
    }
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = (blockIdx.y * 4 + (threadIdx.x >> 6)) * kCrowdStrip;
    if (x >= im.w || y >= im.h) return;
    const int rows = min(kCrowdStrip, im.h - y);
    const unsigned p = (unsigned)x * im.h + y;
    unsigned covered = 0;                              // the union: get_mask zeroes segmentation after segmentation
    for (unsigned s = 0; s < im.n_seg; ++s) {
        const unsigned a = seg_off[im.seg0 + s], n = seg_off[im.seg0 + s + 1] - a;
        covered |= staged ? crowd_strip(lds + (a - r0), (int)n, p, rows) : crowd_strip(ends + a, (int)n, p, rows);
    }
    float* o = masks + im.out + (size_t)y * im.w + x;
    for (int r = 0; r < rows; ++r) o[(size_t)r * im.w] = (covered >> r) & 1 ? 0.f : 1.f;
}

hipError_t launch_crowd_masks(const CrowdLaunch& c, hipStream_t s) {
    if (c.n_images == 0) return hipSuccess;
    // a wave covers 64 consecutive x, a workgroup four strips of kCrowdStrip rows; z is the image.  No loop over tiles: the
    // launch has one form at every size
    hipLaunchKernelGGL(crowd_mask_kernel, dim3((c.max_w + 63) / 64, (c.max_h + 4 * kCrowdStrip - 1) / (4 * kCrowdStrip), c.n_images),
                       dim3(256), 0, s, c.ends, c.seg_off, c.images, c.masks);
    return hipGetLastError();
}

}  // namespace lwp
