// Training augmentation on the device (datasets/transformations.py: Scale -> Rotate -> CropPad -> Flip; coco.py:48,63-65).
// One thread per pixel of the final crop: it undoes the flip and the crop offset, maps the warped-image pixel to its four
// fixed-point taps in the resized image, and evaluates each tap on demand from four source pixels with OpenCV's two-pass
// fixed-point resize.  Neither the resized nor the warped image exists in memory; the integers are those of the staged
// pipeline.  The coordinates restate NumPy's separately-rounded double arithmetic: this translation unit is built with
// -ffp-contract=off (build.py), and the pragma below says the same to the front end.
#include <cmath>

#include "lwp_internal.h"

#pragma clang fp contract(off)

namespace lwp {

// one axis of the resize for destination index d: the two clamped source indices and the weight of the second
struct ResizeTap { int i0, i1; float f; };
__device__ inline ResizeTap resize_tap(int d, int n, double scale, int area) {
    ResizeTap t;
    if (area) {
        t.i0 = min(2 * d, n - 1); t.i1 = min(t.i0 + 1, n - 1); t.f = 0.f;
        return t;
    }
    float f = (float)(((double)d + 0.5) * scale - 0.5);
    int i = (int)floorf(f);
    f = f - (float)i;
    if (i < 0) { i = 0; f = 0.f; }
    if (i >= n - 1) { i = n - 1; f = 0.f; }
    t.i0 = i; t.i1 = min(i + 1, n - 1); t.f = f;
    return t;
}

__global__ void __launch_bounds__(256) augment_kernel(const lwp_augment_plan* __restrict__ plans, int ch, int cw,
                                                      float* __restrict__ image, unsigned char* __restrict__ mask) {
    const int n = blockIdx.z;
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= cw || y >= ch) return;
    const lwp_augment_plan& p = plans[n];
    const int cx = p.flip ? cw - 1 - x : x;            // cv2.flip(.., 1): output x shows crop column cw - 1 - x
    int v[3] = {p.crop_pad[0], p.crop_pad[1], p.crop_pad[2]};
    int m = 1;
    if (p.should_crop && y >= p.dst_y0 && y < p.dst_y1 && cx >= p.dst_x0 && cx < p.dst_x1) {
        const double wy = (double)(p.img_y0 + (y - p.dst_y0)), wx = (double)(p.img_x0 + (cx - p.dst_x0));
        const int X = ((int)rint((p.m[1] * wy + p.m[2]) * 1024.0) + 16 + (int)rint(p.m[0] * wx * 1024.0)) >> 5;
        const int Y = ((int)rint((p.m[4] * wy + p.m[5]) * 1024.0) + 16 + (int)rint(p.m[3] * wx * 1024.0)) >> 5;
        const int sx = X >> 5, sy = Y >> 5, fi = X & 31, fj = Y & 31;
        const int wgt[4] = {32 * (32 - fi) * (32 - fj), 32 * fi * (32 - fj), 32 * (32 - fi) * fj, 32 * fi * fj};
        const float vx1 = (float)fi / 32.f, vy1 = (float)fj / 32.f, vx0 = 1.f - vx1, vy0 = 1.f - vy1;
        const float wf[4] = {vy0 * vx0, vy0 * vx1, vy1 * vx0, vy1 * vx1};
        const unsigned char* __restrict__ src = p.image;
        const float* __restrict__ msk = p.mask;
        const int W = p.src_w;
        ResizeTap tx[2], ty[2];
        for (int k = 0; k < 2; ++k) {
            tx[k] = resize_tap(min(max(sx + k, 0), p.rs_w - 1), p.src_w, p.rs_scale, p.area);
            ty[k] = resize_tap(min(max(sy + k, 0), p.rs_h - 1), p.src_h, p.rs_scale, p.area);
        }
        int acc[3] = {0, 0, 0};
        float tapm[4];
        for (int t = 0; t < 4; ++t) {
            const int ky = t >> 1, kx = t & 1;
            const bool inside = sy + ky >= 0 && sy + ky < p.rs_h && sx + kx >= 0 && sx + kx < p.rs_w;
            int px[3] = {p.warp_pad[0], p.warp_pad[1], p.warp_pad[2]};
            float pm = 1.f;
            if (inside) {
                const ResizeTap a = tx[kx], b = ty[ky];
                const unsigned char* r0 = src + (size_t)b.i0 * W * 3, * r1 = src + (size_t)b.i1 * W * 3;
                if (p.area) {
                    for (int c = 0; c < 3; ++c)
                        px[c] = ((int)r0[a.i0 * 3 + c] + (int)r0[a.i1 * 3 + c] + (int)r1[a.i0 * 3 + c] + (int)r1[a.i1 * 3 + c] + 2) >> 2;
                } else {
                    const int a1 = (int)rintf(a.f * 2048.f), a0 = (int)rintf((1.f - a.f) * 2048.f);
                    const int b1 = (int)rintf(b.f * 2048.f), b0 = (int)rintf((1.f - b.f) * 2048.f);
                    for (int c = 0; c < 3; ++c) {
                        const int q0 = (int)r0[a.i0 * 3 + c] * a0 + (int)r0[a.i1 * 3 + c] * a1;
                        const int q1 = (int)r1[a.i0 * 3 + c] * a0 + (int)r1[a.i1 * 3 + c] * a1;
                        px[c] = (((b0 * (q0 >> 4)) >> 16) + ((b1 * (q1 >> 4)) >> 16) + 2) >> 2;
                    }
                }
                if (msk) {
                    const float* m0 = msk + (size_t)b.i0 * W, * m1 = msk + (size_t)b.i1 * W;
                    if (p.area) {
                        pm = (((m0[a.i0] + m0[a.i1]) + m1[a.i0]) + m1[a.i1]) * 0.25f;
                    } else {
                        const float q0 = m0[a.i0] * (1.f - a.f) + m0[a.i1] * a.f;
                        const float q1 = m1[a.i0] * (1.f - a.f) + m1[a.i1] * a.f;
                        pm = q0 * (1.f - b.f) + q1 * b.f;
                    }
                }
            }
            for (int c = 0; c < 3; ++c) acc[c] += px[c] * wgt[t];
            tapm[t] = pm;
        }
        for (int c = 0; c < 3; ++c) v[c] = (acc[c] + (1 << 14)) >> 15;
        if (msk) {                                     // a NULL mask is all ones: exactly 1 after every stage
            const float wm = ((tapm[0] * wf[0] + tapm[1] * wf[1]) + tapm[2] * wf[2]) + tapm[3] * wf[3];
            m = (int)(unsigned char)(int)wm;           // the uint8 crop truncates: only 1.0 survives
        }
    }
    const size_t plane = (size_t)ch * cw, at = (size_t)y * cw + x;
    float* o = image + (size_t)n * 3 * plane + at;
    for (int c = 0; c < 3; ++c) o[c * plane] = ((float)v[c] - 128.f) / 256.f;
    mask[(size_t)n * plane + at] = (unsigned char)m;
}

// coco.py:48 on the uint8 mask: rint(float(block sum) * float(1 / stride^2)), round-half-even
__global__ void __launch_bounds__(256) augment_mask_small_kernel(const unsigned char* __restrict__ mask, int cw, int stride, int h,
                                                                 int w, float inv_area, float* __restrict__ dst) {
    const int n = blockIdx.y, pix = blockIdx.x * 256 + threadIdx.x;
    if (pix >= h * w) return;
    const int y = pix / w, x = pix - y * w;
    const unsigned char* b = mask + ((size_t)n * h * stride + (size_t)y * stride) * cw + (size_t)x * stride;
    int sum = 0;
    for (int dy = 0; dy < stride; ++dy)
        for (int dx = 0; dx < stride; ++dx) sum += b[(size_t)dy * cw + dx];
    dst[(size_t)n * h * w + pix] = rintf((float)sum * inv_area);
}

hipError_t launch_augment(const lwp_augment_plan* plans_device, int N, int crop_h, int crop_w, int stride, float* image,
                          unsigned char* mask, float* mask_small, hipStream_t s) {
    // a wave covers 64 consecutive x of one row, a workgroup four rows: every channel plane is written in 256-byte runs
    hipLaunchKernelGGL(augment_kernel, dim3((crop_w + 63) / 64, (crop_h + 3) / 4, N), dim3(256), 0, s, plans_device, crop_h, crop_w,
                       image, mask);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const int h = crop_h / stride, w = crop_w / stride;
    hipLaunchKernelGGL(augment_mask_small_kernel, dim3((h * w + 255) / 256, N), dim3(256), 0, s, mask, crop_w, stride, h, w,
                       (float)(1.0 / ((double)stride * stride)), mask_small);
    return hipGetLastError();
}

}  // namespace lwp
