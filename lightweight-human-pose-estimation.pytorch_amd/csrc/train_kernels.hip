// Training targets and the per-stage masked L2 loss (datasets/coco.py:48,71-159, modules/loss.py, train.py:92-97) on the device.
// The targets reproduce CPython's double arithmetic statement by statement: this translation unit is built with
// -ffp-contract=off (build.py), and the pragma below says the same to the front end.
#include <cmath>

#include "lwp_internal.h"

#pragma clang fp contract(off)

namespace lwp {

// ------------------------------------------------------------------------------------------------ targets
// Python's int(): truncation toward zero.  The clamp keeps the cast defined for coordinates far outside the frame; every
// caller clamps the result into the map afterwards, so +-2^30 decides like the unclamped value.
__device__ inline int py_int(double v) { return (int)fmin(fmax(v, -1073741824.0), 1073741824.0); }
__device__ inline int floordiv(int a, int b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }   // Python's //, b > 0

// One thread per (frame, output pixel).  The frame's persons pass through LDS in chunks of kTrainChunk: per key-point
// (x, y, x / stride, y / stride, visibility), so the pixel loops divide nothing that is the same for every pixel.  A pixel
// belongs to one thread for the whole kernel: the Gaussian sum of a channel is carried from chunk to chunk through that
// thread's own element of keypoint_maps, and a PAF hit of a later chunk overwrites the earlier one (the last person wins).
__global__ void __launch_bounds__(256) train_targets_kernel(TrainTargetsParams p) {
    extern __shared__ double s_kp[];                   // [kTrainChunk][K][5]
    const int n = blockIdx.y, K = p.K, L = p.L, hw = p.h * p.w;
    const int pix = blockIdx.x * 256 + threadIdx.x;
    const bool active = pix < hw;
    const int my = active ? pix / p.w : 0, mx = active ? pix - my * p.w : 0;
    const int P = min(max(p.n_persons[n], 0), p.Pmax);
    float* kmap = p.keypoint_maps + (size_t)n * (K + 1) * hw + pix;
    float* pmap = p.paf_maps + (size_t)n * 2 * L * hw + pix;
    const double stride = (double)p.stride, sigma = p.sigma, thick = p.thickness;
    const double shift = stride / 2 - 0.5, reach = 4 * sigma;
    const double cx = (double)(mx * p.stride) + shift, cy = (double)(my * p.stride) + shift;
    const int lim_x = p.w * p.stride, lim_y = p.h * p.stride;
    float bg_max = 0.f;
    for (int c0 = 0; c0 == 0 || c0 < P; c0 += kTrainChunk) {
        const int cnt = min(kTrainChunk, P - c0);
        const bool last = c0 + kTrainChunk >= P;
        const double* src = p.kpts + ((size_t)n * p.Pmax + c0) * K * 3;
        for (int i = threadIdx.x; i < cnt * K; i += 256) {
            const double x = src[i * 3], y = src[i * 3 + 1];
            double* d = s_kp + i * 5;
            d[0] = x; d[1] = y; d[2] = x / stride; d[3] = y / stride; d[4] = src[i * 3 + 2];
        }
        __syncthreads();
        if (active) {
            // ---- _generate_keypoint_maps / _add_gaussian: per channel the persons in label order
            for (int k = 0; k < K; ++k) {
                float acc = c0 ? kmap[(size_t)k * hw] : 0.f;
                for (int q = 0; q < cnt; ++q) {
                    const double* d = s_kp + (q * K + k) * 5;
                    if (!(d[4] <= 1)) continue;
                    const double x = d[0], y = d[1];
                    const int tl0 = max(py_int(x - reach), 0), tl1 = max(py_int(y - reach), 0);
                    const int br0 = min(py_int(x + reach), lim_x), br1 = min(py_int(y + reach), lim_y);
                    if (mx < floordiv(tl0, p.stride) || mx >= floordiv(br0, p.stride) || my < floordiv(tl1, p.stride) ||
                        my >= floordiv(br1, p.stride))
                        continue;
                    const double d2 = (cx - x) * (cx - x) + (cy - y) * (cy - y);
                    const double exponent = d2 / 2 / sigma / sigma;
                    if (exponent > 4.6052) continue;
                    acc += (float)exp(-exponent);      // NumPy 2: the Python float is rounded to float32, then a float32 add
                    if (acc > 1.f) acc = 1.f;
                }
                kmap[(size_t)k * hw] = acc;
                if (last) bg_max = fmaxf(bg_max, acc);
            }
            // ---- _generate_paf_maps / _set_paf: per limb the persons in label order, a later hit overwrites
            if (c0 == 0)
                for (int c = 0; c < 2 * L; ++c) pmap[(size_t)c * hw] = 0.f;
            for (int l = 0; l < L; ++l) {
                const int4 lb = *(const int4*)(p.limbs + l * 4);
                bool hit = false;
                float vx = 0.f, vy = 0.f;
                for (int q = 0; q < cnt; ++q) {
                    const double* a = s_kp + (q * K + lb.x) * 5;
                    const double* b = s_kp + (q * K + lb.y) * 5;
                    if (!(a[4] <= 1) || !(b[4] <= 1)) continue;
                    const double x_a = a[2], y_a = a[3], x_b = b[2], y_b = b[3];
                    const int x_min = py_int(fmax(fmin(x_a, x_b) - thick, 0.0)), x_max = py_int(fmin(fmax(x_a, x_b) + thick, (double)p.w));
                    const int y_min = py_int(fmax(fmin(y_a, y_b) - thick, 0.0)), y_max = py_int(fmin(fmax(y_a, y_b) + thick, (double)p.h));
                    if (mx < x_min || mx >= x_max || my < y_min || my >= y_max) continue;
                    double x_ba = x_b - x_a, y_ba = y_b - y_a;
                    // Python's ** 0.5 is pow(); sqrt is the correctly rounded value pow() aims at
                    const double norm_ba = sqrt(x_ba * x_ba + y_ba * y_ba);
                    if (norm_ba < 1e-7) continue;
                    x_ba /= norm_ba;
                    y_ba /= norm_ba;
                    const double x_ca = (double)mx - x_a, y_ca = (double)my - y_a;
                    if (fabs(x_ca * y_ba - y_ca * x_ba) <= thick) { vx = (float)x_ba; vy = (float)y_ba; hit = true; }
                }
                if (hit) { pmap[(size_t)lb.z * hw] = vx; pmap[(size_t)lb.w * hw] = vy; }
            }
        }
        __syncthreads();
    }
    if (active) kmap[(size_t)K * hw] = 1.f - bg_max;   // keypoint_maps[-1] = 1 - keypoint_maps.max(axis=0), float32
}

hipError_t launch_train_targets(const TrainTargetsParams& p, int N, hipStream_t s) {
    const int hw = p.h * p.w;
    const size_t lds = (size_t)kTrainChunk * p.K * 5 * sizeof(double);      // <= 20 KB at K = 64
    hipLaunchKernelGGL(train_targets_kernel, dim3((hw + 255) / 256, N), dim3(256), lds, s, p);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ mask
// (N, H, W) -> (N, H / stride, W / stride): the mean of each stride x stride block (cv2.resize INTER_AREA by 1 / stride
// where the size divides, coco.py:48).  The block of a binary mask sums to an integer: exact in any order.
__global__ void __launch_bounds__(256) mask_downsample_kernel(const float* __restrict__ src, int W, int stride, int h, int w,
                                                               float* __restrict__ dst) {
    const int n = blockIdx.y, pix = blockIdx.x * 256 + threadIdx.x;
    if (pix >= h * w) return;
    const int y = pix / w, x = pix - y * w;
    const float* b = src + ((size_t)n * h * stride + (size_t)y * stride) * W + (size_t)x * stride;
    double sum = 0.0;
    for (int dy = 0; dy < stride; ++dy)
        for (int dx = 0; dx < stride; ++dx) sum += (double)b[(size_t)dy * W + dx];
    dst[(size_t)n * h * w + pix] = (float)(sum / (double)(stride * stride));
}

hipError_t launch_mask_downsample(const float* src, int N, int H, int W, int stride, float* dst, hipStream_t s) {
    const int h = H / stride, w = W / stride;
    hipLaunchKernelGGL(mask_downsample_kernel, dim3((h * w + 255) / 256, N), dim3(256), 0, s, src, W, stride, h, w, dst);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ loss
// sum(((out - target) * mask)^2 / 2 / batch) of up to kLossMaxOuts stage tensors in one pass: a thread owns (frame, pixel)
// positions, reads the mask value once per position and each target element once for all stages; every term and every sum
// is float64.  Fixed order throughout: the grid is a function of the problem size alone, a thread walks its positions and
// channels in order, the wave folds by shuffles, thread 0 adds the four wave sums in order and stores the workgroup's partial;
// stage_loss_reduce_kernel then adds the partials of a stage in index order.  No atomics: same inputs, same bits.
__device__ inline double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

__global__ void __launch_bounds__(256) stage_loss_kernel(StageLossParams p) {
    __shared__ double s_part[kLossMaxOuts][4];
    double acc[kLossMaxOuts];
#pragma unroll
    for (int s = 0; s < kLossMaxOuts; ++s) acc[s] = 0.0;
    const int64_t total = (int64_t)p.N * p.hw;
    const double batch = (double)p.batch;
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < total; q += (int64_t)gridDim.x * 256) {
        const int64_t n = q / p.hw, pix = q - n * p.hw;
        const double m = (double)p.mask[q];
#pragma unroll
        for (int kind = 0; kind < 2; ++kind) {
            const int C = kind ? p.CP : p.CH;
            const float* tg = kind ? p.paf_maps : p.keypoint_maps;
            if (!tg) continue;
            const int64_t base = n * C * p.hw + pix;
            for (int c = 0; c < C; ++c) {
                const int64_t at = base + (int64_t)c * p.hw;
                const double t = (double)tg[at];
#pragma unroll
                for (int s = kind; s < kLossMaxOuts; s += 2) {
                    if (s < p.S && p.outs[s]) {
                        const double d = ((double)p.outs[s][at] - t) * m;
                        acc[s] += d * d / 2 / batch;
                    }
                }
            }
        }
    }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int s = 0; s < kLossMaxOuts; ++s) {
        const double v = wave_sum(acc[s]);
        if (lane == 0) s_part[s][wv] = v;
    }
    __syncthreads();
    if (threadIdx.x < kLossMaxOuts && (int)threadIdx.x < p.S) {
        const int s = threadIdx.x;
        p.partials[(size_t)s * gridDim.x + blockIdx.x] = ((s_part[s][0] + s_part[s][1]) + s_part[s][2]) + s_part[s][3];
    }
}

// With `log` the same thread also adds its stage's sum / divisor to the handle's running log (lwp_stage_losses_log), in float64,
// and thread 0 counts the add when `adds` is given: one thread per entry, launches in stream order, no atomics.  The sum stored
// in `losses` is the same with or without a log.
__global__ void __launch_bounds__(64) stage_loss_reduce_kernel(const double* __restrict__ partials, int blocks, int S, double* __restrict__ losses,
                                                               double* __restrict__ log, double divisor, int64_t* __restrict__ adds) {
    const int s = threadIdx.x;
    if (s >= S) return;
    double sum = 0.0;
    for (int b = 0; b < blocks; ++b) sum += partials[(size_t)s * blocks + b];
    losses[s] = sum;
    if (log) log[s] += sum / divisor;
    if (adds && s == 0) adds[0] += 1;
}

int stage_loss_blocks(int N, int hw) {
    const int64_t need = ((int64_t)N * hw + 255) / 256;
    return (int)(need < 1 ? 1 : (need > kLossMaxBlocks ? kLossMaxBlocks : need));
}

hipError_t launch_stage_losses(const StageLossParams& p, double* losses, hipStream_t s, double* log, double divisor, int64_t* adds) {
    const int blocks = stage_loss_blocks(p.N, p.hw);
    hipLaunchKernelGGL(stage_loss_kernel, dim3(blocks), dim3(256), 0, s, p);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(stage_loss_reduce_kernel, dim3(1), dim3(64), 0, s, (const double*)p.partials, blocks, p.S, losses, log, divisor, adds);
    return hipGetLastError();
}

}  // namespace lwp
