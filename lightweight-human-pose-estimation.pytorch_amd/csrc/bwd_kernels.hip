// Stage backward (train.py:99-103 differentiated through initial_stage / refinement_stages, with_mobilenet.py:25-86), f32.
//
// Activations and gradients are NHWC windows (pointer + row stride), like the forward path.  Every GEMM here runs on
// v_mfma_f32_16x16x4_f32 (lane l: A[i = l & 15][k = l >> 4], B[k = l >> 4][j = l & 15], C[i = 4 (l >> 4) + r][j = l & 15]):
//   dgrad   dX[p][ci] = sum_tap sum_o dZ[p - off(tap)][o] * W[tap][o][ci]     M = pixels, N = cin, K = taps x cout
//   wgrad   dW[tap][o][ci] = sum_p dZ[p][o] * X[p + off(tap)][ci]            M = cout, N = cin, K = pixels (split over workgroups)
// A workgroup is 4 waves on a 64 x 64 output tile: wave w owns rows 16w .. 16w + 15 and four 16 x 16 accumulators (independent
// chains, so the 40-cycle dependent latency of the instruction is covered).  Operand tiles go through LDS, 16 deep.
// lwp_set_backward_precision puts dgrad and wgrad on v_mfma_f32_16x16x32_{bf16,f16} instead (dgrad_h16_kernel, wgrad_h16_kernel
// below: the same arrays, tiles, ranges and partials, operands rounded on their way into LDS); everything else stays f32.
// No floating-point atomics anywhere: wgrad writes per-split partial sums and a second kernel adds them in split order, so the
// same inputs give the same bits.
#include "lwp_internal.h"
#include "h16.h"
#include <type_traits>

namespace lwp {

// ---------------------------------------------------------------------------------------- loss gradient
// dL/d out = loss_scale * (out - target) * mask^2 / batch_size (modules/loss.py differentiated); targets NCHW, out and gradient NHWC
__global__ void __launch_bounds__(256) loss_grad_kernel(LossGradParams p) {
    const int s = blockIdx.y;
    const int C = (s & 1) ? p.CP : p.CH;
    const float* out = p.outs[s];
    const float* tgt = (s & 1) ? p.paf_maps : p.keypoint_maps;
    float* dst = p.dst[s];
    const int64_t total = (int64_t)p.N * C * p.hw;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int px = (int)(i % p.hw);
        const int64_t nc = i / p.hw;
        const int c = (int)(nc % C);
        const int64_t n = nc / C;
        const float m = p.mask[n * p.hw + px];
        const int64_t at = (n * p.hw + px) * p.ld + c;
        const float d = out[at] - tgt[i];
        dst[at] = d * m * m * p.scale;
    }
}

hipError_t launch_loss_grad(const LossGradParams& p, hipStream_t s) {
    if (p.S < 1 || p.S > kLossMaxOuts) return hipErrorInvalidValue;
    const int64_t total = (int64_t)p.N * (p.CH > p.CP ? p.CH : p.CP) * p.hw;
    const unsigned bx = (unsigned)std::min<int64_t>((total + 255) / 256, 4096);
    hipLaunchKernelGGL(loss_grad_kernel, dim3(bx, (unsigned)p.S), dim3(256), 0, s, p);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------- element-wise pieces
__global__ void __launch_bounds__(256) relu_mask_kernel(float* g, int g_ld, const float* y, int y_ld, const float* res, int res_ld,
                                                        int64_t M, int C) {
    const int64_t total = M * C;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t px = i / C;
        const int c = (int)(i % C);
        const float r = res ? res[px * res_ld + c] : 0.0f;
        if (!(y[px * y_ld + c] > r)) g[px * g_ld + c] = 0.0f;
    }
}
hipError_t launch_relu_mask(float* g, int g_ld, const float* y, int y_ld, const float* res, int res_ld, int64_t M, int C, hipStream_t s) {
    const unsigned bx = (unsigned)std::min<int64_t>((M * C + 255) / 256, 8192);
    hipLaunchKernelGGL(relu_mask_kernel, dim3(bx), dim3(256), 0, s, g, g_ld, y, y_ld, res, res_ld, M, C);
    return hipGetLastError();
}

__global__ void __launch_bounds__(256) grad_add_kernel(float* dst, int dst_ld, const float* src, int src_ld, int64_t M, int C, int beta) {
    const int64_t total = M * C;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t px = i / C;
        const int c = (int)(i % C);
        const float v = src[px * src_ld + c];
        float* d = dst + px * dst_ld + c;
        *d = beta ? *d + v : v;
    }
}
hipError_t launch_grad_add(float* dst, int dst_ld, const float* src, int src_ld, int64_t M, int C, int beta, hipStream_t s) {
    const unsigned bx = (unsigned)std::min<int64_t>((M * C + 255) / 256, 8192);
    hipLaunchKernelGGL(grad_add_kernel, dim3(bx), dim3(256), 0, s, dst, dst_ld, src, src_ld, M, C, beta);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------- data gradient
constexpr int BW_T = 64;       // output tile edge
constexpr int BW_K = 16;       // K depth of one LDS stage
constexpr int BW_APAD = 17;    // dgrad A tile [64 pixels][16 + 1]
constexpr int BW_BPAD = 68;    // [16][64 + 4] tiles

__global__ void __launch_bounds__(256) dgrad_kernel(DgradParams p) {
    __shared__ float As[BW_T * BW_APAD];
    __shared__ float Bs[BW_K * BW_BPAD];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int HW = p.H * p.W;
    const int64_t M = (int64_t)p.N * HW;
    const int64_t m0 = (int64_t)blockIdx.x * BW_T;
    const int ci0 = blockIdx.y * BW_T;
    // this thread's A-load row: one pixel of the tile, four consecutive k
    const int arow = t >> 2, ak = (t & 3) * 4;
    const int64_t am = m0 + arow;
    const bool a_in = am < M;
    int an = 0, ay = 0, ax = 0;
    if (a_in) { an = (int)(am / HW); const int r = (int)(am % HW); ay = r / p.W; ax = r % p.W; }
    // B-load: row k of the stage, four consecutive input channels
    const int brow = t >> 4, bn = (t & 15) * 4;
    const bool b_in = ci0 + bn < p.cin_pad;
    f32x4 acc[4] = {{0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}};
    const int half = p.ks / 2;
    for (int tap = 0; tap < p.ks * p.ks; ++tap) {
        // forward: Y[q] takes X[q + (k - half) * dil], so dX[q] takes dZ[q - (k - half) * dil]
        const int sy = ay - (tap / p.ks - half) * p.dil, sx = ax - (tap % p.ks - half) * p.dil;
        const bool a_ok = a_in && sy >= 0 && sy < p.H && sx >= 0 && sx < p.W;
        const float* arow_ptr = p.dz + ((int64_t)an * HW + (int64_t)sy * p.W + sx) * p.dz_ld;
        const float* wt = p.w + (size_t)tap * p.cout_pad * p.cin_pad;
        for (int o0 = 0; o0 < p.cout; o0 += BW_K) {
            float av[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) av[j] = (a_ok && o0 + ak + j < p.cout) ? arow_ptr[o0 + ak + j] : 0.0f;
            f32x4 bv = {0, 0, 0, 0};
            if (b_in) bv = *(const f32x4*)(wt + (size_t)(o0 + brow) * p.cin_pad + ci0 + bn);   // rows < cout_pad (a multiple of 64), zero beyond cout
            __syncthreads();
#pragma unroll
            for (int j = 0; j < 4; ++j) As[arow * BW_APAD + ak + j] = av[j];
            *(f32x4*)(Bs + brow * BW_BPAD + bn) = bv;
            __syncthreads();
#pragma unroll
            for (int kk = 0; kk < BW_K; kk += 4) {
                const float a = As[(16 * wv + (lane & 15)) * BW_APAD + kk + (lane >> 4)];
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, Bs[(kk + (lane >> 4)) * BW_BPAD + 16 * j + (lane & 15)], acc[j], 0, 0, 0);
            }
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int ci = ci0 + 16 * j + (lane & 15);
        if (ci >= p.cin) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int64_t m = m0 + 16 * wv + 4 * (lane >> 4) + r;
            if (m >= M) continue;
            float* d = p.dx + m * p.dx_ld + ci;
            *d = ci >= p.acc_from ? *d + acc[j][r] : acc[j][r];
        }
    }
}

// ---------------------------------------------------------------------------------------- 16-bit operands (lwp_set_backward_precision)
// The same tiles, grids, windows and pixel ranges on v_mfma_f32_16x16x32_{bf16,f16}: lane l holds A[i = l & 15][k = 8 (l >> 4) .. + 7]
// and B[k = 8 (l >> 4) .. + 7][j = l & 15], C as above.  The operands stay f32 in memory; each is rounded once, (T)v, on its way
// into LDS, dZ after its multiplication by grad_scale; the f32 accumulator is multiplied by 1 / grad_scale before it is stored or
// added (both exact: the scale is a power of two).  A stage is 32 deep.  Both LDS tiles are [64 rows][32 k] of 16 bits, k along the
// row whatever the operand's order in memory: thread t stages row t >> 2, k = 8 (t & 3) .. + 7, eight dword loads (along the
// memory row where k runs along it: dgrad's dZ; one per memory row where k runs across: dgrad's W, both operands of wgrad) and
// one 16-byte LDS store, so the transposition costs nothing beyond the address.  A lane then reads its 8 k with one ds_read_b128.
// Rows are 64 bytes, four 16-byte chunks; chunk q of row r sits at q ^ f(r >> 2 & 3), f = (0, 2, 3, 1): the 16 lanes a
// ds_read_b128 serves together ({0-3, 12-15, 20-27}, ...: eight rows at one chunk, eight at its neighbour) then fall on 16
// different 16-byte slots of the 256-byte bank row, and the 8 lanes of a store (two rows, four chunks) on 128 contiguous bytes.
constexpr int BH_K = 32;
__device__ __forceinline__ int bh_at(int row, int q) { return row * BH_K + 8 * (q ^ ((0x78 >> (2 * ((row >> 2) & 3))) & 3)); }
template <typename T> __device__ __forceinline__ void bh_store(T* tile, int row, int q, const float (&v)[8]) {
    typename H16<T>::x8 h;
#pragma unroll
    for (int j = 0; j < 8; ++j) h[j] = (T)v[j];
    *(typename H16<T>::x8*)(tile + bh_at(row, q)) = h;
}
// fp16 subnormals.  The MFMA aligns its 32 products to the largest NOMINAL exponent, a subnormal operand counting with the
// exponent field of 2^-14, and keeps 24 bits below that: a product with a subnormal operand loses as many bits as the operand
// has leading zeros (measured: DESIGN 3q).  So a stage whose tiles hold a subnormal (bh_subnormal, or-ed over the workgroup by the
// stage's second barrier) runs four products instead of one: each fragment is split into its normal elements and its subnormal
// ones times 2^10 (exact: m 2^-24 -> m 2^-14, now normal), normal x normal goes to the accumulator, the two mixed products to a
// second one that stands for 2^-10 of its value, subnormal x subnormal to a third (2^-20).  The same operands, the same exact
// products, no further rounding point; a stage without subnormals (every stage of the integer fixtures) runs as before.  bf16's
// subnormals lie below 2^-126, where the f32 operands are subnormal themselves: no split there.
template <typename T> struct H16Split { static constexpr bool on = false; };
template <> struct H16Split<_Float16> { static constexpr bool on = true; };
template <typename T> __device__ __forceinline__ int bh_subnormal(const float (&v)[8]) {
    if constexpr (!H16Split<T>::on) return 0;
    int any = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float a = fabsf((float)(T)v[j]);
        any |= (a != 0.0f && a < 6.103515625e-05f) ? 1 : 0;      // below 2^-14
    }
    return any;
}
template <typename X8> __device__ __forceinline__ void bh_split(const X8& v, X8& normal, X8& sub) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const _Float16 h = v[j];
        const bool s = (__builtin_bit_cast(unsigned short, h) & 0x7C00) == 0;      // exponent field 0: a subnormal or a zero
        normal[j] = s ? (_Float16)0 : h;
        sub[j] = s ? h * (_Float16)1024 : (_Float16)0;
    }
}
// one stage of a wave's four 16 x 16 tiles: a and the four b fragments come from LDS
template <typename T> __device__ __forceinline__ void bh_products(const T* As, const T* Bs, int wv, int lane, int sub, f32x4 (&acc)[4],
                                                                 f32x4 (&acc1)[4], f32x4 (&acc2)[4]) {
    typedef typename H16<T>::x8 x8;
    const x8 a = *(const x8*)(As + bh_at(16 * wv + (lane & 15), lane >> 4));
    if constexpr (H16Split<T>::on) {
        if (sub) {
            x8 an, as;
            bh_split(a, an, as);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                x8 bn, bs;
                bh_split(*(const x8*)(Bs + bh_at(16 * j + (lane & 15), lane >> 4)), bn, bs);
                acc[j] = H16<T>::mfma16(an, bn, acc[j]);
                acc1[j] = H16<T>::mfma16(as, bn, acc1[j]);
                acc1[j] = H16<T>::mfma16(an, bs, acc1[j]);
                acc2[j] = H16<T>::mfma16(as, bs, acc2[j]);
            }
            return;
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = H16<T>::mfma16(a, *(const x8*)(Bs + bh_at(16 * j + (lane & 15), lane >> 4)), acc[j]);
}
// the value of an accumulator element: acc + 2^-10 acc1 + 2^-20 acc2 (the last two are zero without the split)
template <typename T> __device__ __forceinline__ float bh_value(float a, float a1, float a2) {
    if constexpr (H16Split<T>::on) return (a + a1 * 0.0009765625f) + a2 * 9.5367431640625e-07f;
    return a;
}

template <typename T> __global__ void __launch_bounds__(256) dgrad_h16_kernel(DgradParams p, float scale, float inv_scale) {
    __shared__ __attribute__((aligned(16))) T As[BW_T * BH_K];      // [pixel][cout channel]
    __shared__ __attribute__((aligned(16))) T Bs[BW_T * BH_K];      // [cin channel][cout channel]
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int HW = p.H * p.W;
    const int64_t M = (int64_t)p.N * HW;
    const int64_t m0 = (int64_t)blockIdx.x * BW_T;
    const int ci0 = blockIdx.y * BW_T;
    const int row = t >> 2, q = t & 3;
    const int64_t am = m0 + row;
    const bool a_in = am < M;
    int an = 0, ay = 0, ax = 0;
    if (a_in) { an = (int)(am / HW); const int r = (int)(am % HW); ay = r / p.W; ax = r % p.W; }
    const bool b_in = ci0 + row < p.cin;
    f32x4 acc[4] = {{0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}};
    f32x4 acc1[4] = {{0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}}, acc2[4] = {{0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}};
    const int half = p.ks / 2;
    for (int tap = 0; tap < p.ks * p.ks; ++tap) {
        const int sy = ay - (tap / p.ks - half) * p.dil, sx = ax - (tap % p.ks - half) * p.dil;
        const bool a_ok = a_in && sy >= 0 && sy < p.H && sx >= 0 && sx < p.W;
        const float* arow_ptr = p.dz + ((int64_t)an * HW + (int64_t)sy * p.W + sx) * p.dz_ld;
        const float* wt = p.w + (size_t)tap * p.cout_pad * p.cin_pad + ci0 + row;
        for (int o0 = 0; o0 < p.cout; o0 += BH_K) {
            float av[8], bv[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int o = o0 + 8 * q + j;
                av[j] = (a_ok && o < p.cout) ? arow_ptr[o] * scale : 0.0f;
                bv[j] = (b_in && o < p.cout) ? wt[(size_t)o * p.cin_pad] : 0.0f;
            }
            __syncthreads();
            bh_store(As, row, q, av);
            bh_store(Bs, row, q, bv);
            const int sub = H16Split<T>::on ? __syncthreads_or(bh_subnormal<T>(av) | bh_subnormal<T>(bv)) : (__syncthreads(), 0);
            bh_products<T>(As, Bs, wv, lane, sub, acc, acc1, acc2);
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int ci = ci0 + 16 * j + (lane & 15);
        if (ci >= p.cin) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int64_t m = m0 + 16 * wv + 4 * (lane >> 4) + r;
            if (m >= M) continue;
            float* d = p.dx + m * p.dx_ld + ci;
            const float v = bh_value<T>(acc[j][r], acc1[j][r], acc2[j][r]) * inv_scale;
            *d = ci >= p.acc_from ? *d + v : v;
        }
    }
}

static bool bwd_precision_ok(const BwdPrecision& bp) {
    return bp.dtype == LWP_F32 ? bp.scale == 1.0f : ((bp.dtype == LWP_BF16 || bp.dtype == LWP_F16) && bp.scale >= 1.0f && bp.scale <= 16777216.0f);
}

hipError_t launch_dgrad(const DgradParams& p, hipStream_t s, BwdPrecision bp) {
    const int64_t M = (int64_t)p.N * p.H * p.W;
    if (M < 1 || M >= (1ll << 31) - BW_T || p.cout < 1 || p.cin < 1 || p.cout > p.cout_pad || p.cin > p.cin_pad || (p.cin_pad & 3) ||
        (p.cout_pad % BW_K) || (p.ks != 1 && p.ks != 3) || !bwd_precision_ok(bp))
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)((M + BW_T - 1) / BW_T), (unsigned)((p.cin + BW_T - 1) / BW_T));
    if (bp.dtype == LWP_BF16) hipLaunchKernelGGL(dgrad_h16_kernel<__bf16>, grid, dim3(256), 0, s, p, bp.scale, 1.0f / bp.scale);
    else if (bp.dtype == LWP_F16) hipLaunchKernelGGL(dgrad_h16_kernel<_Float16>, grid, dim3(256), 0, s, p, bp.scale, 1.0f / bp.scale);
    else hipLaunchKernelGGL(dgrad_kernel, grid, dim3(256), 0, s, p);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------- weight and bias gradient
// bias: db[o] = sum over the split's pixels of dZ[p][o]; 4 pixel lanes per channel, added in lane order (red: 256 floats of LDS).
// The 16-bit kernel runs the same statement: the column sums read the unrounded, unscaled dZ in either mode.
__device__ __forceinline__ void wgrad_bias_sums(const WgradParams& p, float* red, int o0, int z, int64_t p_begin, int64_t p_end) {
    const int t = threadIdx.x, c = t & 63, pl = t >> 6;
    const int co_p = wgrad_pad64(p.cout), ci_p = wgrad_pad64(p.cin);
    float sum = 0.0f;
    if (o0 + c < p.cout)
        for (int64_t px = p_begin + pl; px < p_end; px += 4) sum += p.dz[px * p.dz_ld + o0 + c];
    red[pl * 64 + c] = sum;
    __syncthreads();
    if (t < 64) {
        float* bpart = p.partial + (size_t)p.splits * p.ks * p.ks * co_p * ci_p;
        bpart[(size_t)z * co_p + o0 + t] = ((red[t] + red[64 + t]) + red[128 + t]) + red[192 + t];
    }
}

// grid: x = cout tiles x cin tiles, y = tap (+ one extra row of workgroups for the bias column sums), z = pixel split
__global__ void __launch_bounds__(256) wgrad_kernel(WgradParams p) {
    __shared__ float As[BW_K * BW_BPAD];      // [pixel][cout channel]
    __shared__ float Bs[BW_K * BW_BPAD];      // [pixel][cin channel]
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int taps = p.ks * p.ks;
    const int co_p = wgrad_pad64(p.cout), ci_p = wgrad_pad64(p.cin);
    const int ci_t = ci_p / BW_T;
    const int o0 = (blockIdx.x / ci_t) * BW_T, c0 = (blockIdx.x % ci_t) * BW_T;
    const int tap = blockIdx.y, z = blockIdx.z;
    const int HW = p.H * p.W;
    const int64_t M = (int64_t)p.N * HW;
    const int64_t p_begin = (int64_t)z * p.chunk;
    const int64_t p_end = p_begin + p.chunk < M ? p_begin + p.chunk : M;
    if (tap == taps) {
        if (c0 == 0) wgrad_bias_sums(p, As, o0, z, p_begin, p_end);
        return;
    }
    const int half = p.ks / 2;
    const int dy = (tap / p.ks - half) * p.dil, dx = (tap % p.ks - half) * p.dil;
    const int lrow = t >> 4, lc = (t & 15) * 4;       // this thread's load: pixel lrow of the stage, four consecutive channels
    f32x4 acc[4] = {{0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}};
    for (int64_t px0 = p_begin; px0 < p_end; px0 += BW_K) {
        const int64_t px = px0 + lrow;
        float av[4] = {0, 0, 0, 0}, bv[4] = {0, 0, 0, 0};
        if (px < p_end) {
            const float* zr = p.dz + px * p.dz_ld + o0 + lc;
#pragma unroll
            for (int j = 0; j < 4; ++j) if (o0 + lc + j < p.cout) av[j] = zr[j];
            const int n = (int)(px / HW), r = (int)(px % HW);
            const int sy = r / p.W + dy, sx = r % p.W + dx;
            if (sy >= 0 && sy < p.H && sx >= 0 && sx < p.W) {
                const float* xr = p.x + ((int64_t)n * HW + (int64_t)sy * p.W + sx) * p.x_ld + c0 + lc;
#pragma unroll
                for (int j = 0; j < 4; ++j) if (c0 + lc + j < p.cin) bv[j] = xr[j];
            }
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 4; ++j) { As[lrow * BW_BPAD + lc + j] = av[j]; Bs[lrow * BW_BPAD + lc + j] = bv[j]; }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < BW_K; kk += 4) {
            const float a = As[(kk + (lane >> 4)) * BW_BPAD + 16 * wv + (lane & 15)];
#pragma unroll
            for (int j = 0; j < 4; ++j)
                acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, Bs[(kk + (lane >> 4)) * BW_BPAD + 16 * j + (lane & 15)], acc[j], 0, 0, 0);
        }
    }
    float* part = p.partial + (((size_t)z * taps + tap) * co_p + o0) * ci_p + c0;
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r)
            part[(size_t)(16 * wv + 4 * (lane >> 4) + r) * ci_p + 16 * j + (lane & 15)] = acc[j][r];
}

// pixel ranges of at least 64 pixels, as many as bring the grid to about four workgroups per CU
void wgrad_plan(int64_t M, int cout, int cin, int ks, int* splits, int* chunk) {
    const int64_t tiles = (int64_t)(wgrad_pad64(cout) / BW_T) * (wgrad_pad64(cin) / BW_T) * ks * ks;
    int64_t sp = (1024 + tiles - 1) / tiles;
    const int64_t max_sp = (M + 63) / 64;
    if (sp > max_sp) sp = max_sp;
    if (sp < 1) sp = 1;
    int64_t ch = ((M + sp - 1) / sp + BW_K - 1) / BW_K * BW_K;
    *chunk = (int)ch;
    *splits = (int)((M + ch - 1) / ch);
}

// wgrad_kernel's grid, ranges and partial layout on 16-bit operands (the rules are above dgrad_h16_kernel).  K is the pixel axis,
// across the memory rows of both operands; a range need not be a multiple of the 32-deep stage (pixels past p_end are zeros).
template <typename T> __global__ void __launch_bounds__(256) wgrad_h16_kernel(WgradParams p, float scale, float inv_scale) {
    __shared__ __attribute__((aligned(16))) T As[BW_T * BH_K];      // [cout channel][pixel]
    __shared__ __attribute__((aligned(16))) T Bs[BW_T * BH_K];      // [cin channel][pixel]
    __shared__ float red[256];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int taps = p.ks * p.ks;
    const int co_p = wgrad_pad64(p.cout), ci_p = wgrad_pad64(p.cin);
    const int ci_t = ci_p / BW_T;
    const int o0 = (blockIdx.x / ci_t) * BW_T, c0 = (blockIdx.x % ci_t) * BW_T;
    const int tap = blockIdx.y, z = blockIdx.z;
    const int HW = p.H * p.W;
    const int64_t M = (int64_t)p.N * HW;
    const int64_t p_begin = (int64_t)z * p.chunk;
    const int64_t p_end = p_begin + p.chunk < M ? p_begin + p.chunk : M;
    if (tap == taps) {
        if (c0 == 0) wgrad_bias_sums(p, red, o0, z, p_begin, p_end);
        return;
    }
    const int half = p.ks / 2;
    const int dy = (tap / p.ks - half) * p.dil, dx = (tap % p.ks - half) * p.dil;
    const int row = t >> 2, q = t & 3;
    const bool a_in = o0 + row < p.cout, b_in = c0 + row < p.cin;
    const float* zc = p.dz + o0 + row;
    const float* xc = p.x + c0 + row;
    f32x4 acc[4] = {{0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}};
    f32x4 acc1[4] = {{0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}}, acc2[4] = {{0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}};
    for (int64_t px0 = p_begin; px0 < p_end; px0 += BH_K) {
        const int64_t pf = px0 + 8 * q;                 // this thread's first pixel of the stage; (n, y, x) walks on from it
        int n = 0, y = 0, x = 0;
        if (pf < p_end) { n = (int)(pf / HW); const int r = (int)(pf % HW); y = r / p.W; x = r % p.W; }
        float av[8], bv[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const bool in = pf + j < p_end;
            const int sy = y + dy, sx = x + dx;
            av[j] = (in && a_in) ? zc[(pf + j) * p.dz_ld] * scale : 0.0f;
            bv[j] = (in && b_in && sy >= 0 && sy < p.H && sx >= 0 && sx < p.W) ? xc[((int64_t)n * HW + (int64_t)sy * p.W + sx) * p.x_ld] : 0.0f;
            if (++x == p.W) { x = 0; if (++y == p.H) { y = 0; ++n; } }
        }
        __syncthreads();
        bh_store(As, row, q, av);
        bh_store(Bs, row, q, bv);
        const int sub = H16Split<T>::on ? __syncthreads_or(bh_subnormal<T>(av) | bh_subnormal<T>(bv)) : (__syncthreads(), 0);
        bh_products<T>(As, Bs, wv, lane, sub, acc, acc1, acc2);
    }
    float* part = p.partial + (((size_t)z * taps + tap) * co_p + o0) * ci_p + c0;
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r)
            part[(size_t)(16 * wv + 4 * (lane >> 4) + r) * ci_p + 16 * j + (lane & 15)] = bh_value<T>(acc[j][r], acc1[j][r], acc2[j][r]) * inv_scale;
}

hipError_t launch_wgrad(const WgradParams& p, hipStream_t s, BwdPrecision bp) {
    const int64_t M = (int64_t)p.N * p.H * p.W;
    if (M < 1 || M >= (1ll << 31) - BW_T || p.cout < 1 || p.cin < 1 || (p.ks != 1 && p.ks != 3) || p.splits < 1 || p.splits > 65535 ||
        p.chunk < BW_K || (p.chunk % BW_K) || (int64_t)p.splits * p.chunk < M || !bwd_precision_ok(bp))
        return hipErrorInvalidValue;
    const unsigned tiles = (unsigned)((wgrad_pad64(p.cout) / BW_T) * (wgrad_pad64(p.cin) / BW_T));
    const dim3 grid(tiles, (unsigned)(p.ks * p.ks + (p.no_bias ? 0 : 1)), (unsigned)p.splits);
    if (bp.dtype == LWP_BF16) hipLaunchKernelGGL(wgrad_h16_kernel<__bf16>, grid, dim3(256), 0, s, p, bp.scale, 1.0f / bp.scale);
    else if (bp.dtype == LWP_F16) hipLaunchKernelGGL(wgrad_h16_kernel<_Float16>, grid, dim3(256), 0, s, p, bp.scale, 1.0f / bp.scale);
    else hipLaunchKernelGGL(wgrad_kernel, grid, dim3(256), 0, s, p);
    return hipGetLastError();
}

__global__ void __launch_bounds__(256) wgrad_reduce_kernel(WgradParams p, float* dw, float* db, int accumulate) {
    const int taps = p.ks * p.ks;
    const int co_p = wgrad_pad64(p.cout), ci_p = wgrad_pad64(p.cin);
    const int64_t nw = (int64_t)p.cout * p.cin * taps;
    const int64_t total = nw + (p.no_bias ? 0 : p.cout);
    const float* bpart = p.partial + (size_t)p.splits * taps * co_p * ci_p;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        float sum = 0.0f;
        float* d;
        if (i < nw) {                                   // OIHW: ((o * cin) + ci) * taps + tap
            const int tap = (int)(i % taps);
            const int64_t oc = i / taps;
            const int ci = (int)(oc % p.cin), o = (int)(oc / p.cin);
            for (int z = 0; z < p.splits; ++z) sum += p.partial[(((size_t)z * taps + tap) * co_p + o) * ci_p + ci];
            d = dw + i;
        } else {
            const int o = (int)(i - nw);
            for (int z = 0; z < p.splits; ++z) sum += bpart[(size_t)z * co_p + o];
            d = db + o;
        }
        *d = accumulate ? *d + sum : sum;
    }
}

hipError_t launch_wgrad_reduce(const WgradParams& p, float* dw, float* db, int accumulate, hipStream_t s) {
    const int64_t total = (int64_t)p.cout * p.cin * p.ks * p.ks + (p.no_bias ? 0 : p.cout);
    const unsigned bx = (unsigned)std::min<int64_t>((total + 255) / 256, 4096);
    hipLaunchKernelGGL(wgrad_reduce_kernel, dim3(bx), dim3(256), 0, s, p, dw, db, accumulate);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------- cpm: ELU
// (with_mobilenet.py:7-21; modules/conv.py:24-32 with bn=False: depthwise 3x3 + ELU, 1x1 + ELU.)  This and the depthwise family
// below are memory-bound element-wise and reduction shapes: a lane owns four consecutive channels of a pixel, every access is 16
// bytes, a wave covers whole rows.
__global__ void __launch_bounds__(256) elu_grad_kernel(float* g, int g_ld, const float* y, int y_ld, int64_t M, int C4) {
    const int64_t total = M * C4;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t px = i / C4;
        const int c = (int)(i % C4) * 4;
        f32x4* gp = (f32x4*)(g + px * g_ld + c);
        const f32x4 yv = *(const f32x4*)(y + px * y_ld + c);
        f32x4 gv = *gp;
#pragma unroll
        for (int k = 0; k < 4; ++k) gv[k] = gv[k] * (yv[k] > 0.0f ? 1.0f : yv[k] + 1.0f);
        *gp = gv;
    }
}
static bool quad_ok(const void* p, int ld) { return p && ((uintptr_t)p & 15) == 0 && ld > 0 && (ld & 3) == 0; }
hipError_t launch_elu_grad(float* g, int g_ld, const float* y, int y_ld, int64_t M, int C, hipStream_t s) {
    if (M < 1 || C < 4 || (C & 3) || C > g_ld || C > y_ld || !quad_ok(g, g_ld) || !quad_ok(y, y_ld)) return hipErrorInvalidValue;
    const unsigned bx = (unsigned)std::min<int64_t>((M * (C / 4) + 255) / 256, 8192);
    hipLaunchKernelGGL(elu_grad_kernel, dim3(bx), dim3(256), 0, s, g, g_ld, y, y_ld, M, C / 4);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------- depthwise 3x3, stride 1 | 2, dilation 1 | 2
// One family for the cpm's depthwise convs (stride 1, dilation 1, ELU behind them) and the backbone's (with_mobilenet.py:94-104:
// conv_dw, BatchNorm + ReLU behind it).  The forward is Z[n, oy, ox, c] = sum_k X[n, s oy + d (ky - 1), s ox + d (kx - 1), c] w[k][c]
// on an Ho x Wo map, Ho = (H - 1) / s + 1 (padding = dilation).  Stride and dilation are template arguments: the index arithmetic
// of a pair is compile-time, and at (1, 1) Ho x Wo is H x W itself.
template <typename F> static void dw_for_sd(int stride, int dil, F&& launch) {      // both 1 or 2 (dw_grad_shape_ok)
    typedef std::integral_constant<int, 1> I1;
    typedef std::integral_constant<int, 2> I2;
    if (stride == 1) { if (dil == 1) launch(I1(), I1()); else launch(I1(), I2()); }
    else { if (dil == 1) launch(I2(), I1()); else launch(I2(), I2()); }
}

// dX[n, y, x, c] = sum over taps of dZ[n, (y + d - d ky) / s, (x + d - d kx) / s, c] * w[tap][c]: one fmaf chain per output in tap
// order 0..8; a tap whose source index is not divisible by s or lies outside the Ho x Wo map contributes a zero
template <int S, int D> __global__ void __launch_bounds__(256) dw_dgrad_kernel(DwGradParams p) {
    const int C4 = p.C / 4;
    const int Ho = S == 1 ? p.H : p.Ho, Wo = S == 1 ? p.W : p.Wo;
    const int HW = p.H * p.W, HWo = Ho * Wo;
    const int64_t total = (int64_t)p.N * HW * C4;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t px = i / C4;
        const int c = (int)(i % C4) * 4;
        const int64_t n = px / HW;
        const int r = (int)(px % HW);
        const int y = r / p.W, x = r % p.W;
        f32x4 acc = {0, 0, 0, 0};
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int ny = y + D - D * (tap / 3), nx = x + D - D * (tap % 3);
            const int sy = ny / S, sx = nx / S;
            f32x4 z = {0, 0, 0, 0};
            if (ny >= 0 && nx >= 0 && ny % S == 0 && nx % S == 0 && sy < Ho && sx < Wo)
                z = *(const f32x4*)(p.dz + (n * HWo + (int64_t)sy * Wo + sx) * p.dz_ld + c);
            const f32x4 wv = *(const f32x4*)(p.w + tap * p.C + c);
#pragma unroll
            for (int k = 0; k < 4; ++k) acc[k] = fmaf(z[k], wv[k], acc[k]);
        }
        f32x4* d = (f32x4*)(p.dx + px * p.dx_ld + c);
        if (p.beta) {
            const f32x4 old = *d;
#pragma unroll
            for (int k = 0; k < 4; ++k) acc[k] = old[k] + acc[k];
        }
        *d = acc;
    }
}
static bool dw_grad_shape_ok(const DwGradParams& p) {
    const int64_t M = (int64_t)p.N * p.H * p.W;
    return p.N >= 1 && p.H >= 1 && p.W >= 1 && M < (1ll << 31) - BW_T && (p.stride == 1 || p.stride == 2) && (p.dil == 1 || p.dil == 2) &&
           p.Ho == (p.H - 1) / p.stride + 1 && p.Wo == (p.W - 1) / p.stride + 1 && p.C >= 4 && (p.C & 3) == 0 && p.C <= p.dz_ld &&
           quad_ok(p.dz, p.dz_ld);
}
hipError_t launch_dw_dgrad(const DwGradParams& p, hipStream_t s) {
    if (!dw_grad_shape_ok(p) || !quad_ok(p.w, 4) || !quad_ok(p.dx, p.dx_ld) || p.C > p.dx_ld) return hipErrorInvalidValue;
    const int64_t total = (int64_t)p.N * p.H * p.W * (p.C / 4);
    const dim3 grid((unsigned)std::min<int64_t>((total + 255) / 256, 8192));
    dw_for_sd(p.stride, p.dil, [&](auto S, auto D) {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(dw_dgrad_kernel<decltype(S)::value, decltype(D)::value>), grid, dim3(256), 0, s, p);
    });
    return hipGetLastError();
}

// dW[c][tap] = sum over output pixels q of dZ[q][c] * X[s q + d off(tap)][c], off(tap) = (tap / 3 - 1, tap % 3 - 1), and, with SUM, a
// tenth accumulator row g[c] = sum_q dZ[q][c] (the gradient of the folded bias, which the BatchNorm chain rule needs).  grid:
// x = 64-channel group, y = range of output pixels (dw_wgrad_plan over N Ho Wo).  Thread t owns channels 4 (t & 15) .. + 3 of the
// group and the pixels p_begin + (t >> 4) + 16 k of the range, k ascending: 36 fmaf chains (and 4 sums).  The 16 pixel lanes are
// then added through LDS in a fixed binary tree (lane i += lane i + 8, + 4, + 2, + 1), and lane 0 writes the range's [rows][C]
// partial.  A second launch adds the partials in range order.
constexpr int DW_CG = 64;          // channels of a workgroup
constexpr int DW_PL = 16;          // pixel lanes
template <bool SUM, int S, int D> __global__ void __launch_bounds__(256) dw_wgrad_kernel(DwGradParams p) {
    constexpr int ROWS = SUM ? 10 : 9;
    __shared__ float red[DW_PL * ROWS * DW_CG];       // [pixel lane][tap, then the sum of dZ][channel]: 36 KB, 40 KB with SUM
    const int t = threadIdx.x, cq = (t & 15) * 4, pl = t >> 4;
    const int c = blockIdx.x * DW_CG + cq;
    const bool c_in = c < p.C;                         // C is a multiple of 4: a quad is inside or outside as a whole
    const int Ho = S == 1 ? p.H : p.Ho, Wo = S == 1 ? p.W : p.Wo;
    const int HW = p.H * p.W, HWo = Ho * Wo;
    const int64_t M = (int64_t)p.N * HWo;
    const int64_t p_begin = (int64_t)blockIdx.y * p.chunk;
    const int64_t p_end = p_begin + p.chunk < M ? p_begin + p.chunk : M;
    f32x4 acc[ROWS];
#pragma unroll
    for (int row = 0; row < ROWS; ++row) acc[row] = f32x4{0, 0, 0, 0};
    if (c_in)
        for (int64_t px = p_begin + pl; px < p_end; px += DW_PL) {
            const f32x4 z = *(const f32x4*)(p.dz + px * p.dz_ld + c);
            const int64_t n = px / HWo;
            const int r = (int)(px % HWo);
            const int y0 = S * (r / Wo) - D, x0 = S * (r % Wo) - D;      // the source of tap 0
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) {
                const int sy = y0 + D * (tap / 3), sx = x0 + D * (tap % 3);
                if ((unsigned)sy >= (unsigned)p.H || (unsigned)sx >= (unsigned)p.W) continue;      // outside the map, below 0 too
                const f32x4 xv = *(const f32x4*)(p.x + (n * HW + (int64_t)sy * p.W + sx) * p.x_ld + c);
#pragma unroll
                for (int k = 0; k < 4; ++k) acc[tap][k] = fmaf(z[k], xv[k], acc[tap][k]);
            }
            if constexpr (SUM) {
#pragma unroll
                for (int k = 0; k < 4; ++k) acc[9][k] = acc[9][k] + z[k];
            }
        }
#pragma unroll
    for (int row = 0; row < ROWS; ++row) *(f32x4*)(red + (pl * ROWS + row) * DW_CG + cq) = acc[row];
    __syncthreads();
    for (int st = DW_PL / 2; st > 0; st >>= 1) {
        if (pl < st) {
#pragma unroll
            for (int row = 0; row < ROWS; ++row) {
                f32x4* a = (f32x4*)(red + (pl * ROWS + row) * DW_CG + cq);
                const f32x4 b = *(const f32x4*)(red + ((pl + st) * ROWS + row) * DW_CG + cq);
                f32x4 v = *a;
#pragma unroll
                for (int k = 0; k < 4; ++k) v[k] = v[k] + b[k];
                *a = v;
            }
        }
        __syncthreads();
    }
    if (pl == 0 && c_in) {
        float* part = p.partial + (size_t)blockIdx.y * ROWS * p.C;
#pragma unroll
        for (int row = 0; row < ROWS; ++row) *(f32x4*)(part + row * p.C + c) = *(const f32x4*)(red + row * DW_CG + cq);
    }
}

// pixel ranges of at least 64 pixels, as many as bring the grid to about four workgroups per CU (as wgrad_plan)
void dw_wgrad_plan(int64_t M, int C, int* splits, int* chunk) {
    const int64_t groups = (C + DW_CG - 1) / DW_CG;
    int64_t sp = (1024 + groups - 1) / groups;
    const int64_t max_sp = (M + 63) / 64;
    if (sp > max_sp) sp = max_sp;
    if (sp < 1) sp = 1;
    const int64_t ch = ((M + sp - 1) / sp + DW_PL - 1) / DW_PL * DW_PL;
    *chunk = (int)ch;
    *splits = (int)((M + ch - 1) / ch);
}

hipError_t launch_dw_wgrad(const DwGradParams& p, bool sum_dz, hipStream_t s) {
    const int64_t M = (int64_t)p.N * p.Ho * p.Wo;
    if (!dw_grad_shape_ok(p) || !quad_ok(p.x, p.x_ld) || p.C > p.x_ld || !quad_ok(p.partial, 4) || p.splits < 1 || p.splits > 65535 ||
        p.chunk < DW_PL || (p.chunk % DW_PL) || (int64_t)p.splits * p.chunk < M ||
        (!sum_dz && (p.stride != 1 || p.dil != 1)))      // nine rows: the cpm's form only, the one network layer kind without BatchNorm
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)((p.C + DW_CG - 1) / DW_CG), (unsigned)p.splits);
    if (!sum_dz) hipLaunchKernelGGL(HIP_KERNEL_NAME(dw_wgrad_kernel<false, 1, 1>), grid, dim3(256), 0, s, p);
    else
        dw_for_sd(p.stride, p.dil, [&](auto S, auto D) {
            hipLaunchKernelGGL(HIP_KERNEL_NAME(dw_wgrad_kernel<true, decltype(S)::value, decltype(D)::value>), grid, dim3(256), 0, s, p);
        });
    return hipGetLastError();
}

// partials in range order -> dw as OIHW (C, 1, 3, 3) and, where g is given, their tenth row -> g (C); thread i = row * C + c:
// neighbouring lanes read neighbouring partials
__global__ void __launch_bounds__(256) dw_wgrad_reduce_kernel(DwGradParams p, float* dw, float* g, int accumulate) {
    const int rows = g ? 10 : 9;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= rows * p.C) return;
    const int row = i / p.C, c = i % p.C;
    float sum = 0.0f;
    for (int z = 0; z < p.splits; ++z) sum += p.partial[(size_t)z * rows * p.C + i];
    float* d = row < 9 ? dw + c * 9 + row : g + c;
    *d = accumulate ? *d + sum : sum;
}
hipError_t launch_dw_wgrad_reduce(const DwGradParams& p, float* dw, float* g, int accumulate, hipStream_t s) {
    if (p.C < 1 || p.splits < 1 || !p.partial || !dw) return hipErrorInvalidValue;
    hipLaunchKernelGGL(dw_wgrad_reduce_kernel, dim3((unsigned)(((g ? 10 : 9) * p.C + 255) / 256)), dim3(256), 0, s, p, dw, g, accumulate);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------- backbone: the stem's weight gradient
// (with_mobilenet.py:93: conv 3 -> 32, 3x3, stride 2, pad 1, on the N x 3 x H x W input the stem kernel reads.)
// G[o][k] = sum over output pixels q = (n, y, x) of dZ[q][o] * X[n, ci, 2 y + ky - 1, 2 x + kx - 1], k = ci * 9 + ky * 3 + kx (OIHW), and
// g[o] = sum_q dZ[q][o].  A workgroup owns one range of output pixels; thread t owns output channel t & 31 and the rows
// k = (t >> 5) + 8 j, j = 0..3, of the 28-row table (row 27 is the bias sum: its X is 1), one chain per row in pixel order.  The
// 32 lanes of a k group read one X value (a broadcast) and 32 consecutive floats of dZ.  [28][32] partials per range, added in
// range order by the reduce kernel.  No dgrad: there is no gradient at the image.
constexpr int ST_ROWS = 28;
__global__ void __launch_bounds__(256) stem_wgrad_kernel(StemWgradParams p) {
    const int t = threadIdx.x, o = t & 31, kg = t >> 5;
    const int HWo = p.Ho * p.Wo;
    const int64_t plane = (int64_t)p.H * p.W;
    const int64_t M = (int64_t)p.N * HWo;
    const int64_t p_begin = (int64_t)blockIdx.x * p.chunk;
    const int64_t p_end = p_begin + p.chunk < M ? p_begin + p.chunk : M;
    int ci[4], dy[4], dx[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int k = kg + 8 * j;
        ci[j] = k / 9; dy[j] = (k % 9) / 3 - 1; dx[j] = k % 3 - 1;
    }
    float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int64_t px = p_begin; px < p_end; ++px) {
        const float z = p.dz[px * p.dz_ld + o];
        const int64_t n = px / HWo;
        const int r = (int)(px % HWo);
        const int y = r / p.Wo, x = r % p.Wo;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int k = kg + 8 * j;
            if (k > 27) continue;
            float xv = 1.0f;
            if (k < 27) {
                const int sy = 2 * y + dy[j], sx = 2 * x + dx[j];
                xv = (sy >= 0 && sy < p.H && sx >= 0 && sx < p.W) ? p.x[(n * 3 + ci[j]) * plane + (int64_t)sy * p.W + sx] : 0.0f;
            }
            acc[j] = fmaf(z, xv, acc[j]);
        }
    }
    float* part = p.partial + (size_t)blockIdx.x * ST_ROWS * 32;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int k = kg + 8 * j;
        if (k < ST_ROWS) part[k * 32 + o] = acc[j];
    }
}
// pixel ranges of at least 64 pixels, at most 1024 of them
void stem_wgrad_plan(int64_t M, int* splits, int* chunk) {
    int64_t sp = std::min<int64_t>(1024, (M + 63) / 64);
    if (sp < 1) sp = 1;
    const int64_t ch = (M + sp - 1) / sp;
    *chunk = (int)ch;
    *splits = (int)((M + ch - 1) / ch);
}
hipError_t launch_stem_wgrad(const StemWgradParams& p, hipStream_t s) {
    const int64_t M = (int64_t)p.N * p.Ho * p.Wo;
    if (p.N < 1 || p.H < 1 || p.W < 1 || p.Ho != (p.H - 1) / 2 + 1 || p.Wo != (p.W - 1) / 2 + 1 || (int64_t)p.N * 3 * p.H * p.W >= (1ll << 31) ||
        !p.dz || !p.x || !p.partial || p.dz_ld < 32 || p.splits < 1 || p.splits > 65535 || p.chunk < 1 || (int64_t)p.splits * p.chunk < M)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(stem_wgrad_kernel, dim3((unsigned)p.splits), dim3(256), 0, s, p);
    return hipGetLastError();
}
__global__ void __launch_bounds__(256) stem_wgrad_reduce_kernel(StemWgradParams p, float* G, float* g) {
    const int i = blockIdx.x * 256 + threadIdx.x;      // i = k * 32 + o
    if (i >= ST_ROWS * 32) return;
    const int k = i / 32, o = i % 32;
    float sum = 0.0f;
    for (int z = 0; z < p.splits; ++z) sum += p.partial[(size_t)z * ST_ROWS * 32 + i];
    if (k < 27) G[o * 27 + k] = sum;
    else g[o] = sum;
}
hipError_t launch_stem_wgrad_reduce(const StemWgradParams& p, float* G, float* g, hipStream_t s) {
    if (p.splits < 1 || !p.partial || !G || !g) return hipErrorInvalidValue;
    hipLaunchKernelGGL(stem_wgrad_reduce_kernel, dim3((ST_ROWS * 32 + 255) / 256), dim3(256), 0, s, p, G, g);
    return hipGetLastError();
}

// the folded pointwise weights of a fused backbone block as a plain [cout][cin] matrix, the B operand of its 1x1 dgrad (the blob
// holds them in fragment order only): float(double(w) * gamma / sqrt(double(var) + 1e-5)), the very value pack_weights stores
__global__ void __launch_bounds__(256) pw_fold_kernel(const float* w, const float* gamma, const float* var, float* out, int cout, int cin) {
    const int64_t total = (int64_t)cout * cin;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int o = (int)(i / cin);
        const double scale = (double)gamma[o] / sqrt((double)var[o] + 1e-5);
        out[i] = (float)((double)w[i] * scale);
    }
}
hipError_t launch_pw_fold(const float* w, const float* gamma, const float* var, float* out, int cout, int cin, hipStream_t s) {
    if (!w || !gamma || !var || !out || cout < 1 || cin < 1) return hipErrorInvalidValue;
    const int64_t total = (int64_t)cout * cin;
    hipLaunchKernelGGL(pw_fold_kernel, dim3((unsigned)std::min<int64_t>((total + 255) / 256, 4096)), dim3(256), 0, s, w, gamma, var, out, cout, cin);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------- BatchNorm at running statistics
// z = s (W * x + b - mu) + beta, s = gamma / sqrt(var + 1e-5) (modules/conv.py:8 in eval()).  From G = dL/d(sW), g = dL/d(folded bias):
//   dW = s G, db = s g, dbeta = g, dgamma = (<W, G> + g (b - mu)) / sqrt(var + 1e-5).  One workgroup per output channel, float64.
// A conv without bias (the backbone's) passes a row of zeros as b and no db.
__global__ void __launch_bounds__(256) bn_chain_kernel(BnChainParams p) {
    __shared__ double red[256];
    const int o = blockIdx.x, t = threadIdx.x;
    const double inv = 1.0 / sqrt((double)p.var[o] + 1e-5);
    const double sc = (double)p.gamma[o] * inv;
    const float* G = p.G + (size_t)o * p.K;
    const float* W = p.W + (size_t)o * p.K;
    float* dW = p.dW + (size_t)o * p.K;
    double dot = 0.0;
    for (int k = t; k < p.K; k += 256) {
        dot += (double)W[k] * (double)G[k];
        const float v = (float)(sc * (double)G[k]);
        dW[k] = p.accumulate ? dW[k] + v : v;
    }
    red[t] = dot;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if (t < st) red[t] += red[t + st];
        __syncthreads();
    }
    if (t == 0) {
        const double g = (double)p.g[o];
        const float vb = (float)(sc * g), vbeta = (float)g;
        const float vg = (float)((red[0] + g * ((double)p.b[o] - (double)p.mean[o])) * inv);
        if (p.db) p.db[o] = p.accumulate ? p.db[o] + vb : vb;     // (a conv without bias has no db)
        p.dbeta[o] = p.accumulate ? p.dbeta[o] + vbeta : vbeta;
        p.dgamma[o] = p.accumulate ? p.dgamma[o] + vg : vg;
    }
}

hipError_t launch_bn_chain(const BnChainParams& p, hipStream_t s) {
    if (p.cout < 1 || p.K < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(bn_chain_kernel, dim3((unsigned)p.cout), dim3(256), 0, s, p);
    return hipGetLastError();
}

}  // namespace lwp
