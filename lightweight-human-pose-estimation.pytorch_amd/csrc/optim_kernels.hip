// Stage fine-tuning step on the device: Adam over the flat stage-gradient array (train.py:41-55, :106) and the refold / repack of
// the changed stage layers into the forward's weight blob (pack_weights, net_graph.cpp, for fp32 L_GEMM layers).
// Both kernels restate double arithmetic statement by statement (torch's single-tensor Adam; pack_weights' host loops): this
// translation unit is built with -ffp-contract=off (build.py), and the pragma below says the same to the front end.  No
// floating-point atomics: every destination element has exactly one writer.
#include <cmath>

#include "lwp_internal.h"

#pragma clang fp contract(off)

namespace lwp {

// ------------------------------------------------------------------------------------------------ Adam
// One element, float64 throughout, one rounding at each of the three stores (the caller stores the returned values).
__device__ inline void adam_element(const AdamParams& p, double step_size, bool decay, float g32, float& p32, float& m32, float& v32) {
    double g = (double)g32;
    const double w = (double)p32;
    double m = (double)m32, v = (double)v32;
    if (decay) g = g + p.weight_decay * w;
    m = m + (g - m) * p.one_minus_b1;
    v = p.b2 * v + p.one_minus_b2 * g * g;
    const double denom = sqrt(v) / p.sqrt_bc2 + p.eps;
    p32 = (float)(w - step_size * m / denom);
    m32 = (float)m;
    v32 = (float)v;
}

// One workgroup per chunk of at most kAdamChunk elements of ONE parameter (one learning rate, one weight-decay flag).  A chunk
// whose gradient and raw offsets are multiples of four floats moves 16 bytes per access; the head of a parameter that starts
// off that grid is a chunk of its own (at most three elements) and takes the scalar path.
__global__ void __launch_bounds__(256) stage_adam_kernel(AdamParams p) {
    const AdamChunk c = p.chunks[blockIdx.x];
    const double step_size = p.step_size[c.group & 3];
    const bool decay = (c.group & 4) != 0;
    const float* g = p.grads + c.goff;
    float* w = p.raw + c.roff;
    float* m = p.exp_avg + c.goff;
    float* v = p.exp_avg_sq + c.goff;
    const unsigned n = c.n;
    if (p.vec_ok && ((c.goff | c.roff) & 3u) == 0) {
        const unsigned i = threadIdx.x * 4;
        if (i + 3 < n) {
            const float4 g4 = *(const float4*)(g + i);
            float4 w4 = *(const float4*)(w + i), m4 = *(const float4*)(m + i), v4 = *(const float4*)(v + i);
            adam_element(p, step_size, decay, g4.x, w4.x, m4.x, v4.x);
            adam_element(p, step_size, decay, g4.y, w4.y, m4.y, v4.y);
            adam_element(p, step_size, decay, g4.z, w4.z, m4.z, v4.z);
            adam_element(p, step_size, decay, g4.w, w4.w, m4.w, v4.w);
            *(float4*)(w + i) = w4; *(float4*)(m + i) = m4; *(float4*)(v + i) = v4;
        } else {
            for (unsigned k = i; k < n; ++k) adam_element(p, step_size, decay, g[k], w[k], m[k], v[k]);
        }
        return;
    }
    for (unsigned k = threadIdx.x; k < n; k += 256) adam_element(p, step_size, decay, g[k], w[k], m[k], v[k]);
}

hipError_t launch_stage_adam(const AdamParams& p, hipStream_t s) {
    if (p.n_chunks <= 0) return hipSuccess;
    static_assert(kAdamChunk == 256 * 4, "one float4 per thread covers a chunk");
    hipLaunchKernelGGL(stage_adam_kernel, dim3(p.n_chunks), dim3(256), 0, s, p);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ repack
// raw value of the padded [cout_pad][cin_pad] matrix of tap t, folded: 0 outside the layer's (or its source convs') extent
__device__ inline float repack_value(const RepackLayer& l, const float* __restrict__ raw, int o, int ci, int t, double scale) {
    if (l.n_blocks == 0) {
        if (o >= l.cout || ci >= l.cin) return 0.f;
        return (float)((double)raw[l.w_raw + ((size_t)o * l.cin + ci) * l.taps + t] * scale);
    }
    for (int b = 0; b < l.n_blocks; ++b) {
        const RepackBlock& k = l.blk[b];
        if (o >= k.out_off && o < k.out_off + k.cout && ci >= k.in_off && ci < k.in_off + k.cin)
            return raw[k.w_raw + (size_t)(o - k.out_off) * k.cin + (ci - k.in_off)];
    }
    return 0.f;
}

// One thread per 16 bytes of a layer's fragment-order copy: (tap, k-step, 32-channel tile, s, lane) holds
// W[tile * 32 + (lane & 31)][step * 32 + 8 s + 4 (lane >> 5) + j], j = 0..3, which is also four consecutive floats of the
// [tap][cout_pad][cin_pad] copy, so the thread writes both.  The threads with (tap, step, s, lane >> 5) = 0 cover every output
// channel of the padded bias row once and write it too.  Workgroups map to layers through the table's block prefix.
__global__ void __launch_bounds__(256) stage_repack_kernel(const RepackLayer* __restrict__ tab, int n_layers, const float* __restrict__ raw,
                                                           float* __restrict__ blob) {
    int li = 0;
    while (li + 1 < n_layers && blockIdx.x >= tab[li + 1].block_begin) ++li;
    const RepackLayer& l = tab[li];
    const unsigned item = (blockIdx.x - l.block_begin) * 256 + threadIdx.x;
    const int ksteps = l.cin_pad / 32, ntiles = l.cout_pad / 32;
    if (item >= (unsigned)l.taps * ksteps * ntiles * 256) return;
    const int ln = item & 63, sq = (item >> 6) & 3;
    unsigned r = item >> 8;
    const int nt = r % ntiles; r /= ntiles;
    const int ks = r % ksteps;
    const int t = r / ksteps;
    const int o = nt * 32 + (ln & 31), ci0 = ks * 32 + 8 * sq + 4 * (ln >> 5);
    double scale = 1.0;
    const bool bn = l.gamma_raw >= 0 && o < l.cout;
    if (bn) scale = (double)raw[l.gamma_raw + o] / sqrt((double)raw[l.var_raw + o] + 1e-5);
    float4 v;
    v.x = repack_value(l, raw, o, ci0 + 0, t, scale);
    v.y = repack_value(l, raw, o, ci0 + 1, t, scale);
    v.z = repack_value(l, raw, o, ci0 + 2, t, scale);
    v.w = repack_value(l, raw, o, ci0 + 3, t, scale);
    *(float4*)(blob + l.w_off + ((size_t)t * l.cout_pad + o) * l.cin_pad + ci0) = v;
    *(float4*)(blob + l.w2_off + (size_t)item * 4) = v;
    if (t == 0 && ks == 0 && sq == 0 && ln < 32) {
        float b = 0.f;
        if (l.n_blocks == 0) {
            if (o < l.cout) {
                const double cb = l.b_raw >= 0 ? (double)raw[l.b_raw + o] : 0.0;
                if (bn) b = (float)((cb - (double)raw[l.mean_raw + o]) * scale + (double)raw[l.beta_raw + o]);
                else b = (float)cb;
            }
        } else {
            for (int k = 0; k < l.n_blocks; ++k)
                if (o >= l.blk[k].out_off && o < l.blk[k].out_off + l.blk[k].cout) b = raw[l.blk[k].b_raw + (o - l.blk[k].out_off)];
        }
        blob[l.b_off + o] = b;
    }
}

hipError_t launch_stage_repack(const RepackLayer* tab_device, int n_layers, int n_blocks, const float* raw, float* blob, hipStream_t s) {
    if (n_layers <= 0 || n_blocks <= 0) return hipSuccess;
    hipLaunchKernelGGL(stage_repack_kernel, dim3(n_blocks), dim3(256), 0, s, tab_device, n_layers, raw, blob);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ repack, depthwise and fused layers
// An L_DW / L_DWPW layer as pack_weights writes it.  Without BatchNorm (the cpm trunk): the depthwise (C, 1, 3, 3) as [tap][C] with a zero bias
// row, the pointwise (cout, C, 1, 1) in the f32 MFMA fragment order [C/32][cout/32][4][64 lanes][4] (lane (q = lane >> 4,
// c = lane & 15) holds value v = 8 u + 2 j + t = W[n = 32 w + 16 t + c][k = 32 s + 16 u + 4 q + j]) with a zero bias row.  The
// fold scale of a layer without BatchNorm is exactly 1.0, so pack_weights' float(double(w) * 1.0) is w itself: every element is
// a plain copy of its raw value.  With BatchNorm (the backbone, LWP_TRAIN_ALL; a half whose gamma offset is >= 0): the fold of
// pack_weights, scale = gamma / sqrt(double(var) + 1e-5) in double, float(double(w) * scale), and the bias row
// float((0 - mu) * scale + beta) (these convs have no bias of their own).  One thread per destination float.
__global__ void __launch_bounds__(256) dw_repack_kernel(DwRepack l, const float* __restrict__ raw, float* __restrict__ blob) {
    const unsigned i = blockIdx.x * 256 + threadIdx.x;
    const unsigned n_dw = 9u * l.C, n_pw = (unsigned)l.C * l.cout;
    if (i < n_dw) {
        const unsigned t = i / l.C, c = i % l.C;
        if (l.dw_gamma < 0) {
            blob[l.w_off + i] = raw[l.dw_raw + c * 9 + t];
            if (t == 0) blob[l.b_off + c] = 0.f;
            return;
        }
        const double scale = (double)raw[l.dw_gamma + c] / sqrt((double)raw[l.dw_var + c] + 1e-5);
        blob[l.w_off + i] = (float)((double)raw[l.dw_raw + c * 9 + t] * scale);
        if (t == 0) blob[l.b_off + c] = (float)((0.0 - (double)raw[l.dw_mean + c]) * scale + (double)raw[l.dw_beta + c]);
        return;
    }
    const unsigned e = i - n_dw;
    if (e >= n_pw) return;
    const unsigned nw = l.cout / 32;
    const unsigned v = ((e >> 8) & 3) * 4 + (e & 3), lane = (e >> 2) & 63;
    const unsigned sw = e >> 10, s = sw / nw, wv = sw % nw;
    const unsigned u = v >> 3, j = (v >> 1) & 3, t = v & 1, q = lane >> 4, c = lane & 15;
    const unsigned k = 32 * s + 16 * u + 4 * q + j, n = 32 * wv + 16 * t + c;
    if (l.pw_gamma < 0) {
        blob[l.w2_off + e] = raw[l.pw_raw + (size_t)n * l.C + k];
        if (e < (unsigned)l.cout) blob[l.b2_off + e] = 0.f;
        return;
    }
    const double scale = (double)raw[l.pw_gamma + n] / sqrt((double)raw[l.pw_var + n] + 1e-5);
    blob[l.w2_off + e] = (float)((double)raw[l.pw_raw + (size_t)n * l.C + k] * scale);
    if (e < (unsigned)l.cout) {
        const double sc = (double)raw[l.pw_gamma + e] / sqrt((double)raw[l.pw_var + e] + 1e-5);
        blob[l.b2_off + e] = (float)((0.0 - (double)raw[l.pw_mean + e]) * sc + (double)raw[l.pw_beta + e]);
    }
}

hipError_t launch_dw_repack(const DwRepack& l, const float* raw, float* blob, hipStream_t s) {
    if (l.C < 1 || l.dw_raw < 0 || (l.cout > 0 && (l.pw_raw < 0 || l.C % 32 || l.cout % 32))) return hipErrorInvalidValue;
    const unsigned total = 9u * l.C + (unsigned)l.C * l.cout;
    hipLaunchKernelGGL(dw_repack_kernel, dim3((total + 255) / 256), dim3(256), 0, s, l, raw, blob);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ repack, stem
// model.0 (LWP_TRAIN_ALL): OIHW (32, 3, 3, 3) -> [(ky, kx, ci)][oc] with BatchNorm folded as above, and the bias row
__global__ void __launch_bounds__(256) stem_repack_kernel(StemRepack l, const float* __restrict__ raw, float* __restrict__ blob) {
    const unsigned i = blockIdx.x * 256 + threadIdx.x;     // i = (t * 3 + ci) * 32 + o
    if (i >= 27u * 32u + 32u) return;
    const unsigned o = i & 31u;
    const double scale = (double)raw[l.gamma + o] / sqrt((double)raw[l.var + o] + 1e-5);
    if (i >= 27u * 32u) {
        blob[l.b_off + o] = (float)((0.0 - (double)raw[l.mean + o]) * scale + (double)raw[l.beta + o]);
        return;
    }
    const unsigned tc = i >> 5, t = tc / 3, ci = tc % 3;
    blob[l.w_off + i] = (float)((double)raw[l.w_raw + (o * 3 + ci) * 9 + t] * scale);
}

hipError_t launch_stem_repack(const StemRepack& l, const float* raw, float* blob, hipStream_t s) {
    if (l.w_raw < 0 || l.gamma < 0 || l.beta < 0 || l.mean < 0 || l.var < 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(stem_repack_kernel, dim3((27 * 32 + 32 + 255) / 256), dim3(256), 0, s, l, raw, blob);
    return hipGetLastError();
}

}  // namespace lwp
