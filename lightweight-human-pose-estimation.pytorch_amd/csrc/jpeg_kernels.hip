// JPEG decode, device half: from the coefficient blocks the host's entropy decode left (jpeg_host.h) to interleaved BGR, for a
// whole batch of images of mixed sizes and samplings in two launches.  Everything is the integer arithmetic of libjpeg's default
// decode path, restated: jidctint.c's jpeg_idct_islow (stage A), jdsample.c's fancy h2v1 / h2v2 up-sampling and jdcolor.c's
// table-driven YCbCr conversion (stage B).  No floating point anywhere; built with -ffp-contract=off like the other exact files
// and with -fwrapv: 32-bit sums that overflow (possible only for coefficients no 8-bit picture produces) wrap as libjpeg's do on
// the machines it runs on, instead of being undefined.
//
// Workgroups are mapped to images by prefix sums with an upper-bound search: stage A over the planes' first blocks, stage B
// over the images' first pixel groups, so an image boundary may fall anywhere inside a workgroup and no launch is per image.
#include "lwp_internal.h"

namespace lwp {

// the last index i of the n + 1 ascending starts with start[i] <= v (v below start[n])
__device__ inline int jpeg_owner(const unsigned* __restrict__ start, int n, unsigned v) {
    int lo = 0, hi = n;                               // start[lo] <= v < start[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (start[mid] <= v) lo = mid; else hi = mid;
    }
    return lo;
}

// jidctint.c: one 8-point pass in the even part / odd part form, CONST_BITS = 13.  The caller descales: the column pass by
// CONST_BITS - PASS1_BITS = 11, the row pass by CONST_BITS + PASS1_BITS + 3 = 18, both round-half-up with an arithmetic shift.
// The pass order is part of the result: the rounding between the passes is.  libjpeg's shortcuts for all-zero AC terms give the
// same integers as this butterfly.  Coefficient times quantiser is at most 2^15 * 2^8 and stays in int32.
template <int SHIFT>
__device__ inline void jpeg_idct8(const int (&in)[8], int (&out)[8]) {
    int z1 = (in[2] + in[6]) * 4433;                  // FIX(0.541196100)
    const int e2 = z1 + in[6] * -15137;               // FIX(1.847759065)
    const int e3 = z1 + in[2] * 6270;                 // FIX(0.765366865)
    const int e0 = (in[0] + in[4]) * 8192, e1 = (in[0] - in[4]) * 8192;
    const int t10 = e0 + e3, t13 = e0 - e3, t11 = e1 + e2, t12 = e1 - e2;
    int t0 = in[7], t1 = in[5], t2 = in[3], t3 = in[1];
    z1 = t0 + t3;
    int z2 = t1 + t2, z3 = t0 + t2, z4 = t1 + t3;
    const int z5 = (z3 + z4) * 9633;                  // FIX(1.175875602)
    t0 *= 2446;                                       // FIX(0.298631336)
    t1 *= 16819;                                      // FIX(2.053119869)
    t2 *= 25172;                                      // FIX(3.072711026)
    t3 *= 12299;                                      // FIX(1.501321110)
    z1 *= -7373;                                      // FIX(0.899976223)
    z2 *= -20995;                                     // FIX(2.562915447)
    z3 = z3 * -16069 + z5;                            // FIX(1.961570560)
    z4 = z4 * -3196 + z5;                             // FIX(0.390180644)
    t0 += z1 + z3; t1 += z2 + z4; t2 += z2 + z3; t3 += z1 + z4;
    constexpr int half = 1 << (SHIFT - 1);
    out[0] = (t10 + t3 + half) >> SHIFT; out[7] = (t10 - t3 + half) >> SHIFT;
    out[1] = (t11 + t2 + half) >> SHIFT; out[6] = (t11 - t2 + half) >> SHIFT;
    out[2] = (t12 + t1 + half) >> SHIFT; out[5] = (t12 - t1 + half) >> SHIFT;
    out[3] = (t13 + t0 + half) >> SHIFT; out[4] = (t13 - t0 + half) >> SHIFT;
}

__device__ inline int jpeg_clamp255(int v) { return min(max(v, 0), 255); }

// Stage A.  Eight lanes own a block: lane r loads coefficient row r as one 16-byte load (with contiguous blocks a wave reads
// 1 KiB an instruction), dequantises it and parks it in a padded LDS tile; lane c then takes column c through the column pass
// and writes it back; lane r takes row r through the row pass, adds 128, clamps and stores its 8 samples as one 8-byte store.
__global__ void __launch_bounds__(kJpegBlocksPerGroup * 8) jpeg_idct_kernel(JpegLaunch j) {
    __shared__ int tile[kJpegBlocksPerGroup][8][9];
    const int slot = threadIdx.x >> 3, r = threadIdx.x & 7;
    const unsigned g = blockIdx.x * kJpegBlocksPerGroup + slot;
    const bool live = g < j.total_blocks;
    int p = 0;
    if (live) {
        p = jpeg_owner(j.plane_block0, j.n_planes, g);
        const JpegPlane pl = j.planes[p];
        const int4 raw = *reinterpret_cast<const int4*>(j.coef + (size_t)g * 64 + r * 8);
        const uint4 qraw = *reinterpret_cast<const uint4*>(j.qtables + pl.qt + r * 8);
        const int cw[4] = {raw.x, raw.y, raw.z, raw.w};
        const unsigned qw[4] = {qraw.x, qraw.y, qraw.z, qraw.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            tile[slot][r][2 * i] = (int)(short)(cw[i] & 0xffff) * (int)(qw[i] & 0xffff);
            tile[slot][r][2 * i + 1] = (cw[i] >> 16) * (int)(qw[i] >> 16);
        }
    }
    __syncthreads();
    int in[8], out[8];
    if (live) {
#pragma unroll
        for (int i = 0; i < 8; ++i) in[i] = tile[slot][i][r];
        jpeg_idct8<11>(in, out);
    }
    __syncthreads();
    if (live) {
#pragma unroll
        for (int i = 0; i < 8; ++i) tile[slot][i][r] = out[i];
    }
    __syncthreads();
    if (!live) return;
#pragma unroll
    for (int i = 0; i < 8; ++i) in[i] = tile[slot][r][i];
    jpeg_idct8<18>(in, out);
    const JpegPlane pl = j.planes[p];
    const unsigned b = g - pl.block0;
    const int by = (int)(b / (unsigned)pl.blocks_w), bx = (int)(b % (unsigned)pl.blocks_w);
    unsigned lo = 0, hi = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        lo |= (unsigned)jpeg_clamp255(out[i] + 128) << (8 * i);
        hi |= (unsigned)jpeg_clamp255(out[4 + i] + 128) << (8 * i);
    }
    unsigned char* dst = j.workspace + pl.plane + ((size_t)by * 8 + r) * ((size_t)pl.blocks_w * 8) + (size_t)bx * 8;
    *reinterpret_cast<uint2*>(dst) = make_uint2(lo, hi);
}

// jdsample.c, fancy up-sampling of one chroma plane at output pixel (x, y); the plane's edges are at its TRUE size (cw x ch),
// not at the block padding, and the edge row / column is replicated (which turns the interior formulas into libjpeg's
// special cases for the first and the last column)
__device__ inline int jpeg_chroma(const unsigned char* __restrict__ pl, int stride, int cw, int ch, int mode, int x, int y) {
    if (mode == 1) return pl[(size_t)y * stride + x];
    const int i = x >> 1, side = x & 1 ? min(i + 1, cw - 1) : max(i - 1, 0);
    if (mode == 2) {                                   // h2v1: (3 near + far + 1) >> 2 on even columns, + 2 on odd ones
        const unsigned char* row = pl + (size_t)y * stride;
        return (3 * row[i] + row[side] + (x & 1 ? 2 : 1)) >> 2;
    }
    // h2v2: vertically 3 near + far, unrounded (far: the row above for even output rows, below for odd ones), then
    // (3 near + far + 8) >> 4 on even columns, + 7 on odd ones
    const int jn = y >> 1, jf = y & 1 ? min(jn + 1, ch - 1) : max(jn - 1, 0);
    const unsigned char* near = pl + (size_t)jn * stride;
    const unsigned char* far = pl + (size_t)jf * stride;
    const int s_here = 3 * near[i] + far[i], s_side = 3 * near[side] + far[side];
    return (3 * s_here + s_side + (x & 1 ? 7 : 8)) >> 4;
}

// Stage B.  One thread per kJpegPixelsPerThread adjacent pixels of one output row: up-sample, jdcolor.c's conversion (the
// tables' entries as formulas; cb, cr minus 128, arithmetic shifts), interleaved BGR store.
__global__ void __launch_bounds__(kJpegUnitsPerGroup) jpeg_color_kernel(JpegLaunch j) {
    const unsigned u = blockIdx.x * kJpegUnitsPerGroup + threadIdx.x;
    if (u >= j.total_units) return;
    const JpegImage im = j.images[jpeg_owner(j.image_unit0, j.n_images, u)];
    const unsigned local = u - im.unit0, per_row = (unsigned)(im.width + kJpegPixelsPerThread - 1) / kJpegPixelsPerThread;
    const int y = (int)(local / per_row), x0 = (int)(local % per_row) * kJpegPixelsPerThread;
    const int n = min(kJpegPixelsPerThread, im.width - x0);
    const unsigned char* yp = j.workspace + im.plane[0] + (size_t)y * im.stride[0] + x0;
    unsigned char px[kJpegPixelsPerThread * 3];
#pragma unroll
    for (int k = 0; k < kJpegPixelsPerThread; ++k) {
        if (k >= n) { px[3 * k] = px[3 * k + 1] = px[3 * k + 2] = 0; continue; }
        const int Y = yp[k];
        int B = Y, G = Y, R = Y;
        if (im.mode != 0) {
            const int cb = jpeg_chroma(j.workspace + im.plane[1], im.stride[1], im.chroma_w, im.chroma_h, im.mode, x0 + k, y) - 128;
            const int cr = jpeg_chroma(j.workspace + im.plane[2], im.stride[2], im.chroma_w, im.chroma_h, im.mode, x0 + k, y) - 128;
            R = jpeg_clamp255(Y + ((91881 * cr + 32768) >> 16));
            B = jpeg_clamp255(Y + ((116130 * cb + 32768) >> 16));
            G = jpeg_clamp255(Y + ((-22554 * cb - 46802 * cr + 32768) >> 16));
        }
        px[3 * k] = (unsigned char)B; px[3 * k + 1] = (unsigned char)G; px[3 * k + 2] = (unsigned char)R;
    }
    unsigned char* o = im.out + ((size_t)y * im.width + x0) * 3;
    if (n == kJpegPixelsPerThread && ((size_t)o & 3) == 0) {      // 12 bytes as three dwords where the row lets them be aligned
        unsigned* o4 = reinterpret_cast<unsigned*>(o);
#pragma unroll
        for (int w = 0; w < 3; ++w)
            o4[w] = (unsigned)px[4 * w] | ((unsigned)px[4 * w + 1] << 8) | ((unsigned)px[4 * w + 2] << 16) | ((unsigned)px[4 * w + 3] << 24);
    } else {
#pragma unroll
        for (int b = 0; b < 3 * kJpegPixelsPerThread; ++b)
            if (b < 3 * n) o[b] = px[b];
    }
}

hipError_t launch_jpeg_idct(const JpegLaunch& j, hipStream_t s) {
    if (j.total_blocks == 0) return hipSuccess;
    hipLaunchKernelGGL(jpeg_idct_kernel, dim3((j.total_blocks + kJpegBlocksPerGroup - 1) / kJpegBlocksPerGroup), dim3(kJpegBlocksPerGroup * 8), 0, s, j);
    return hipGetLastError();
}

hipError_t launch_jpeg_color(const JpegLaunch& j, hipStream_t s) {
    if (j.total_units == 0) return hipSuccess;
    hipLaunchKernelGGL(jpeg_color_kernel, dim3((j.total_units + kJpegUnitsPerGroup - 1) / kJpegUnitsPerGroup), dim3(kJpegUnitsPerGroup), 0, s, j);
    return hipGetLastError();
}

}  // namespace lwp
