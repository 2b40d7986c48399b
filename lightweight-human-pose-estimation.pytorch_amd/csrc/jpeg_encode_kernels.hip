// JPEG encode, device half: from BGR frames to the stuffed entropy-coded scan of each, for a whole batch of frames of mixed
// sizes and samplings (lwp_internal.h lists the six stages).  Everything is the integer arithmetic of libjpeg's default
// compression path, restated: jccolor.c's 16-bit fixed-point conversion, jcsample.c's h2v1 / h2v2 box filters with their
// alternating bias, jcsample.c's / jcprepct.c's edge rules, jccoefct.c's dummy blocks, jfdctint.c's jpeg_fdct_islow, jcdctmgr.c's
// rounding quantiser and jchuff.c's coding with Annex K's tables.  No floating point anywhere; plain C++ loads and stores and
// vector atomics only.  Every value written has one writer, or is OR-ed into a zeroed word whose bits have one writer each, so
// nothing depends on the order in which workgroups run, and the same frames give the same bytes.
//
// Workgroups are mapped to images by prefix sums with an upper-bound search (stages A, B, D, F), so an image boundary may fall
// anywhere inside a workgroup; stages C and E take one workgroup an image and step over it in tiles with a carry.
#include "lwp_internal.h"

namespace lwp {

// the last index i of the n + 1 ascending starts with start[i] <= v (v below start[n])
__device__ inline int jpeg_enc_owner(const unsigned* __restrict__ start, int n, unsigned v) {
    int lo = 0, hi = n;                               // start[lo] <= v < start[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (start[mid] <= v) lo = mid; else hi = mid;
    }
    return lo;
}

// element c of a three-element member of a record held in registers (a run-time index would send the record to scratch)
template <class T> __device__ inline T jpeg_enc_pick(const T (&a)[3], int c) { return c == 0 ? a[0] : c == 1 ? a[1] : a[2]; }

// jccolor.c's rgb_ycc_convert: the table entries as formulas, SCALEBITS = 16.  c: 0 Y, 1 Cb, 2 Cr
__device__ inline int jpeg_enc_sample(const unsigned char* __restrict__ px, int c) {
    const int b = px[0], g = px[1], r = px[2];
    if (c == 0) return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16;
    if (c == 1) return (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16;
    return (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16;
}

// jfdctint.c: one 8-point pass, CONST_BITS = 13, PASS1_BITS = 2.  FIRST: the row pass, which leaves PASS1_BITS of scale in
// outputs 0 and 4 and descales the others by CONST_BITS - PASS1_BITS; else the column pass, which descales by PASS1_BITS and by
// CONST_BITS + PASS1_BITS.  Every DESCALE rounds half up with an arithmetic shift.  Samples are at most 128 in magnitude: the
// products stay far inside int32.
template <bool FIRST>
__device__ inline void jpeg_fdct8(const int (&d)[8], int (&out)[8]) {
    const int t0 = d[0] + d[7], t7 = d[0] - d[7], t1 = d[1] + d[6], t6 = d[1] - d[6];
    const int t2 = d[2] + d[5], t5 = d[2] - d[5], t3 = d[3] + d[4], t4 = d[3] - d[4];
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    constexpr int n = FIRST ? 11 : 15, half = 1 << (n - 1);
    if (FIRST) {
        out[0] = (t10 + t11) << 2;
        out[4] = (t10 - t11) << 2;
    } else {
        out[0] = (t10 + t11 + 2) >> 2;
        out[4] = (t10 - t11 + 2) >> 2;
    }
    int z1 = (t12 + t13) * 4433;                      // FIX(0.541196100)
    out[2] = (z1 + t13 * 6270 + half) >> n;           // FIX(0.765366865)
    out[6] = (z1 + t12 * -15137 + half) >> n;         // FIX(1.847759065)
    z1 = t4 + t7;
    int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
    const int z5 = (z3 + z4) * 9633;                  // FIX(1.175875602)
    const int u4 = t4 * 2446;                         // FIX(0.298631336)
    const int u5 = t5 * 16819;                        // FIX(2.053119869)
    const int u6 = t6 * 25172;                        // FIX(3.072711026)
    const int u7 = t7 * 12299;                        // FIX(1.501321110)
    z1 *= -7373;                                      // FIX(0.899976223)
    z2 *= -20995;                                     // FIX(2.562915447)
    z3 = z3 * -16069 + z5;                            // FIX(1.961570560)
    z4 = z4 * -3196 + z5;                             // FIX(0.390180644)
    out[7] = (u4 + z1 + z3 + half) >> n;
    out[5] = (u5 + z2 + z4 + half) >> n;
    out[3] = (u6 + z2 + z3 + half) >> n;
    out[1] = (u7 + z1 + z4 + half) >> n;
}

// Stage A.  Eight lanes own a block of the MCU-padded grid.  A dummy block (beyond the real blocks of its component) takes the
// place of the real block whose DC jccoefct.c copies into it: the block to its left, or for a dummy block row the last block of
// the row above inside the MCU (itself replaced by ITS left neighbour where it is a dummy); its AC terms are stored as zeros.
// Lane r gathers sample row r (edges: the column index is clamped to the last pixel; the row index to the last row, for the
// down-sampled chroma of 4:2:0 to the last DOWN-SAMPLED row, whose two source rows are then clamped to the last pixel row),
// runs the row pass and parks it in a padded LDS tile; lane c takes column c through the column pass and the quantiser; the
// tile turns the result back so that lane r stores coefficient row r as one 16-byte store.
__global__ void __launch_bounds__(kJpegEncBlocksPerGroup * 8) jpeg_enc_dct_kernel(JpegEncLaunch e) {
    __shared__ int tile[kJpegEncBlocksPerGroup][8][9];
    const int slot = threadIdx.x >> 3, r = threadIdx.x & 7;
    const unsigned g = blockIdx.x * kJpegEncBlocksPerGroup + slot;
    const bool live = g < e.total_blocks;
    bool dummy = false;
    int c = 0;
    int in[8], out[8];
    if (live) {
        const JpegEncImage im = e.images[jpeg_enc_owner(e.block_start, e.n_images, g)];
        const unsigned b = g - im.block0;
        c = b >= im.plane0[2] ? 2 : b >= im.plane0[1] ? 1 : 0;
        const unsigned lb = b - jpeg_enc_pick(im.plane0, c), grid_w = (unsigned)jpeg_enc_pick(im.blocks_w, c);
        const int real_w = jpeg_enc_pick(im.real_w, c), real_h = jpeg_enc_pick(im.real_h, c);
        int by = (int)(lb / grid_w), bx = (int)(lb % grid_w);
        const int hc = c ? 1 : im.hs;
        if (by >= real_h) {
            dummy = true;
            by = real_h - 1;
            bx = min(bx / hc * hc + hc - 1, real_w - 1);
        } else if (bx >= real_w) {
            dummy = true;
            bx = real_w - 1;
        }
        const int W = im.width, H = im.height;
        const int fh = c ? im.hs : 1, fv = c ? im.vs : 1;              // full-resolution pixels a sample of this component covers
        const int rows = (H + fv - 1) / fv;                           // the component's true height
        const int y = min(by * 8 + r, rows - 1);
        const unsigned char* row0 = im.src + (size_t)min(y * fv, H - 1) * W * 3;
        const unsigned char* row1 = im.src + (size_t)min(y * fv + fv - 1, H - 1) * W * 3;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int x = bx * 8 + k;
            int v;
            if (fh == 1) {
                v = jpeg_enc_sample(row0 + (size_t)min(x, W - 1) * 3, c);
            } else {
                const size_t x0 = (size_t)min(2 * x, W - 1) * 3, x1 = (size_t)min(2 * x + 1, W - 1) * 3;
                if (fv == 1) v = (jpeg_enc_sample(row0 + x0, c) + jpeg_enc_sample(row0 + x1, c) + (k & 1)) >> 1;      // bias 0, 1, 0, 1 ..
                else v = (jpeg_enc_sample(row0 + x0, c) + jpeg_enc_sample(row0 + x1, c) + jpeg_enc_sample(row1 + x0, c) +
                          jpeg_enc_sample(row1 + x1, c) + 1 + (k & 1)) >> 2;                                            // bias 1, 2, 1, 2 ..
            }
            in[k] = v - 128;
        }
        jpeg_fdct8<true>(in, out);
#pragma unroll
        for (int k = 0; k < 8; ++k) tile[slot][r][k] = out[k];
    }
    __syncthreads();
    if (live) {
#pragma unroll
        for (int k = 0; k < 8; ++k) in[k] = tile[slot][k][r];
        jpeg_fdct8<false>(in, out);
        const uint16_t* q = e.qtables + (c ? 64 : 0);
#pragma unroll
        for (int k = 0; k < 8; ++k) {                   // jcdctmgr.c: the DCT output carries a factor of 8, so does the divisor
            const int q8 = 8 * (int)q[k * 8 + r];
            const int m = (abs(out[k]) + (q8 >> 1)) / q8;
            out[k] = dummy && (k | r) ? 0 : out[k] < 0 ? -m : m;
        }
    }
    __syncthreads();
    if (live) {
#pragma unroll
        for (int k = 0; k < 8; ++k) tile[slot][k][r] = out[k];
    }
    __syncthreads();
    if (!live) return;
    int4 w;
    w.x = (tile[slot][r][0] & 0xffff) | (tile[slot][r][1] << 16);
    w.y = (tile[slot][r][2] & 0xffff) | (tile[slot][r][3] << 16);
    w.z = (tile[slot][r][4] & 0xffff) | (tile[slot][r][5] << 16);
    w.w = (tile[slot][r][6] & 0xffff) | (tile[slot][r][7] << 16);
    *reinterpret_cast<int4*>(e.coef + (size_t)g * 64 + r * 8) = w;
}

// ---- the entropy code of one block, shared by the length pass and the write pass
struct JpegEncCount {
    unsigned total = 0;
    __device__ void put(unsigned, int len) { total += (unsigned)len; }
};
// Bits go MSB first into a 64-bit window; every full 32 bits leave as one byte-swapped word OR-ed into the zeroed scan (the first
// and the last word of a block are shared with its neighbours, whose bits are zero in this lane's word).
struct JpegEncWriter {
    unsigned* words; unsigned w, limit;
    unsigned long long acc = 0;
    int n;
    __device__ void flush() {
        if (w < limit) atomicOr(words + w, __builtin_bswap32((unsigned)(acc >> 32)));
        ++w;
    }
    __device__ void put(unsigned code, int len) {      // 1 <= len <= 16, n < 32
        acc |= (unsigned long long)code << (64 - n - len);
        n += len;
        if (n >= 32) { flush(); acc <<= 32; n -= 32; }
    }
};

struct JpegEncBlockRef { unsigned plane_index; int pred; int comp; };

// the block at stream index s of an image: its index in plane order, its component, and the DC it is predicted from (the
// component's block before it in MCU order, 0 at the start of the scan and of every restart interval)
__device__ inline JpegEncBlockRef jpeg_enc_locate(const JpegEncImage& im, unsigned s, const int16_t* __restrict__ coef) {
    const unsigned mcu = s / im.per_mcu, k = s % im.per_mcu, nl = (unsigned)(im.hs * im.vs);
    const unsigned my = mcu / (unsigned)im.mcus_x, mx = mcu % (unsigned)im.mcus_x;
    const int c = k < nl ? 0 : (int)(k - nl) + 1;
    auto at = [&](unsigned yy, unsigned xx, int cc, unsigned j) {
        return cc == 0 ? im.plane0[0] + (yy * (unsigned)im.vs + j / (unsigned)im.hs) * (unsigned)im.blocks_w[0] + xx * (unsigned)im.hs + j % (unsigned)im.hs
                       : jpeg_enc_pick(im.plane0, cc) + yy * (unsigned)jpeg_enc_pick(im.blocks_w, cc) + xx;
    };
    JpegEncBlockRef ref;
    ref.comp = c;
    ref.plane_index = at(my, mx, c, c == 0 ? k : 0);
    if (c == 0 && k > 0) {
        ref.pred = coef[(size_t)(im.block0 + at(my, mx, 0, k - 1)) * 64];
    } else if (s < im.per_mcu || (im.ri_blocks && s / im.ri_blocks * im.ri_blocks + im.per_mcu > s)) {
        ref.pred = 0;                                  // the first MCU of the scan or of a restart interval
    } else {
        const unsigned pm = mcu - 1;
        ref.pred = coef[(size_t)(im.block0 + at(pm / (unsigned)im.mcus_x, pm % (unsigned)im.mcus_x, c, c == 0 ? nl - 1 : 0)) * 64];
    }
    return ref;
}

__device__ inline int jpeg_enc_coef(const unsigned (&w)[32], int natural) {
    return (int)(short)(natural & 1 ? w[natural >> 1] >> 16 : w[natural >> 1] & 0xffff);
}

// jchuff.c's encode_one_block: the DC difference's category and bits, then run / size symbols with ZRL for runs above 15 and
// EOB when the block ends in zeros.  dc / ac: the component's code tables in LDS.  Magnitudes above 10 bits (no 8-bit picture
// has them) would pick a wrong symbol, never an address outside the table.
template <class Sink>
__device__ inline void jpeg_enc_block(const unsigned (&w)[32], int pred, const unsigned* dc, const unsigned* ac, Sink& sink) {
    constexpr unsigned char zz[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                      41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                      30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
    int v = jpeg_enc_coef(w, 0) - pred;
    int s = 32 - __clz(abs(v));
    unsigned h = dc[s & 15];
    sink.put(h >> 5, (int)(h & 31));
    if (s) sink.put((unsigned)(v < 0 ? v - 1 : v) & ((1u << s) - 1), s);
    int run = 0;
#pragma unroll
    for (int k = 1; k < 64; ++k) {
        v = jpeg_enc_coef(w, zz[k]);
        if (v == 0) { ++run; continue; }
        while (run > 15) {
            h = ac[0xF0];
            sink.put(h >> 5, (int)(h & 31));
            run -= 16;
        }
        s = 32 - __clz(abs(v));
        h = ac[((run << 4) | s) & 255];
        sink.put(h >> 5, (int)(h & 31));
        sink.put((unsigned)(v < 0 ? v - 1 : v) & ((1u << s) - 1), s);
        run = 0;
    }
    if (run) { h = ac[0]; sink.put(h >> 5, (int)(h & 31)); }
}

// the code tables of both table pairs into LDS: dc[2][16], ac[2][256]
__device__ inline void jpeg_enc_load_tables(unsigned* lds, const unsigned* __restrict__ huff) {
    for (int i = threadIdx.x; i < 2 * 16 + 2 * 256; i += kJpegEncGroup) lds[i] = huff[i];
    __syncthreads();
}

__device__ inline void jpeg_enc_load_block(const int16_t* __restrict__ coef, size_t block, unsigned (&w)[32]) {
    const uint4* p = reinterpret_cast<const uint4*>(coef + block * 64);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const uint4 q = p[i];
        w[4 * i] = q.x; w[4 * i + 1] = q.y; w[4 * i + 2] = q.z; w[4 * i + 3] = q.w;
    }
}

// Stage B.  One lane a block, in stream order over the batch.
__global__ void __launch_bounds__(kJpegEncGroup) jpeg_enc_lengths_kernel(JpegEncLaunch e) {
    __shared__ unsigned tab[2 * 16 + 2 * 256];
    jpeg_enc_load_tables(tab, e.huff);
    const unsigned g = blockIdx.x * kJpegEncGroup + threadIdx.x;
    if (g >= e.total_blocks) return;
    const JpegEncImage im = e.images[jpeg_enc_owner(e.block_start, e.n_images, g)];
    const JpegEncBlockRef ref = jpeg_enc_locate(im, g - im.block0, e.coef);
    unsigned w[32];
    jpeg_enc_load_block(e.coef, (size_t)im.block0 + ref.plane_index, w);
    const int t = ref.comp ? 1 : 0;
    JpegEncCount sink;
    jpeg_enc_block(w, ref.pred, tab + 16 * t, tab + 32 + 256 * t, sink);
    e.bits[g] = sink.total;
}

// Stage C.  The bit offset of a block is the running sum of the counts in front of it, rounded up to a byte wherever a restart
// interval starts.  An element is the function it applies to the sum in front of it, x -> x + a for a plain block and
// x -> roundup8(x + a) + b once an interval start is inside; these compose to the same form (roundup8 of a multiple of 8 plus b
// is that multiple plus roundup8(b)), so a tile of kJpegEncGroup blocks is scanned in LDS and the tiles are chained by a carry.
struct JpegEncStep { unsigned a, b, round; };
__device__ inline JpegEncStep jpeg_enc_then(const JpegEncStep f, const JpegEncStep g) {        // f first, then g
    if (!g.round) return f.round ? JpegEncStep{f.a, f.b + g.a, 1u} : JpegEncStep{f.a + g.a, 0u, 0u};
    return f.round ? JpegEncStep{f.a, ((f.b + g.a + 7u) & ~7u) + g.b, 1u} : JpegEncStep{f.a + g.a, g.b, 1u};
}
__device__ inline unsigned jpeg_enc_apply(const JpegEncStep f, unsigned x) { return f.round ? ((x + f.a + 7u) & ~7u) + f.b : x + f.a; }

__global__ void __launch_bounds__(kJpegEncGroup) jpeg_enc_offsets_kernel(JpegEncLaunch e) {
    __shared__ unsigned sa[kJpegEncGroup], sb[kJpegEncGroup], sr[kJpegEncGroup];
    __shared__ unsigned carry;
    const JpegEncImage im = e.images[blockIdx.x];
    const int t = threadIdx.x;
    if (t == 0) { carry = 0; e.istart[im.int0] = 0; }
    __syncthreads();
    for (unsigned base = 0; base < im.n_blocks; base += kJpegEncGroup) {
        const unsigned s = base + t;
        const bool in = s < im.n_blocks;
        const unsigned bits = in ? e.bits[im.block0 + s] : 0;
        const bool start = in && s && im.ri_blocks && s % im.ri_blocks == 0;
        JpegEncStep f = start ? JpegEncStep{0u, bits, 1u} : JpegEncStep{bits, 0u, 0u};
        sa[t] = f.a; sb[t] = f.b; sr[t] = f.round;
        __syncthreads();
        for (int d = 1; d < kJpegEncGroup; d <<= 1) {
            JpegEncStep p{0u, 0u, 0u};
            if (t >= d) p = JpegEncStep{sa[t - d], sb[t - d], sr[t - d]};
            __syncthreads();
            if (t >= d) { f = jpeg_enc_then(p, f); sa[t] = f.a; sb[t] = f.b; sr[t] = f.round; }
            __syncthreads();
        }
        const unsigned before = carry;
        const unsigned end = jpeg_enc_apply(f, before);            // the first bit behind this block
        if (in) {
            e.offs[im.block0 + s] = end - bits;
            if (start) e.istart[im.int0 + s / im.ri_blocks] = (end - bits) >> 3;
        }
        __syncthreads();
        if (t == kJpegEncGroup - 1) carry = end;
        __syncthreads();
    }
    if (t == 0) e.ulen[blockIdx.x] = (carry + 7u) >> 3;
}

// Stage D.  One lane a block: its codes at its bit offset; the last block of a restart interval (and of the scan) fills the
// rest of its last byte with one-bits.
__global__ void __launch_bounds__(kJpegEncGroup) jpeg_enc_write_kernel(JpegEncLaunch e) {
    __shared__ unsigned tab[2 * 16 + 2 * 256];
    jpeg_enc_load_tables(tab, e.huff);
    const unsigned g = blockIdx.x * kJpegEncGroup + threadIdx.x;
    if (g >= e.total_blocks) return;
    const JpegEncImage im = e.images[jpeg_enc_owner(e.block_start, e.n_images, g)];
    const unsigned s = g - im.block0;
    const JpegEncBlockRef ref = jpeg_enc_locate(im, s, e.coef);
    unsigned w[32];
    jpeg_enc_load_block(e.coef, (size_t)im.block0 + ref.plane_index, w);
    const int t = ref.comp ? 1 : 0;
    const unsigned pos = e.offs[g];
    JpegEncWriter sink;
    sink.words = reinterpret_cast<unsigned*>(e.workspace + im.ubytes);
    sink.limit = im.ucap >> 2;
    sink.w = pos >> 5;
    sink.n = (int)(pos & 31);
    jpeg_enc_block(w, ref.pred, tab + 16 * t, tab + 32 + 256 * t, sink);
    const bool last = s + 1 == im.n_blocks || (im.ri_blocks && (s + 1) % im.ri_blocks == 0);
    if (last && (sink.n & 7)) {
        const int pad = 8 - (sink.n & 7);
        sink.put((1u << pad) - 1, pad);
    }
    if (sink.n) sink.flush();
}

__device__ inline unsigned jpeg_enc_ff_bytes(unsigned v) {             // how many of the four bytes are 0xFF
    const unsigned m = v & (v >> 4) & 0x0f0f0f0fu;                      // low nibble of each byte: both nibbles' AND
    const unsigned all = m & (m >> 2) & 0x03030303u;
    return __popc(all & (all >> 1) & 0x01010101u);
}

// Stage E.  One workgroup an image: lane t of a tile counts the 0xFF bytes of chunk t (the bytes behind the scan's end are
// still zero), the tile is scanned in LDS and chained by a carry.  The stuffed length follows: every 0xFF takes a byte more,
// every interval but the first a marker.
__global__ void __launch_bounds__(kJpegEncGroup) jpeg_enc_stuff_scan_kernel(JpegEncLaunch e) {
    __shared__ unsigned sc[kJpegEncGroup];
    __shared__ unsigned carry;
    const JpegEncImage im = e.images[blockIdx.x];
    const int t = threadIdx.x;
    const unsigned L = e.ulen[blockIdx.x];
    const unsigned chunks = min((L + kJpegEncChunk - 1) / kJpegEncChunk, im.n_chunks);
    if (t == 0) carry = 0;
    __syncthreads();
    for (unsigned base = 0; base < chunks; base += kJpegEncGroup) {
        const unsigned c = base + t;
        unsigned n = 0;
        if (c < chunks) {
            const uint4* p = reinterpret_cast<const uint4*>(e.workspace + im.ubytes + (size_t)c * kJpegEncChunk);
#pragma unroll
            for (int i = 0; i < kJpegEncChunk / 16; ++i) {
                const uint4 q = p[i];
                n += jpeg_enc_ff_bytes(q.x) + jpeg_enc_ff_bytes(q.y) + jpeg_enc_ff_bytes(q.z) + jpeg_enc_ff_bytes(q.w);
            }
        }
        unsigned sum = n;
        sc[t] = sum;
        __syncthreads();
        for (int d = 1; d < kJpegEncGroup; d <<= 1) {
            const unsigned p = t >= d ? sc[t - d] : 0;
            __syncthreads();
            sum += p;
            sc[t] = sum;
            __syncthreads();
        }
        const unsigned before = carry;
        if (c < chunks) e.ffbase[im.chunk0 + c] = before + sum - n;
        __syncthreads();
        if (t == kJpegEncGroup - 1) carry = before + sum;
        __syncthreads();
    }
    if (t == 0) e.slen[blockIdx.x] = L + carry + 2u * (im.n_int - 1u);
}

// Stage F.  One lane a chunk of the un-stuffed scan: its bytes go out behind the bytes, the stuffing zeros and the markers in
// front of it; RSTn stands in front of the first byte of interval n + 1, numbered modulo 8.
__global__ void __launch_bounds__(kJpegEncGroup) jpeg_enc_stuff_kernel(JpegEncLaunch e) {
    const unsigned q = blockIdx.x * kJpegEncGroup + threadIdx.x;
    if (q >= e.total_chunks) return;
    const int i = jpeg_enc_owner(e.chunk_start, e.n_images, q);
    const JpegEncImage im = e.images[i];
    const unsigned L = min(e.ulen[i], im.ucap);
    const unsigned b0 = (q - im.chunk0) * kJpegEncChunk;
    if (b0 >= L) return;
    const unsigned* starts = e.istart + im.int0;
    unsigned lo = 0, hi = im.n_int;                    // starts[lo] < b0 or lo == 0; starts[hi] >= b0 (hi == n_int: none)
    while (hi - lo > 1) {
        const unsigned mid = (lo + hi) >> 1;
        if (starts[mid] < b0) lo = mid; else hi = mid;
    }
    unsigned next = lo + 1;                            // the first interval that starts at b0 or behind it
    unsigned next_at = next < im.n_int ? starts[next] : 0xffffffffu;
    const unsigned char* in = e.workspace + im.ubytes;
    unsigned char* out = e.workspace + im.sbytes;
    unsigned o = b0 + e.ffbase[q] + 2u * lo;
    const unsigned end = min(b0 + kJpegEncChunk, L);
    for (unsigned j = b0; j < end; ++j) {
        if (j == next_at) {
            if (o + 1 < im.scap) { out[o] = 0xFF; out[o + 1] = (unsigned char)(0xD0 + ((next - 1) & 7)); }
            o += 2;
            ++next;
            next_at = next < im.n_int ? starts[next] : 0xffffffffu;
        }
        const unsigned char v = in[j];
        if (o < im.scap) out[o] = v;
        ++o;
        if (v == 0xFF) {
            if (o < im.scap) out[o] = 0;
            ++o;
        }
    }
}

static unsigned groups(unsigned n, unsigned per) { return (n + per - 1) / per; }

hipError_t launch_jpeg_enc_dct(const JpegEncLaunch& e, hipStream_t s) {
    hipLaunchKernelGGL(jpeg_enc_dct_kernel, dim3(groups(e.total_blocks, kJpegEncBlocksPerGroup)), dim3(kJpegEncBlocksPerGroup * 8), 0, s, e);
    return hipGetLastError();
}
hipError_t launch_jpeg_enc_lengths(const JpegEncLaunch& e, hipStream_t s) {
    hipLaunchKernelGGL(jpeg_enc_lengths_kernel, dim3(groups(e.total_blocks, kJpegEncGroup)), dim3(kJpegEncGroup), 0, s, e);
    return hipGetLastError();
}
hipError_t launch_jpeg_enc_offsets(const JpegEncLaunch& e, hipStream_t s) {
    hipLaunchKernelGGL(jpeg_enc_offsets_kernel, dim3(e.n_images), dim3(kJpegEncGroup), 0, s, e);
    return hipGetLastError();
}
hipError_t launch_jpeg_enc_write(const JpegEncLaunch& e, hipStream_t s) {
    hipLaunchKernelGGL(jpeg_enc_write_kernel, dim3(groups(e.total_blocks, kJpegEncGroup)), dim3(kJpegEncGroup), 0, s, e);
    return hipGetLastError();
}
hipError_t launch_jpeg_enc_stuff_scan(const JpegEncLaunch& e, hipStream_t s) {
    hipLaunchKernelGGL(jpeg_enc_stuff_scan_kernel, dim3(e.n_images), dim3(kJpegEncGroup), 0, s, e);
    return hipGetLastError();
}
hipError_t launch_jpeg_enc_stuff(const JpegEncLaunch& e, hipStream_t s) {
    hipLaunchKernelGGL(jpeg_enc_stuff_kernel, dim3(groups(e.total_chunks, kJpegEncGroup)), dim3(kJpegEncGroup), 0, s, e);
    return hipGetLastError();
}

}  // namespace lwp
