// JPEG entropy decode on the device: self-synchronising parallel Huffman decoding of baseline scans (Weissenberger & Schmidt,
// "Massively Parallel Huffman Decoding on GPUs", ICPP 2018, in its JPEG form), bit for bit with jpeg_host.cpp's decoder.
//
// The host pre-pass (jpeg_scan_segments) leaves the scan's bytes un-stuffed and cut into segments at the RSTn markers.  A
// segment's bit stream is cut into subsequences of subseq_bytes; one lane owns one subsequence.  The decoder state is the
// triple (bit position, block index within the MCU, coefficient index k; k = 0: a DC symbol is next) and two states are
// equal only if all three agree.  Four launches on one stream, no host round trip between them:
//   1. sync inside a workgroup (jpeg_entropy_sync_kernel): every lane decodes from the first bit of its subsequence in the cold
//      state to the first symbol boundary at or past its end and records that exit and the block starts it saw; then lane i
//      takes lane i - 1's exit as its entry and decodes again, until no lane's entry changed, 256 rounds at the most;
//   2. sync across workgroups and the positions (jpeg_entropy_stitch_kernel, one workgroup a file): one lane per workgroup
//      boundary inside a segment walks forward from the previous workgroup's last exit, re-decoding subsequences until an exit
//      equals the recorded one; repeated until no boundary's entry changed, as many rounds as boundaries at the most (the true
//      state advances at least one workgroup a round, so the result is exact even for a stream that never synchronises).  An
//      exclusive scan of the block starts then gives every subsequence the stream index of its first block;
//   3. the write pass (jpeg_entropy_write_kernel): every lane decodes once more from its true entry; AC values go to their
//      natural-order place of the block's plane-order address, the DC DIFFERENCE to coefficient 0;
//   4. the DC scan (jpeg_entropy_dc_kernel, one wave a segment): per component an inclusive scan of the differences in STREAM
//      order, wrapping, written back to coefficient 0.
// Passes 3 and 4 detect what the host refuses inside a scan and set the file's status word with an atomic.
//
// Bounds: bits past a segment's end read as zero (Bits::peek pads the same way) and no load leaves the byte area; every store
// is guarded by block < total_blocks and k <= 63; every decode loop advances the bit position by at least one bit a turn or
// stops, and the round loops have the caps above, so no kernel spins on malformed input.  Workgroups never wait for each other.
#include "jpeg_host.h"
#include "lwp_internal.h"

namespace lwp {
namespace {

__device__ const unsigned char kEntZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                                 41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                                 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

constexpr unsigned kDead = 0xFFFFFFFFu;               // bit position of a state behind a decoding error: past every segment's end

struct EntState { unsigned pos, bk; };                // bk: block in MCU << 8 | k
__device__ inline bool same(const EntState& a, const EntState& b) { return a.pos == b.pos && a.bk == b.bk; }
__device__ inline EntState exit_of(uint2 r) { return EntState{r.x, r.y & 0xFFFFu}; }

// the last index i in [lo, hi) of the ascending starts with start[i] <= v (start[lo] <= v < start[hi])
__device__ inline unsigned ent_owner(const unsigned* __restrict__ start, unsigned lo, unsigned hi, unsigned v) {
    while (hi - lo > 1) {
        const unsigned mid = (lo + hi) >> 1;
        if (start[mid] <= v) lo = mid; else hi = mid;
    }
    return lo;
}

// the 32 bits at bit position pos of the segment, zero past its end
__device__ inline unsigned ent_peek(const JpegEntropyLaunch& e, const JpegEntSeg& sg, unsigned seg_bits, unsigned pos) {
    if (pos >= seg_bits) return 0;
    const unsigned a = sg.byte0 + (pos >> 3), w = a >> 2;
    const unsigned d0 = w < e.n_words ? e.words[w] : 0u, d1 = w + 1 < e.n_words ? e.words[w + 1] : 0u;
    const unsigned long long win = ((unsigned long long)__builtin_bswap32(d0) << 32) | __builtin_bswap32(d1);
    unsigned r = (unsigned)((win << (8 * (a & 3) + (pos & 7))) >> 32);
    const unsigned left = seg_bits - pos;
    if (left < 32) r &= ~0u << (32 - left);
    return r;
}

struct EntWrite {                                     // the write pass's side of a decode
    const JpegEntFile* f;
    int16_t* coef;
    unsigned n;                                       // block starts so far, file-relative: the next block to start
    unsigned end_block;                               // the segment's first_block + n_blocks
    unsigned cur;                                     // plane-order address of the block being filled, file-relative
    bool bad, finished;                               // a refusal was detected; the segment's last block was seen closed
};

// plane-order address of the block with stream index n (jpeg_decode_blocks' blk), file-relative; total_blocks: none
__device__ inline unsigned ent_block_address(const JpegEntFile& f, unsigned n) {
    const unsigned mcu = n / (unsigned)f.blocks_per_mcu, b = n % (unsigned)f.blocks_per_mcu;
    const unsigned my = mcu / (unsigned)f.mcus_x, mx = mcu % (unsigned)f.mcus_x;
    unsigned c = 0, u = 0, v = 0, hs = 1, vs = 1;
    if (f.components > 1) {
        const unsigned luma = (unsigned)(f.h0 * f.v0);
        if (b < luma) { v = b / (unsigned)f.h0; u = b % (unsigned)f.h0; hs = (unsigned)f.h0; vs = (unsigned)f.v0; }
        else c = min(1u + (b - luma), 2u);
    }
    const unsigned long long a = (unsigned long long)f.plane_block[c] + ((unsigned long long)my * vs + v) * (unsigned)f.blocks_w[c] + (mx * hs + u);
    return a < f.total_blocks ? (unsigned)a : f.total_blocks;
}

__device__ inline int ent_component(const JpegEntFile& f, unsigned bim) {
    if (f.components == 1) return 0;
    const unsigned luma = (unsigned)(f.h0 * f.v0);
    return bim < luma ? 0 : min((int)(1u + (bim - luma)), 2);
}

// Decodes from st while the bit position is below limit (a symbol boundary at or past limit ends it) and returns the block
// starts seen.  tab: the file's kJpegHuffPerFile tables in LDS.  An error leaves the dead state.  With WRITE the coefficients
// are stored and the refusals detected; the state sequence is the same in both forms.
template <bool WRITE>
__device__ inline unsigned ent_decode(const JpegEntropyLaunch& e, const JpegEntFile& f, const JpegEntSeg& sg, const JpegHuffFlat* tab,
                                      EntState& st, unsigned limit, EntWrite* w) {
    const unsigned seg_bits = sg.n_bytes * 8u;
    unsigned pos = st.pos, bim = st.bk >> 8, k = st.bk & 255u, count = 0;
    while (pos < limit) {                             // every turn adds at least one bit to pos, or leaves
        if (WRITE) {
            if (w->n > w->end_block) break;           // behind the segment's last block: another lane saw it closed
            if (w->n == w->end_block && k == 0) {
                if (seg_bits - pos >= 8) w->bad = true;   // whole bytes nobody read
                w->finished = true;
                break;
            }
        }
        const unsigned bits = ent_peek(e, sg, seg_bits, pos);
        const JpegHuffFlat& t = tab[(k == 0 ? 0 : 3) + ent_component(f, bim)];
        unsigned l = 0, sym = 0;
        const unsigned hit = t.look[bits >> 23];
        if (hit) {
            l = hit >> 8; sym = hit & 255u;
        } else {
            const unsigned v16 = bits >> 16;
            for (unsigned len = 10; len <= 16; ++len) {
                const int code = (int)(v16 >> (16 - len));
                if (t.maxcode[len] >= 0 && code <= t.maxcode[len] && code >= t.mincode[len]) {
                    l = len; sym = t.vals[(t.valptr[len] + code - t.mincode[len]) & 255];
                    break;
                }
            }
        }
        bool err = l == 0;                            // a code that matches no symbol
        unsigned sz = 0;
        if (!err) {
            if (k == 0) { sz = sym; err = sz > 11; }
            else {
                const unsigned r = sym >> 4;
                sz = sym & 15u;
                if (sz == 0) {
                    if (r == 15) { k += 16; err = k > 63; }
                    else k = 64;                      // end of block
                } else {
                    k += r;
                    err = k > 63 || sz > 10;
                }
            }
        }
        if (!err) err = pos + l + sz > seg_bits;      // the data ends inside the symbol
        if (err) {
            if (WRITE) w->bad = true;
            pos = kDead; bim = 0; k = 0;
            break;
        }
        int val = 0;
        if (sz) {
            const int raw = (int)((bits << l) >> (32 - sz));
            val = raw < (1 << (sz - 1)) ? raw - (1 << sz) + 1 : raw;
        }
        pos += l + sz;
        if (k == 0) {                                 // that was a DC symbol: a block starts
            ++count;
            if (WRITE) {
                w->cur = ent_block_address(f, w->n);
                ++w->n;
                if (w->cur < f.total_blocks) w->coef[((size_t)f.block0 + w->cur) * 64] = (int16_t)val;
            }
            k = 1;
        } else if (sz) {
            if (WRITE && w->cur < f.total_blocks && k <= 63) w->coef[((size_t)f.block0 + w->cur) * 64 + kEntZigzag[k]] = (int16_t)val;
            ++k;
        }
        if (k >= 64) { k = 0; bim = bim + 1 == (unsigned)f.blocks_per_mcu ? 0 : bim + 1; }
    }
    st.pos = pos; st.bk = (bim << 8) | k;
    return count;
}

// what a lane of the sync and write passes knows of its subsequence
struct EntLane {
    bool live, cold;                                  // it has a subsequence; that is a segment's first
    unsigned g, seg, start, limit;                    // batch index, segment, first bit and end bit
    bool last;                                        // the segment's last
};

__device__ inline EntLane ent_lane(const JpegEntropyLaunch& e, const JpegEntFile& f, unsigned local) {
    EntLane L{};
    L.live = local < f.n_subs;
    if (!L.live) return L;
    L.g = f.sub0 + local;
    L.seg = ent_owner(e.seg_sub0, f.seg0, f.seg0 + f.n_segs, L.g);
    const unsigned j = L.g - e.seg_sub0[L.seg], seg_bits = e.segs[L.seg].n_bytes * 8u, sub_bits = (unsigned)e.subseq_bytes * 8u;
    L.cold = j == 0;
    L.last = L.g + 1 == e.seg_sub0[L.seg + 1];
    L.start = j * sub_bits;
    L.limit = L.last ? seg_bits : min(L.start + sub_bits, seg_bits);
    return L;
}

__device__ inline void ent_load_tables(const JpegEntropyLaunch& e, unsigned file, uint4* lds) {
    const uint4* src = reinterpret_cast<const uint4*>(e.tables + (size_t)file * kJpegHuffPerFile);
    constexpr int n = (int)(kJpegHuffPerFile * sizeof(JpegHuffFlat) / 16);
    for (int i = (int)threadIdx.x; i < n; i += kJpegEntropyGroup) lds[i] = src[i];
}

constexpr int kTableWords16 = (int)(kJpegHuffPerFile * sizeof(JpegHuffFlat) / 16);

__global__ void __launch_bounds__(kJpegEntropyGroup) jpeg_entropy_sync_kernel(JpegEntropyLaunch e) {
    __shared__ uint4 tab_raw[kTableWords16];
    __shared__ uint2 exits[kJpegEntropyGroup];
    const unsigned file = ent_owner(e.file_wg0, 0, (unsigned)e.n_files, blockIdx.x);
    const JpegEntFile f = e.files[file];
    ent_load_tables(e, file, tab_raw);
    const JpegHuffFlat* tab = reinterpret_cast<const JpegHuffFlat*>(tab_raw);
    const unsigned t = threadIdx.x;
    const EntLane L = ent_lane(e, f, (blockIdx.x - f.wg0) * kJpegEntropyGroup + t);
    JpegEntSeg sg{};
    if (L.live) sg = e.segs[L.seg];
    __syncthreads();
    // round 0: the cold state at the subsequence's first bit
    EntState used{L.start, 0}, st = used;
    unsigned count = 0;
    if (L.live) count = ent_decode<false>(e, f, sg, tab, st, L.limit, nullptr);
    exits[t] = make_uint2(st.pos, st.bk);
    __syncthreads();
    const bool follows = L.live && !L.cold && t > 0;  // lane 0's predecessor is another workgroup's: the stitch kernel's business
    int rounds = 1;
    for (; rounds <= kJpegEntropyGroup; ++rounds) {
        EntState entry = used;
        if (follows) entry = exit_of(exits[t - 1]);
        __syncthreads();
        int changed = 0;
        if (follows && !same(entry, used)) {
            used = entry; st = entry;
            count = ent_decode<false>(e, f, sg, tab, st, L.limit, nullptr);
            exits[t] = make_uint2(st.pos, st.bk);
            changed = 1;
        }
        if (!__syncthreads_or(changed)) break;
    }
    if (L.live) e.rec[L.g] = make_uint2(st.pos, (count << 16) | st.bk);
    if (t == 0) atomicMax(&e.status[e.n_files], rounds);
}

__global__ void __launch_bounds__(kJpegEntropyGroup) jpeg_entropy_stitch_kernel(JpegEntropyLaunch e) {
    __shared__ uint4 tab_raw[kTableWords16];
    __shared__ unsigned sc[kJpegEntropyGroup];
    const unsigned file = blockIdx.x, t = threadIdx.x;
    const JpegEntFile f = e.files[file];
    if (f.n_subs == 0) return;                        // the same in every lane
    ent_load_tables(e, file, tab_raw);
    const JpegHuffFlat* tab = reinterpret_cast<const JpegHuffFlat*>(tab_raw);
    for (unsigned w = 1 + t; w < f.n_wgs; w += kJpegEntropyGroup) e.wg_entry[f.wg0 + w] = make_uint2(kDead - 1, 0xFFFFFFFFu);   // no state
    __syncthreads();
    int rounds = 0;
    for (unsigned r = 0; r + 1 < f.n_wgs; ++r) {
        for (unsigned w = 1 + t; w < f.n_wgs; w += kJpegEntropyGroup) {
            const unsigned g = f.sub0 + w * kJpegEntropyGroup;
            const unsigned seg = ent_owner(e.seg_sub0, f.seg0, f.seg0 + f.n_segs, g);
            unsigned dirty = 0;
            if (g != e.seg_sub0[seg]) {               // the boundary lies inside a segment
                const uint2 prev = e.rec[g - 1], old = e.wg_entry[f.wg0 + w];
                if (prev.x != old.x || (prev.y & 0xFFFFu) != old.y) { e.wg_entry[f.wg0 + w] = make_uint2(prev.x, prev.y & 0xFFFFu); dirty = 1; }
            }
            e.wg_dirty[f.wg0 + w] = dirty;
        }
        __syncthreads();
        int any = 0;
        for (unsigned w = 1 + t; w < f.n_wgs; w += kJpegEntropyGroup) {
            if (!e.wg_dirty[f.wg0 + w]) continue;
            any = 1;
            const unsigned g0 = f.sub0 + w * kJpegEntropyGroup;
            const unsigned seg = ent_owner(e.seg_sub0, f.seg0, f.seg0 + f.n_segs, g0);
            const JpegEntSeg sg = e.segs[seg];
            const unsigned seg_bits = sg.n_bytes * 8u, sub_bits = (unsigned)e.subseq_bytes * 8u;
            const unsigned stop = min(min(g0 + kJpegEntropyGroup, f.sub0 + f.n_subs), e.seg_sub0[seg + 1]);
            const uint2 en = e.wg_entry[f.wg0 + w];
            EntState st{en.x, en.y};
            for (unsigned g = g0; g < stop; ++g) {
                const unsigned j = g - sg.sub0;
                const unsigned limit = g + 1 == e.seg_sub0[seg + 1] ? seg_bits : min((j + 1) * sub_bits, seg_bits);
                const unsigned count = ent_decode<false>(e, f, sg, tab, st, limit, nullptr);
                const uint2 old = e.rec[g];
                e.rec[g] = make_uint2(st.pos, (count << 16) | st.bk);
                if (same(st, exit_of(old))) break;
            }
        }
        ++rounds;
        if (!__syncthreads_or(any)) break;
    }
    if (t == 0) atomicMax(&e.status[e.n_files + 1], rounds);
    __syncthreads();
    // positions: an exclusive scan of the block starts over the file's subsequences (a segment subtracts its first's)
    unsigned carry = 0;
    for (unsigned base = 0; base < f.n_subs; base += kJpegEntropyGroup) {
        const unsigned i = base + t;
        const unsigned c = i < f.n_subs ? e.rec[f.sub0 + i].y >> 16 : 0u;
        sc[t] = c;
        __syncthreads();
        for (unsigned off = 1; off < kJpegEntropyGroup; off <<= 1) {
            const unsigned v = t >= off ? sc[t - off] : 0u;
            __syncthreads();
            sc[t] += v;
            __syncthreads();
        }
        if (i < f.n_subs) e.subpos[f.sub0 + i] = carry + sc[t] - c;
        carry += sc[kJpegEntropyGroup - 1];
        __syncthreads();
    }
}

__global__ void __launch_bounds__(kJpegEntropyGroup) jpeg_entropy_write_kernel(JpegEntropyLaunch e) {
    __shared__ uint4 tab_raw[kTableWords16];
    const unsigned file = ent_owner(e.file_wg0, 0, (unsigned)e.n_files, blockIdx.x);
    const JpegEntFile f = e.files[file];
    ent_load_tables(e, file, tab_raw);
    const JpegHuffFlat* tab = reinterpret_cast<const JpegHuffFlat*>(tab_raw);
    __syncthreads();
    const EntLane L = ent_lane(e, f, (blockIdx.x - f.wg0) * kJpegEntropyGroup + threadIdx.x);
    if (!L.live) return;
    const JpegEntSeg sg = e.segs[L.seg];
    EntState st{0, 0};
    if (!L.cold) st = exit_of(e.rec[L.g - 1]);
    EntWrite w{};
    w.f = &f; w.coef = e.coef;
    w.n = sg.first_block + (e.subpos[L.g] - e.subpos[sg.sub0]);
    w.end_block = sg.first_block + sg.n_blocks;
    const unsigned k = st.bk & 255u;
    w.cur = k != 0 && w.n >= 1 && w.n <= w.end_block ? ent_block_address(f, w.n - 1) : f.total_blocks;
    w.bad = st.pos == kDead && L.last;
    ent_decode<true>(e, f, sg, tab, st, L.limit, &w);
    // the segment's end: every block there and the last one closed (a lane behind the last block has nothing to add)
    if (L.last && !w.finished && w.n <= w.end_block && !(w.n == w.end_block && (st.bk & 255u) == 0 && st.pos != kDead)) w.bad = true;
    if (w.bad) atomicOr(&e.status[file], 1);
}

// One wave a segment.  Component c's blocks of the segment in stream order: hv of every MCU; 64 at a time, an inclusive scan
// across the wave and a carry.
__global__ void __launch_bounds__(kJpegEntropyGroup) jpeg_entropy_dc_kernel(JpegEntropyLaunch e) {
    const unsigned lane = threadIdx.x & 63u, s = blockIdx.x * (kJpegEntropyGroup / 64) + (threadIdx.x >> 6);
    if (s >= e.n_segs) return;                        // the same in every lane of the wave
    const JpegEntSeg sg = e.segs[s];
    const JpegEntFile f = e.files[sg.file];
    const unsigned mcu0 = sg.first_block / (unsigned)f.blocks_per_mcu, n_mcus = sg.n_blocks / (unsigned)f.blocks_per_mcu;
    bool bad = false;
    unsigned in_mcu0 = 0;
    for (int c = 0; c < f.components; ++c) {
        const unsigned hv = c == 0 && f.components > 1 ? (unsigned)(f.h0 * f.v0) : 1u;
        const unsigned n = n_mcus * hv;
        int carry = 0;
        for (unsigned base = 0; base < n; base += 64) {
            const unsigned i = base + lane;
            unsigned addr = f.total_blocks;
            if (i < n) addr = ent_block_address(f, (mcu0 + i / hv) * (unsigned)f.blocks_per_mcu + in_mcu0 + i % hv);
            int16_t* p = e.coef + ((size_t)f.block0 + addr) * 64;
            int v = addr < f.total_blocks ? (int)*p : 0;
            for (int off = 1; off < 64; off <<= 1) {
                const int up = __shfl_up(v, off, 64);
                if ((int)lane >= off) v = (int)((unsigned)v + (unsigned)up);
            }
            v = (int)((unsigned)v + (unsigned)carry);
            if (addr < f.total_blocks) {
                if (v < -2048 || v > 2047) bad = true;
                *p = (int16_t)v;
            }
            carry = __shfl(v, 63, 64);
        }
        in_mcu0 += hv;
    }
    if (bad) atomicOr(&e.status[sg.file], 1);
}

}  // namespace

hipError_t launch_jpeg_entropy(const JpegEntropyLaunch& e, hipStream_t s) {
    if (e.n_wgs == 0) return hipSuccess;
    hipLaunchKernelGGL(jpeg_entropy_sync_kernel, dim3(e.n_wgs), dim3(kJpegEntropyGroup), 0, s, e);
    hipLaunchKernelGGL(jpeg_entropy_stitch_kernel, dim3((unsigned)e.n_files), dim3(kJpegEntropyGroup), 0, s, e);
    hipLaunchKernelGGL(jpeg_entropy_write_kernel, dim3(e.n_wgs), dim3(kJpegEntropyGroup), 0, s, e);
    hipLaunchKernelGGL(jpeg_entropy_dc_kernel, dim3((e.n_segs + kJpegEntropyGroup / 64 - 1) / (kJpegEntropyGroup / 64)), dim3(kJpegEntropyGroup), 0, s, e);
    return hipGetLastError();
}

}  // namespace lwp
