// COCO key-point evaluation on the device: COCOeval (pycocotools cocoeval.py) for iouType 'keypoints' with its default
// parameters, one category.  coco_match_kernel is computeOks + evaluateImg, one workgroup per image; the dataset's selected
// detections are then ordered by score (rocPRIM's stable radix sort on an order-preserving key) and coco_accumulate_kernel is
// accumulate, one workgroup per (area range, IoU threshold).  Everything is float64 and every operation is rounded on its own,
// as NumPy's are: this translation unit is built with -ffp-contract=off (build.py), and the pragma below says the same to the
// front end.  The counts are integers and the divisions IEEE, so precision / recall / scores have one answer; only exp() may
// differ from the host's in its last bit, which the OKS sum carries.
#include <cmath>
#include <cstring>

#include <rocprim/device/device_radix_sort.hpp>

#include "lwp_internal.h"

#pragma clang fp contract(off)

namespace lwp {

constexpr int kEvalThreads = 256;
static_assert(kEvalScanChunk == kEvalThreads, "the scans take one element per thread and step");
static_assert(kEvalAT <= kEvalThreads && kEvalR <= kEvalThreads && kEvalMaxDets <= kEvalThreads, "one thread each");

// Params.iouThrs / recThrs / kpt_oks_sigmas / areaRng as NumPy computes them: linspace is arange * step + start with the
// last value set to stop, and each operation is rounded separately
void coco_eval_defaults(CocoEvalParams* p) {
    static const double sig[kEvalK] = {.26, .25, .25, .35, .35, .79, .79, .72, .72, .62, .62, 1.07, 1.07, .87, .87, .89, .89};
    for (int k = 0; k < kEvalK; ++k) {
        volatile double s = sig[k] / 10.0;
        volatile double s2 = s * 2;
        p->vars[k] = s2 * s2;
    }
    volatile double step_t = (0.95 - 0.5) / (kEvalT - 1), step_r = (1.0 - 0.0) / (kEvalR - 1);
    for (int i = 0; i < kEvalT; ++i) {
        volatile double v = (double)i * step_t;
        p->iou_thr[i] = v + 0.5;
    }
    p->iou_thr[kEvalT - 1] = 0.95;
    for (int i = 0; i < kEvalR; ++i) {
        volatile double v = (double)i * step_r;
        p->rec_thr[i] = v + 0.0;
    }
    p->rec_thr[kEvalR - 1] = 1.0;
    const double lo[kEvalA] = {0.0, 32.0 * 32.0, 96.0 * 96.0}, hi[kEvalA] = {1e5 * 1e5, 96.0 * 96.0, 1e5 * 1e5};   // all, medium, large
    for (int a = 0; a < kEvalA; ++a) { p->area_lo[a] = lo[a]; p->area_hi[a] = hi[a]; }
}

// ---------------------------------------------------------------------------------------------- per image
__global__ void __launch_bounds__(kEvalThreads) coco_match_kernel(const CocoEvalParams p) {
    const int img = blockIdx.x, tid = threadIdx.x;
    const int64_t d0 = p.dt_off[img], g0 = p.gt_off[img];
    const int64_t D = p.dt_off[img + 1] - d0, G = p.gt_off[img + 1] - g0;
    const int64_t s0 = p.sel_off[img], o0 = p.oks_off[img];
    const int Ds = (int)(D < kEvalMaxDets ? D : kEvalMaxDets);
    __shared__ int s_sel[kEvalMaxDets];
    __shared__ double s_kp[kEvalMaxDets][kEvalK][2];
    __shared__ double s_area[kEvalMaxDets];
    __shared__ int s_npig[kEvalA];
    if (tid < kEvalA) s_npig[tid] = 0;

    // argsort(-score, kind='mergesort')[:20] by counting: the rank of a detection is the number of detections in front of it
    for (int64_t d = tid; d < D; d += kEvalThreads) {
        const double s = p.dt_score[d0 + d];
        int rank = 0;
        for (int64_t e = 0; e < D && rank < kEvalMaxDets; ++e) {
            const double se = p.dt_score[d0 + e];
            rank += (se > s || (se == s && e < d)) ? 1 : 0;
        }
        if (rank < kEvalMaxDets) s_sel[rank] = (int)d;
    }
    __syncthreads();
    for (int i = tid; i < Ds * kEvalK; i += kEvalThreads) {
        const int r = i / kEvalK, k = i - r * kEvalK;
        const double* kp = p.dt_kp + ((d0 + s_sel[r]) * kEvalK + k) * 3;
        s_kp[r][k][0] = kp[0];
        s_kp[r][k][1] = kp[1];
    }
    // ground truths: crowd and per-range ignore flags, and how many count in each range
    for (int64_t g = tid; g < G; g += kEvalThreads) {
        const double area = p.gt_area[g0 + g];
        const bool ig = p.gt_ignore[g0 + g] != 0;
        unsigned f = p.gt_iscrowd[g0 + g] != 0 ? 1u : 0u;
        for (int a = 0; a < kEvalA; ++a) {
            const bool iga = ig || area < p.area_lo[a] || area > p.area_hi[a];
            if (iga) f |= 2u << a;
            else atomicAdd(&s_npig[a], 1);
        }
        p.gt_flag[g0 + g] = (unsigned char)f;
    }
    __syncthreads();
    if (tid < Ds) {
        // loadRes: the box of all 17 entries, the zeros of missing key-points included
        double x0 = s_kp[tid][0][0], x1 = x0, y0 = s_kp[tid][0][1], y1 = y0;
        for (int k = 1; k < kEvalK; ++k) {
            x0 = fmin(x0, s_kp[tid][k][0]); x1 = fmax(x1, s_kp[tid][k][0]);
            y0 = fmin(y0, s_kp[tid][k][1]); y1 = fmax(y1, s_kp[tid][k][1]);
        }
        s_area[tid] = (x1 - x0) * (y1 - y0);
        p.sel_idx[s0 + tid] = s_sel[tid];
        p.sel_score[s0 + tid] = p.dt_score[d0 + s_sel[tid]];
    }
    if (tid < kEvalA) p.npig_img[(int64_t)img * kEvalA + tid] = s_npig[tid];

    // computeOks: entry (i, j) of the selected detections x all ground truths, columns in input order
    const int64_t n_oks = (int64_t)Ds * G;
    for (int64_t idx = tid; idx < n_oks; idx += kEvalThreads) {
        const int i = (int)(idx / G);
        const int64_t j = idx - (int64_t)i * G;
        const double* gk = p.gt_kp + (g0 + j) * kEvalK * 3;
        int k1 = 0;
        for (int k = 0; k < kEvalK; ++k) k1 += gk[3 * k + 2] > 0 ? 1 : 0;
        const double area = p.gt_area[g0 + j] + 2.220446049250313e-16;       // np.spacing(1)
        double sum = 0;
        if (k1 > 0) {
            for (int k = 0; k < kEvalK; ++k) {
                if (!(gk[3 * k + 2] > 0)) continue;
                const double dx = s_kp[i][k][0] - gk[3 * k], dy = s_kp[i][k][1] - gk[3 * k + 1];
                const double e = (dx * dx + dy * dy) / p.vars[k] / area / 2;
                sum += exp(-e);
            }
        } else {
            // no visible key-point: the distance to the doubled box, over all 17
            const double* bb = p.gt_bbox + (g0 + j) * 4;
            const double bx0 = bb[0] - bb[2], bx1 = bb[0] + bb[2] * 2, by0 = bb[1] - bb[3], by1 = bb[1] + bb[3] * 2;
            for (int k = 0; k < kEvalK; ++k) {
                const double xd = s_kp[i][k][0], yd = s_kp[i][k][1];
                const double dx = fmax(0.0, bx0 - xd) + fmax(0.0, xd - bx1), dy = fmax(0.0, by0 - yd) + fmax(0.0, yd - by1);
                const double e = (dx * dx + dy * dy) / p.vars[k] / area / 2;
                sum += exp(-e);
            }
        }
        p.oks[o0 + idx] = sum / (double)(k1 > 0 ? k1 : kEvalK);
    }
    __syncthreads();      // the OKS entries and the flags, written to global memory by other threads of this workgroup, are read below

    // evaluateImg: 30 independent greedy matchings, one thread each.  The stable order "not ignored first" is two passes over
    // the ground truths; the reference's break (an ignored GT while a counted match is held) skips the second pass.
    if (tid >= kEvalAT) return;
    const int a = tid / kEvalT, t = tid - a * kEvalT;
    unsigned char* gm = p.gt_m + (int64_t)tid * p.NG + g0;
    const unsigned char* gf = p.gt_flag + g0;
    for (int di = 0; di < Ds; ++di) {
        double iou = fmin(p.iou_thr[t], 1 - 1e-10);
        int64_t m = -1;
        const double* row = p.oks + o0 + (int64_t)di * G;
        for (unsigned pass = 0; pass < 2 && !(pass == 1 && m > -1); ++pass)
            for (int64_t g = 0; g < G; ++g) {
                const unsigned f = gf[g];
                if (((f >> (1 + a)) & 1u) != pass) continue;
                if (gm[g] && !(f & 1u)) continue;      // matched already, and not a crowd
                const double v = row[g];
                if (v < iou) continue;                 // equality takes the later GT
                iou = v;
                m = g;
            }
        unsigned ig;
        if (m > -1) {
            ig = (gf[m] >> (1 + a)) & 1u;
            gm[m] = 1;
        } else {
            ig = (s_area[di] < p.area_lo[a] || s_area[di] > p.area_hi[a]) ? 1u : 0u;
        }
        p.dt_m[(int64_t)tid * p.NS + s0 + di] = m > -1 ? 1 : 0;
        p.dt_ig[(int64_t)tid * p.NS + s0 + di] = (unsigned char)ig;
    }
}

hipError_t launch_coco_match(const CocoEvalParams& p, hipStream_t s) {
    if (p.n_images < 1) return hipSuccess;
    hipLaunchKernelGGL(coco_match_kernel, dim3(p.n_images), dim3(kEvalThreads), 0, s, p);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------- order of the accumulation
// a key whose unsigned order is the score's; -0.0 sorts with 0.0, as NumPy's comparison has it
__global__ void __launch_bounds__(kEvalThreads) coco_keys_kernel(const double* __restrict__ score, int64_t NS,
                                                                 unsigned long long* __restrict__ keys, unsigned int* __restrict__ vals) {
    for (int64_t i = (int64_t)blockIdx.x * kEvalThreads + threadIdx.x; i < NS; i += (int64_t)gridDim.x * kEvalThreads) {
        double s = score[i];
        if (s == 0.0) s = 0.0;
        const unsigned long long b = (unsigned long long)__double_as_longlong(s);
        keys[i] = (b >> 63) ? ~b : (b | 0x8000000000000000ull);
        vals[i] = (unsigned int)i;
    }
}

hipError_t coco_sort_temp_bytes(int64_t NS, size_t* bytes) {
    *bytes = 0;
    if (NS < 1) return hipSuccess;
    return rocprim::radix_sort_pairs_desc(nullptr, *bytes, (unsigned long long*)nullptr, (unsigned long long*)nullptr,
                                          (unsigned int*)nullptr, (unsigned int*)nullptr, (size_t)NS, 0, 64, (hipStream_t) nullptr);
}

hipError_t launch_coco_sort(const double* sel_score, int64_t NS, unsigned long long* keys, unsigned long long* keys_out,
                            unsigned int* vals, unsigned int* perm, void* tmp, size_t tmp_bytes, hipStream_t s) {
    if (NS < 1) return hipSuccess;
    const int blocks = (int)((NS + kEvalThreads - 1) / kEvalThreads < 1024 ? (NS + kEvalThreads - 1) / kEvalThreads : 1024);
    hipLaunchKernelGGL(coco_keys_kernel, dim3(blocks), dim3(kEvalThreads), 0, s, sel_score, NS, keys, vals);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    // descending and stable: equal scores keep their (image, rank) order, argsort(-dtScores, kind='mergesort')
    return rocprim::radix_sort_pairs_desc(tmp, tmp_bytes, keys, keys_out, vals, perm, (size_t)NS, 0, 64, s);
}

// ---------------------------------------------------------------------------------------------- accumulate
// inclusive scan of one value per thread over the workgroup (Hillis-Steele between two LDS rows); returns this thread's value
// and leaves the total in buf[0][kEvalThreads - 1].  The caller synchronises before it writes buf again.
template <class T, class Op>
__device__ inline T block_scan(T v, T (*buf)[kEvalThreads], Op op) {
    const int tid = threadIdx.x;
    int cur = 0;
    buf[0][tid] = v;
    __syncthreads();
    for (int off = 1; off < kEvalThreads; off <<= 1) {
        T x = buf[cur][tid];
        if (tid >= off) x = op(buf[cur][tid - off], x);
        buf[cur ^ 1][tid] = x;
        __syncthreads();
        cur ^= 1;
    }
    static_assert(kEvalThreads == 256, "eight steps end in row 0");
    return buf[0][tid];
}

__global__ void __launch_bounds__(kEvalThreads) coco_accumulate_kernel(const CocoEvalParams p) {
    const int at = blockIdx.x, a = at / kEvalT, t = at - a * kEvalT, tid = threadIdx.x;
    __shared__ unsigned long long s_cnt[2][kEvalThreads];
    __shared__ double s_max[2][kEvalThreads];
    const int64_t NS = p.NS;

    // npig: the ground truths of the dataset that count in this range
    long long c = 0;
    for (int64_t i = tid; i < p.n_images; i += kEvalThreads) c += p.npig_img[i * kEvalA + a];
    block_scan((unsigned long long)c, s_cnt, [](unsigned long long x, unsigned long long y) { return x + y; });
    const long long npig = (long long)s_cnt[0][kEvalThreads - 1];
    __syncthreads();
    if (tid == 0 && t == 0) p.npig[a] = npig;
    if (npig == 0) {                                   // the range stays at COCOeval's initial -1
        for (int r = tid; r < kEvalR; r += kEvalThreads) {
            p.precision[((int64_t)t * kEvalR + r) * kEvalA + a] = -1.0;
            p.scores[((int64_t)t * kEvalR + r) * kEvalA + a] = -1.0;
        }
        if (tid == 0) p.recall[t * kEvalA + a] = -1.0;
        return;
    }
    const unsigned char* dm = p.dt_m + (int64_t)at * NS;
    const unsigned char* dig = p.dt_ig + (int64_t)at * NS;
    unsigned long long* tpfp = p.tpfp + (int64_t)at * NS;
    double* pr = p.pr + (int64_t)at * NS;

    // cumsum of tp and fp in score order, a chunk at a time with a carry; pr = tp / (fp + tp + spacing(1))
    unsigned long long carry = 0;
    for (int64_t base = 0; base < NS; base += kEvalScanChunk) {
        const int64_t pos = base + tid;
        unsigned long long v = 0;
        if (pos < NS) {
            const int64_t src = p.perm[pos];
            if (!dig[src]) v = dm[src] ? 1ull : (1ull << 32);
        }
        const unsigned long long incl = block_scan(v, s_cnt, [](unsigned long long x, unsigned long long y) { return x + y; }) + carry;
        if (pos < NS) {
            tpfp[pos] = incl;
            const double tp = (double)(incl & 0xffffffffull), fp = (double)(incl >> 32);
            pr[pos] = tp / (fp + tp + 2.220446049250313e-16);
        }
        carry += s_cnt[0][kEvalThreads - 1];
        __syncthreads();
    }
    // for i in range(nd - 1, 0, -1): if pr[i] > pr[i - 1]: pr[i - 1] = pr[i] -- a running maximum from the end
    double mcarry = -1.0;                              // below every precision
    for (int64_t top = NS; top > 0; top -= kEvalScanChunk) {
        const int64_t pos = top - 1 - tid;             // thread 0 takes the chunk's last element
        const double v = pos >= 0 ? pr[pos] : -1.0;
        const double incl = fmax(block_scan(v, s_max, [](double x, double y) { return fmax(x, y); }), mcarry);
        if (pos >= 0) pr[pos] = incl;
        mcarry = fmax(mcarry, s_max[0][kEvalThreads - 1]);
        __syncthreads();
    }
    // searchsorted(rc, recThrs, side='left') with rc = tp / npig; a threshold no recall reaches leaves 0
    for (int r = tid; r < kEvalR; r += kEvalThreads) {
        const double thr = p.rec_thr[r];
        int64_t lo = 0, hi = NS;
        while (lo < hi) {
            const int64_t mid = lo + (hi - lo) / 2;
            const double rc = (double)(tpfp[mid] & 0xffffffffull) / (double)npig;
            if (rc < thr) lo = mid + 1;
            else hi = mid;
        }
        p.precision[((int64_t)t * kEvalR + r) * kEvalA + a] = lo < NS ? pr[lo] : 0.0;
        p.scores[((int64_t)t * kEvalR + r) * kEvalA + a] = lo < NS ? p.sel_score[p.perm[lo]] : 0.0;
    }
    if (tid == 0) p.recall[t * kEvalA + a] = NS > 0 ? (double)(tpfp[NS - 1] & 0xffffffffull) / (double)npig : 0.0;
}

hipError_t launch_coco_accumulate(const CocoEvalParams& p, hipStream_t s) {
    hipLaunchKernelGGL(coco_accumulate_kernel, dim3(kEvalAT), dim3(kEvalThreads), 0, s, p);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------- detection store
// val.py:52-78 on the result block of the grouping: slot of each of the 18 network key-points in COCO's order (the neck has none)
__constant__ int c_coco_slot[kCocoTypes] = {0, -1, 6, 8, 10, 5, 7, 9, 12, 14, 16, 11, 13, 15, 2, 1, 4, 3};

// The control words after one more image: the first error stays.  Every thread of the workgroup carries the same values.
struct CocoCtl { long long cursor, status, image, detail; };
__device__ inline void coco_ctl_note(CocoCtl& c, int code, int image, long long detail) {
    if (c.status == COCO_ST_OK) { c.status = code; c.image = image; c.detail = detail; }
}
// rows [c.cursor, c.cursor + n) of `image`; returns how many of them lie inside the store (the others are not written)
__device__ inline int coco_ctl_claim(const CocoStore& st, CocoCtl& c, int image, int n, long long* base) {
    *base = c.cursor < (long long)st.row_cap ? c.cursor : (long long)st.row_cap;
    const long long room = (long long)st.row_cap - *base;
    const int w = (int)(room < (long long)n ? room : (long long)n);
    if (threadIdx.x == 0) { st.start[image] = (int)*base; st.count[image] = w; }
    c.cursor += n;
    return w;
}

// One workgroup for the N frames of a call, in frame order: frame f's rows start where frame f - 1's end, a row's place is its
// entry's place.  The cursor and the status are read by every thread before the loop and written by thread 0 behind it.
__global__ void __launch_bounds__(kEvalThreads) coco_append_kernel(const CocoStore st, const CocoAppendParams p) {
    const int tid = threadIdx.x;
    CocoCtl c{st.ctl[0], st.ctl[1], st.ctl[2], st.ctl[3]};
    for (int f = 0; f < p.N; ++f) {
        const int img = p.image_index[f];
        if (img < 0 || img >= st.n_images) continue;   // (checked by the host; uniform)
        const int ne = p.n_entries[f];
        const int n = ne < 0 ? 0 : (ne > p.max_entries ? p.max_entries : ne);
        long long base;
        const int w = coco_ctl_claim(st, c, img, n, &base);
        const double* ent = p.entries + (size_t)f * p.max_entries * kCocoEntry;
        const double* rows = p.kpts_out + (size_t)f * p.max_rows * 4;
        int bad = 0;
        for (int e = tid; e < w; e += kEvalThreads) {
            const double* en = ent + (size_t)e * kCocoEntry;
            double* kp = st.kp + (size_t)(base + e) * kEvalK * 3;
            for (int k = 0; k < kEvalK * 3; ++k) kp[k] = 0.0;
            for (int t = 0; t < kCocoTypes; ++t) {
                const int slot = c_coco_slot[t];
                const double id = en[t];
                if (slot < 0 || id == -1.0) continue;
                int r = (int)id;                       // the rows of a frame are stored compact and in id order
                r = r < 0 ? 0 : (r > p.max_rows - 1 ? p.max_rows - 1 : r);
                const double x = rows[(size_t)r * 4] + 0.5, y = rows[(size_t)r * 4 + 1] + 0.5;
                if (!isfinite(x) || !isfinite(y)) bad = 1;
                kp[slot * 3] = x; kp[slot * 3 + 1] = y; kp[slot * 3 + 2] = 1.0;
            }
            const double m = en[kCocoEntry - 1] - 1.0;                     // max(0, count - 1): the neck does not count
            const double s = en[kCocoEntry - 2] * (m > 0.0 ? m : 0.0);
            if (!isfinite(s)) bad = 1;
            st.score[base + e] = s;
            st.image[base + e] = img;
        }
        const int any_bad = __syncthreads_or(bad);
        const unsigned long long* fl = p.flags + (size_t)f * 4;
        if (fl[0]) coco_ctl_note(c, COCO_ST_FLAGS, img, (long long)fl[0]);
        else if (fl[1] < fl[2]) coco_ctl_note(c, COCO_ST_UNBOUND, img, 0);
        else if (w < n) coco_ctl_note(c, COCO_ST_ROWS, img, 0);
        else if (any_bad) coco_ctl_note(c, COCO_ST_NONFINITE, img, 0);
    }
    __syncthreads();
    if (tid == 0) { st.ctl[0] = c.cursor; st.ctl[1] = c.status; st.ctl[2] = c.image; st.ctl[3] = c.detail; }
}

hipError_t launch_coco_append(const CocoStore& st, const CocoAppendParams& p, hipStream_t s) {
    if (p.N < 1) return hipSuccess;
    hipLaunchKernelGGL(coco_append_kernel, dim3(1), dim3(kEvalThreads), 0, s, st, p);
    return hipGetLastError();
}

__global__ void __launch_bounds__(kEvalThreads) coco_append_rows_kernel(const CocoStore st, int img, int n, const double* __restrict__ kp,
                                                                        const double* __restrict__ score) {
    const int tid = threadIdx.x;
    CocoCtl c{st.ctl[0], st.ctl[1], st.ctl[2], st.ctl[3]};
    long long base;
    const int w = coco_ctl_claim(st, c, img, n, &base);
    for (int64_t i = tid; i < (int64_t)w * kEvalK * 3; i += kEvalThreads) st.kp[(int64_t)base * kEvalK * 3 + i] = kp[i];
    for (int e = tid; e < w; e += kEvalThreads) { st.score[base + e] = score[e]; st.image[base + e] = img; }
    if (w < n) coco_ctl_note(c, COCO_ST_ROWS, img, 0);
    __syncthreads();
    if (tid == 0) { st.ctl[0] = c.cursor; st.ctl[1] = c.status; st.ctl[2] = c.image; st.ctl[3] = c.detail; }
}

hipError_t launch_coco_append_rows(const CocoStore& st, int image, int n, const double* kp, const double* score, hipStream_t s) {
    hipLaunchKernelGGL(coco_append_rows_kernel, dim3(1), dim3(kEvalThreads), 0, s, st, image, n, kp, score);
    return hipGetLastError();
}

// dt_off[0 .. n_images] from the counts, on the device (lwp_coco_rows, which reads tables and rows behind one synchronise): one
// workgroup, a chunk of kEvalScanChunk images at a time with a carry
__global__ void __launch_bounds__(kEvalThreads) coco_offsets_kernel(const CocoStore st, int64_t* __restrict__ dt_off) {
    __shared__ unsigned long long s_cnt[2][kEvalThreads];
    const int tid = threadIdx.x;
    unsigned long long carry = 0;
    if (tid == 0) dt_off[0] = 0;
    for (int base = 0; base < st.n_images; base += kEvalScanChunk) {
        const int i = base + tid;
        int v = i < st.n_images ? st.count[i] : 0;
        v = v < 0 ? 0 : (v > st.row_cap ? st.row_cap : v);
        const unsigned long long incl = block_scan((unsigned long long)v, s_cnt, [](unsigned long long x, unsigned long long y) { return x + y; }) + carry;
        if (i < st.n_images) dt_off[i + 1] = (int64_t)incl;
        carry += s_cnt[0][kEvalThreads - 1];
        __syncthreads();
    }
}

hipError_t launch_coco_offsets(const CocoStore& st, int64_t* dt_off, hipStream_t s) {
    hipLaunchKernelGGL(coco_offsets_kernel, dim3(1), dim3(kEvalThreads), 0, s, st, dt_off);
    return hipGetLastError();
}

// one wave per destination row: lanes 0..50 move the key-points, lane 51 the score and the image index.  Rows [0, min(ND,
// dt_off[n_images])): ND bounds the destination arrays.
__global__ void __launch_bounds__(kEvalThreads) coco_gather_kernel(const CocoStore st, const int64_t* __restrict__ dt_off, int64_t ND,
                                                                   double* __restrict__ dt_kp, double* __restrict__ dt_score,
                                                                   int* __restrict__ dt_image) {
    const int lane = threadIdx.x & 63;
    const int64_t total = dt_off[st.n_images];
    if (total < ND) ND = total;
    const int64_t waves = (int64_t)gridDim.x * (kEvalThreads / 64);
    for (int64_t r = (int64_t)blockIdx.x * (kEvalThreads / 64) + (threadIdx.x >> 6); r < ND; r += waves) {
        int lo = 0, hi = st.n_images;                  // the image with dt_off[i] <= r < dt_off[i + 1]
        while (hi - lo > 1) {
            const int mid = lo + (hi - lo) / 2;
            if (dt_off[mid] <= r) lo = mid;
            else hi = mid;
        }
        int64_t src = (int64_t)st.start[lo] + (r - dt_off[lo]);
        src = src < 0 ? 0 : (src > (int64_t)st.row_cap - 1 ? (int64_t)st.row_cap - 1 : src);
        if (lane < kEvalK * 3) dt_kp[r * kEvalK * 3 + lane] = st.kp[src * kEvalK * 3 + lane];
        else if (lane == kEvalK * 3) {
            dt_score[r] = st.score[src];
            if (dt_image) dt_image[r] = lo;
        }
    }
}

hipError_t launch_coco_gather(const CocoStore& st, const int64_t* dt_off, int64_t ND, double* dt_kp, double* dt_score, int* dt_image,
                              hipStream_t s) {
    if (ND < 1) return hipSuccess;
    const int64_t want = (ND + kEvalThreads / 64 - 1) / (kEvalThreads / 64);
    hipLaunchKernelGGL(coco_gather_kernel, dim3((unsigned)(want < 4096 ? want : 4096)), dim3(kEvalThreads), 0, s, st, dt_off, ND, dt_kp, dt_score,
                       dt_image);
    return hipGetLastError();
}

}  // namespace lwp
