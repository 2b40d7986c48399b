// Internal declarations shared by the host graph code, the HIP kernels and the C-ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include <cstdio>
#include <string>
#include <vector>

#include "../../include/lwpose.h"
#include "jpeg_batch.h"

namespace lwp {

// ------------------------------------------------------------------ parameter table
struct ParamSpec {
    std::string key;
    int64_t shape[4];
    int ndim;
    int role;
};
std::vector<ParamSpec> param_table(int nref, int C, int NH, int NP);

// ------------------------------------------------------------------ layer graph
enum LayerKind { L_STEM = 0, L_DW = 1, L_GEMM = 2, L_DWPW = 3 };
enum Act { ACT_NONE = 0, ACT_RELU = 1, ACT_ELU = 2 };
enum KClass { KC_STEM = 0, KC_DW = 1, KC_PW = 2, KC_C3 = 3, KC_POST = 4, KC_OTHER = 5, KC_COUNT = 6 };

struct BufRef {      // a channel window of an NHWC activation buffer
    int buf = -1;    // index into Graph::bufs
    int coff = 0;    // first channel
    int ld = 0;      // row stride (channels per pixel) the layer addresses the buffer with
};

struct WBlock {              // one source conv of a merged 1x1 layer: W[out_off + o][in_off + i] = conv.weight[o][i]
    std::string conv_key;
    int out_off, in_off, cout, cin;
};

struct Layer {
    int kind = L_GEMM;
    std::string name;          // e.g. "model.3.pw"
    std::string conv_key;      // state_dict prefix of the conv ("model.3.3")
    std::string bn_key;        // state_dict prefix of the BN ("" = none)
    bool has_bias = false;
    int cin = 0, cout = 0, ks = 1, stride = 1, dil = 1, act = ACT_NONE;
    BufRef src, dst, res;      // res.buf < 0: no residual
    int out_index = -1;        // >= 0: this layer also produces stage output #out_index (NCHW)
    int out_index2 = -1, out_split = 0;   // merged heads: channels >= out_split belong to stage output #out_index2
    std::vector<WBlock> blocks;           // non-empty: weight matrix assembled from these convs (zeros elsewhere)
    int64_t macs_per_pixel = 0;           // algorithmic multiply-adds per output pixel (zero blocks not counted)
    int fuse = LWP_MARK_NONE;             // what the layer may share a launch with (LWP_MARK_*): set once by build_graph
    // packed weights (float offsets into the blob)
    size_t w_off = 0, b_off = 0;
    int cin_pad = 0, cout_pad = 0;
    // L_DWPW: the pointwise half (conv_key/bn_key/act/stride/dil above describe the depthwise half)
    std::string conv2_key, bn2_key;
    int act2 = ACT_NONE;
    size_t w2_off = 0, b2_off = 0;
};

struct BufSpec {
    int level;      // spatial level: 1 = H/2, 2 = H/4, 3 = H/8
    int channels;   // capacity in channels per pixel (layers may address it with a smaller ld)
    bool has_pad = false;   // some channels are never written but read with zero weights (the concat buffer): keep them finite
};

struct Graph {
    int nref, C, NH, NP;
    std::vector<BufSpec> bufs;
    std::vector<Layer> layers;
    size_t blob_floats = 0;
    int cat_buf = -1;          // the [feat | heat | paf | pad] buffer
    int cat_channels = 0;
    int dtype = LWP_F32;       // storage / MFMA dtype of the conv stack (weights packed accordingly): LWP_F32, LWP_BF16, LWP_F16
};
Graph build_graph(int nref, int C, int NH, int NP, bool fuse_dwpw, int dtype, bool merge_heads = true);

// The retaining buffer plan of the stages (lwp_train_forward): the SAME layer list, but from cpm.conv's output onward every
// layer writes a buffer of its own, and every stage has its own [feat | heat | paf | pad] concat buffer (cats[s]: stage s's
// heads write its heat / PAF window, refinement stage s + 1 reads it).  Buffer indices below Graph::bufs.size() are the
// graph's own buffers; index Graph::bufs.size() + i is train buffer i (all at level 3).
//
// Scope LWP_TRAIN_CPM moves the cut from cpm.conv to the layer in front of cpm.align (the backbone's last layer, whose output
// is the cpm's input): that layer and every cpm layer write buffers of their own too.  Two cpm tensors never leave a fused
// launch and get a retained copy from a second launch (enqueue_forward): the depthwise output of an L_DWPW block
// (dw_copy[i]: a buffer for a stand-alone launch_dw on the block's input) and the pointwise output of the block that adds
// the residual `a` in its epilogue (nores_copy[i]: a buffer for the same launch without the residual).
//
// Scope LWP_TRAIN_ALL moves the cut to the network input: every backbone layer writes a buffer of its own at its own level
// (BufSpec::level; the train buffers of the narrower scopes are all at level 3), and a fused backbone block gets a dw_copy too.
struct TrainPlan {
    std::vector<Layer> layers;     // Graph::layers with src / dst / res re-pointed
    std::vector<BufSpec> bufs;     // the train buffers
    std::vector<int> cats;         // nref + 1 concat buffers (plan indices)
    int cpm_conv = -1;             // index of cpm.conv
    int cpm_in = -1;               // index of the layer in front of cpm.align (the backbone's last layer: its output is the cpm's input)
    int cut = -1;                  // layers before it run on the graph's own plan and retain nothing; the layers behind it have a
                                   // backward.  LWP_TRAIN_STAGES: cpm.conv; LWP_TRAIN_CPM: cpm_in; LWP_TRAIN_ALL: -1 (every layer
                                   // has a backward: the cut is the network input)
    std::vector<int> dw_copy, nores_copy;   // per layer: plan buffer index, -1: none
    // per train buffer: does it have a gradient buffer?  GRAD_NEVER: a no-residual copy (only its values are read, as the
    // ELU output); GRAD_ON_DEMAND: the cpm's 512-channel input, whose gradient exists only when lwp_train_backward is asked for it
    enum { GRAD_ALWAYS = 0, GRAD_NEVER = 1, GRAD_ON_DEMAND = 2 };
    std::vector<char> grad_mode;
};
TrainPlan build_train_plan(const Graph& g, int scope = LWP_TRAIN_STAGES);
// f32 -> IEEE binary16 / bfloat16 bits, round to nearest even (fp16: subnormals exact, overflow -> inf, NaN stays NaN)
uint16_t f32_to_f16_rne(float f);
uint16_t f32_to_bf16_rne(float f);

struct HostTensor {
    const void* ptr;
    int64_t shape[4];
    int ndim;
};
// folds BN, packs into `blob` (size g.blob_floats); returns "" or an error message
// (LWP_F16: also when a folded weight is beyond the fp16 range, |w| > 65504 — it would be stored as inf)
std::string pack_weights(const Graph& g, const std::vector<std::string>& names,
                         const std::vector<HostTensor>& tensors, std::vector<float>& blob);

// ------------------------------------------------------------------ A/B and experiment switches
// Read from the environment ONCE PER HANDLE (lwp_create) and handed to the launchers through their parameter structs: a
// function-local `static getenv` would freeze whatever value the first launch of the process happened to see, so a test that
// toggles a switch between two engines would compare a kernel with itself.  0 / -1 = "not set": the launcher's own heuristic.
struct Tuning {
    int stem_ty = 0, stem_wl = -1, stem_debug = 0;                 // LWP_STEM_TY, LWP_STEM_WL, LWP_STEM_DEBUG
    int dw_tiled = -1, dw_cc = 0, dw_ph = 0;                       // LWP_DW_TILED (0 never | 1 always), LWP_DW_CC, LWP_DW_PH
    int dw_px = 0;                                                 // LWP_DW_PX (tests: 1 | 2 output pixels per thread of the per-thread depthwise kernel at every size)
    int gemm_wp = -1;                                              // LWP_GEMM_WP (-1 unset, else first digit)
    int gemm_debug = 0;                                            // LWP_GEMM_DEBUG (LWP_ABLATION builds: gemm_ar_kernel without 1 A staging, 2 weight requests, 4 MFMAs, 8 reduction + epilogue)
    bool has_c3 = false, has_pw = false; int c3[3] = {0, 0, 0}, pw[3] = {0, 0, 0};   // LWP_GEMM_C3 / LWP_GEMM_PW = "BM,BN,KS"
    int dwpw_bm = 0, dwpw_nw = 0, dwpw_debug = 0, dwpwh_debug = 0; // LWP_DWPW_BM, LWP_DWPW_NW, LWP_DWPW_DEBUG, LWP_DWPWH_DEBUG
    int dwpw_pipe = -1;                                            // LWP_DWPW_PIPE (f32 software-pipelined 512-output fused kernel: 0 off, 1 forced)
    int dwpw_lean = -1;                                            // LWP_DWPW_LEAN (f32 two-phase fused kernel <16,16>: 0 the classic phase 1, 1 the row-stepped one in 80 VGPRs; unset: 1)
    int dwpw_tiled_wgs = 0;                                        // LWP_DWPW_TILED_WGS (experiments: persistent workgroups per CU)
    int dwpw_tiled = -1;                                           // LWP_DWPW_TILED (front blocks, LDS-tiled fused kernel: 0 off, 1 forced)
    int dwpw_pp_grid = 0;                                          // LWP_DWPW_PP_GRID (tests: persistent grid size, to walk several rounds at small M)
    int dwpw_pp = -1;                                              // LWP_DWPW_PP (bf16 two-half-tile fused kernel: 0 off, 1 forced)
    int heads_rm = 0;                                              // LWP_HEADS_RM
    int gemmh_fold = -1;                                           // LWP_GEMMH_FOLD (0: never fold the next 1x1 into the 3x3's epilogue)
    int gemmh_persist = -1, gemmh_ar_off = 0, gemmh_ar_force = 0, gemmh_debug = 0;   // LWP_GEMMH_PERSIST, LWP_GEMMH_AR=0, LWP_GEMMH_AR_FORCE
    bool has_gemmh_ar = false, has_gemmh = false; int gemmh_ar[4] = {0, 0, 0, 0}, gemmh[4] = {0, 0, 0, 0};   // LWP_GEMMH_AR / LWP_GEMMH = "a,b,c,d"
    int upsample_tiled = -1;                                       // LWP_UPSAMPLE_TILED
    int max_frames_per_pass = 0;                                   // LWP_MAX_FRAMES_PER_PASS (tests: split batches as if the 2 GiB limit were reached earlier)
    int peak_tile = -1, pair_form = -1;                            // LWP_PEAK_TILE (find_peaks tile 0..3), LWP_PAIR_FORM (score_pairs variant)
    int dwpw_lds_pad_kb = 0;                                       // LWP_DWPW_LDS_PAD (KB of unused LDS per workgroup of the bf16 fused blocks: occupancy experiments)
    int host_fetch_dma = -1;                                       // LWP_HOST_FETCH_DMA ("1": host frames by hipMemcpyAsync instead of the fetch kernel)
    int ms_tx = 0;                                                 // LWP_MS_TX (8..40: tile width of the fused multi-scale kernel; 0 = the geometry's plan)
    int ms_vec = -1;                                               // LWP_MS_VEC ("0": the scalar fused multi-scale kernel)
    int ms_fused = -1;                                             // LWP_MS_FUSED ("0": multi-scale step as up-sample + resize kernels)
    int heads_debug = 0;                                           // LWP_HEADS_DEBUG (LWP_ABLATION builds: heads_f32_kernel<8> without 1 pixel-row loads, 2 weight requests, 4 MFMAs, 8 reduction + epilogue)
    int heads_f32_lds = -1;                                        // LWP_HEADS_F32_LDS ("0": the f32 stage heads above 4096 pixels as two GEMMs)
    int post_nchw = -1;                                            // LWP_POST_NCHW (f32: "0" = grouping reads the NHWC concat buffer in place)
    int heads_f32_max_m = 0;                                       // LWP_HEADS_F32_MAXM (tests: force the fused fp32 head pair at larger M)
    int fuse_dwpw = -1, merge_heads = -1, fuse_heads = -1;         // LWP_FUSE_DWPW, LWP_MERGE_HEADS, LWP_FUSE_HEADS ("0": depthwise + pointwise / heat + PAF heads / a stage's head pair as separate launches)
    int pre_batch_vec = -1;                                        // LWP_PRE_BATCH_VEC ("1": the batched uint8 pre-processing with four pixels per thread; default: one thread per pixel)
    int post_stream = -1, post_generic = -1;                       // LWP_POST_STREAM ("0": a pipeline slot's grouping follows the network on the main stream), LWP_POST_GENERIC ("1": the generic grouping kernels under the default skeleton too)
};
Tuning tuning_from_env();
const Tuning& default_tuning();
#ifdef __HIPCC__
// ReLU of the conv kernels.  Not fmaxf: that returns its other operand for a NaN, so the NaN of an inf x 0 behind an fp16
// overflow would read as 0 in the next layer; this keeps it, as torch's ReLU does (tests/exact_cases.py, the f16ovf fixtures).
__device__ __forceinline__ float relu_f(float v) { return v < 0.f ? 0.f : v; }
#endif
// name of the kernel variant a launcher picked, written when the caller supplies a buffer (debug / profiling entry points)
constexpr int kVariantCap = 64;
#define LWP_VARIANT(p, ...) do { if ((p).variant) snprintf((p).variant, lwp::kVariantCap, __VA_ARGS__); } while (0)

// ------------------------------------------------------------------ kernel launch parameters
struct StemParams {       // (__restrict__: the weights stay scalar loads although the kernel loops over tiles and stores in between)
    const float* __restrict__ in;     // N x 3 x H x W
    const float* __restrict__ w;      // [27][32]  (ky, kx, ci) major, oc minor
    const float* __restrict__ bias;   // [32]
    float* __restrict__ out;          // N x Ho x Wo x 32
    int N, H, W, Ho, Wo;
    int f16 = 0;                    // 16-bit path: output element type fp16 (else bf16); sits in the padding before `zeros`
    const float* zeros = nullptr;   // >= 16 bytes of zeros (source of out-of-image quads)
    const Tuning* tune = nullptr; char* variant = nullptr;
};
struct DwParams {
    const float* in; int in_ld;      // NHWC, row stride in_ld
    const float* w;                  // [9][C]
    const float* bias;               // [C]
    float* out; int out_ld;
    int N, Hi, Wi, Ho, Wo, C, stride, dil, act;
    const Tuning* tune = nullptr; char* variant = nullptr;
};
struct GemmParams {
    const float* in; int in_ld;      // window start already applied to the pointer
    int f16 = 0;                     // 16-bit path: element type fp16 (else bf16).  Here, and in the other structs, the field fills
                                     // padding in front of the next pointer: the kernels' argument layout is that of the bf16 path
    const float* w;                  // [taps][cout_pad][cin_pad]
    const float* wf = nullptr;       // fp32 only: the same weights in fragment order [tap][k-step][32-ch tile][4][64][4]
    const float* bias;               // [cout_pad]
    float* out; int out_ld;
    const float* res; int res_ld;    // may be null
    float* out_nchw;                 // may be null: N x cout x H x W  (x out_split channels when out_split > 0)
    float* out_nchw2 = nullptr;      // merged heads: channels >= out_split, N x (cout - out_split) x H x W
    int out_split = 0;
    const float* zeros;              // >= 16 bytes of zeros (source of out-of-image taps)
    int N, H, W, cin_pad, cout, cout_pad, ks, dil, act;
    int debug = 0;                   // reserved for timing experiments
    const Tuning* tune = nullptr; char* variant = nullptr;
    // optional second conv fused into the epilogue (bf16 window-resident kernel only): out2 = act2(W2 . bf16(out) + b2), a 1x1 conv
    // 128 -> 128 over the tile the kernel has just produced; `out` itself is then NOT written.  *fused2 reports whether the
    // launcher took it (else the caller launches the second layer itself).
    const void* w2 = nullptr; const float* bias2 = nullptr; void* out2 = nullptr; int out2_ld = 0, act2 = 0;
    bool* fused2 = nullptr;
};
struct DwPwParams {
    const float* in; int in_ld;          // depthwise input, NHWC
    int f16 = 0;                         // 16-bit path: element type fp16 (else bf16)
    const float* dw_w;                   // [9][C] followed by [C] bias (contiguous)
    const float* pw_w;                   // fragment-packed pointwise weights [C/32][cout/32][4][64][4]
    const float* pw_b;                   // [cout]
    float* out; int out_ld;
    const float* res; int res_ld;        // may be null
    const float* zeros;
    int N, Hi, Wi, Ho, Wo, C, cout, stride, dil, act_dw, act_pw;
    int debug = 0;                       // ablation switches (LWP_DWPW_DEBUG): 1 skip phase 1, 2 skip B loads, 4 skip MFMAs, 8 no XCD tile remap
    const Tuning* tune = nullptr; char* variant = nullptr;
};
bool dwpw_supported(int C, int cout);
hipError_t launch_dwpw(const DwPwParams& p, hipStream_t s);
// LDS-tiled form of the front blocks at large batch (net_kernels_tiled.hip); *used = false: not applicable, the caller goes on
hipError_t try_dwpw_tiled_f32(const DwPwParams& p, hipStream_t s, bool* used);
hipError_t try_dwpw_tiled_bf16(const DwPwParams& p, hipStream_t s, bool* used);
// 16-bit storage path (net_kernels_bf16.hip): same parameter structs, activation / packed-weight pointers are bf16, or fp16
// when the struct's `f16` is set (LWP_F16: every launcher below and the LDS-tiled fused blocks instantiate their kernels for
// either type)
hipError_t launch_stem_bf16(const StemParams& p, hipStream_t s);
hipError_t launch_dwpw_bf16(const DwPwParams& p, hipStream_t s);
hipError_t launch_gemm_bf16(const GemmParams& p, hipStream_t s);
// a stage's head pair (with_mobilenet.py:32-45, 1x1 C -> hidden, ReLU, 1x1 hidden -> NH + NP) as ONE kernel: the hidden tensor
// (247 MB at batch 32 for the initial stage) never leaves the CU.  Weights in the plain [cout_pad][cin_pad] bf16 layout.
struct HeadsParams {
    const void* in; int in_ld;           // [M][128] bf16 / fp16
    int f16 = 0;                         // element type fp16 (else bf16)
    const void* w0; const float* b0;     // [hidden][128] bf16, [hidden]
    const float* w0f = nullptr;          // fp32: w0 again in the layer's fragment-order copy ([k-step 4][32-row tile][s 4][lane 64][4])
    const void* w1; const float* b1;     // [64][hidden] bf16 (rows >= cout are zero), [64]
    void* out; int out_ld;               // bf16 NHWC window (the concat buffer at the heat/PAF channels)
    float* out_nchw; float* out_nchw2;   // may be null: stage outputs, split at out_split
    int out_split, N, H, W, hidden, cout;
    const Tuning* tune = nullptr; char* variant = nullptr;
};
bool heads_bf16_supported(int cin_pad, int hidden, int cout_pad);
hipError_t launch_heads_bf16(const HeadsParams& p, hipStream_t s);
// fp32 form for M <= 4096 (batch 1: 3772 pixels): a workgroup owns 32 pixels of ONE head of a merged pair, that head's hidden
// half split over the waves, fixed-order reduction of the partial outputs.  Pointers are f32 ([hidden][128], [64][hidden], NHWC f32 window).
bool heads_f32_supported(int cin_pad, int hidden, int cout_pad, int64_t M, const Tuning* tune = nullptr);
hipError_t launch_heads_f32(const HeadsParams& p, hipStream_t s);
hipError_t launch_nchw_from_nhwc_bf16(const void* src, int src_ld, float* dst, int N, int HW, int C, hipStream_t s, bool f16 = false);
hipError_t launch_stem(const StemParams& p, hipStream_t s);
hipError_t launch_dw(const DwParams& p, hipStream_t s);
hipError_t launch_gemm(const GemmParams& p, hipStream_t s);

// ------------------------------------------------------------------ post-processing
struct MapView {          // a float32 map set addressed as base[n*ns + y*ys + x*xs + c*cs]
    const float* base;
    int64_t ns, ys, xs, cs;
    int h, w;             // size of the stored grid
};
struct PostCaps { int max_peaks = 2048, max_kpts = 128, max_conn = 4096, max_entries = 256; };

// The grouping tables (modules/keypoints.py:5-8) and group_keypoints' options (:51).  K key-point types, L limbs, pose rows of
// E doubles.  The default (COCO: 18 / 19 / 20, min_paf_score 0.05) runs the specialised kernels; any other skeleton, or
// LWP_POST_GENERIC=1, runs the generic forms, which read the tables at run time.
constexpr int kMaxSkelTypes = 64, kMaxSkelLimbs = 320, kMaxEntrySize = 256;
struct Skeleton {
    int K = 18, L = 19, E = 20;
    double min_paf = 0.05;
    std::vector<int> kpt, paf;      // [L][2] each
    bool is_default = true;
};
Skeleton default_skeleton();

struct PostWorkspace {    // device buffers, sized for (N frames, caps, skeleton)
    int N = 0;
    PostCaps caps;
    int K = 18, L = 19, E = 20;     // key-point types, limbs, doubles per pose row (18 / 19 / 20 by default)
    int generic = 0;                // 1: the generic kernels (runtime tables below) instead of the COCO-specialised ones
    double min_paf = 0.05;
    const int* limbs = nullptr;     // [L][4]: type a, type b, PAF channel x, PAF channel y (generic kernels only)
    int* peak_count = nullptr;      // [N*K]
    uint32_t* peak_key = nullptr;   // [N*K*max_peaks]  (x << 16 | y)
    float* peak_val = nullptr;      // [N*K*max_peaks]
    int* kpt_count = nullptr;       // [N*K]
    int* kpt_xy = nullptr;          // [N*K*max_kpts*2]
    float* kpt_score = nullptr;     // [N*K*max_kpts]
    int* conn_count = nullptr;      // [N*L]
    int* conn_ij = nullptr;         // [N*L*max_conn]   (i << 16 | j)
    double* conn_ratio = nullptr;   // [N*L*max_conn]
    unsigned long long* flags = nullptr;  // [N*4]  0: overflow bits (1 peaks, 2 kpts, 4 conns/entries),
                                          //        1: min order of a pair whose mid-point test failed,
                                          //        2: min order of a pair whose mid-point test passed
    int* sel_count = nullptr;       // [N*L]  connections picked by the greedy matching
    int* seen = nullptr;            // [N*(K+L)]  debug: peaks per type nms_kernel saw [K], candidates per limb match_kernel saw [L] (the counters themselves are re-armed by assemble_kernel)
    int* sel_ij = nullptr;          // [N*L*max_kpts]
    double* sel_r = nullptr;        // [N*L*max_kpts]
    float* sel_sa = nullptr;        // [N*L*max_kpts] score of the connection's first key-point
    float* sel_sb = nullptr;        // [N*L*max_kpts] score of its second key-point
    double* entries_work = nullptr; // [N*max_entries*E] scratch when the entries do not fit LDS
    double* entries = nullptr;      // [N*max_entries*E]
    int* n_entries = nullptr;       // [N]
    double* kpts_out = nullptr;     // [N*K*max_kpts*4]
    void* result_block = nullptr;   // flags, kpts_out, entries, kpt_count, n_entries (+ the tail): one allocation, laid out by result_layout()
    // pose tail (lwp_set_tracking mode != 0): one more section at the END of the result block, so the offsets above never move.
    // P = caps.max_entries pose slots per frame.  All null / 0 with the tail off.
    int tail = 0;                   // the tracking mode the block was laid out for (0: no tail section)
    int* t_n = nullptr;             // [N]        poses of the frame
    unsigned* t_near = nullptr;     // [N]        similarity decisions whose q lay within 1e-12 (relative) of -ln(similarity_threshold)
    int* t_last = nullptr;          // [N]        the lane's id counter after the frame (last id given out)
    int* t_ids = nullptr;           // [N*P]      -1 in mode 1
    int* t_bbox = nullptr;          // [N*P*4]
    int* t_kp = nullptr;            // [N*P*K*2]  -1 = key-point not found
    double* t_conf = nullptr;       // [N*P]
};

// THE byte layout of the result block, on the device and in the pinned host copy alike: N frames of every section, back to
// back in this order; the pose tail, 16-byte aligned, is appended so that the leading offsets never move.  A section of frame
// f starts at off + f * stride.  With the tail off its sections are empty and `bytes` ends behind n_entries.
struct ResultLayout {
    struct Sec { size_t off, stride; };              // bytes: start of frame 0, distance between frames
    Sec flags, kpts_out, entries, kpt_count, n_entries;
    Sec t_conf, t_bbox, t_kp, t_ids, t_n, t_near, t_last;
    size_t tail_off, bytes;
};
inline ResultLayout result_layout(int N, int K, int E, const PostCaps& c, bool tail) {
    ResultLayout l{};
    size_t q = 0;
    auto sec = [&](ResultLayout::Sec& s, size_t stride) { s.off = q; s.stride = stride; q += (size_t)N * stride; };
    const size_t P = (size_t)c.max_entries;          // pose slots per frame
    sec(l.flags, 4 * 8); sec(l.kpts_out, (size_t)K * c.max_kpts * 4 * 8); sec(l.entries, P * E * 8); sec(l.kpt_count, (size_t)K * 4); sec(l.n_entries, 4);
    l.bytes = q;
    l.tail_off = (q + 15) & ~(size_t)15;
    if (!tail) return l;
    q = l.tail_off;
    sec(l.t_conf, P * 8); sec(l.t_bbox, P * 4 * 4); sec(l.t_kp, P * K * 2 * 4); sec(l.t_ids, P * 4); sec(l.t_n, 4); sec(l.t_near, 4); sec(l.t_last, 4);
    l.bytes = q;
    return l;
}
inline ResultLayout result_layout(const PostWorkspace& w) { return result_layout(w.N, w.K, w.E, w.caps, w.tail != 0); }

// ---- pose tail (demo.py:101-118, modules/pose.py:65-118): tracking state of the handle's lanes, on the device
constexpr int kTailMaxPoses = 256;  // pose slots per frame the greedy pass holds in registers (4 per lane of one wave)
struct TailState {
    int lanes = 0, P = 0, K = 0;
    int4* hdr = nullptr;            // [lanes]  x: next id, y: parity (which of the two buffers holds the previous frame), z: poses in it
    int* kp = nullptr;              // [lanes][2][P][K][2]  key-points after smoothing
    int* bbox = nullptr;            // [lanes][2][P][4]
    int* ids = nullptr;             // [lanes][2][P]
    int* f_xprev = nullptr;         // [lanes][2][P][K][2]  1-Euro filter of each coordinate: last raw input,
    int* f_init = nullptr;          //                      0 = never called,
    double* f_dx = nullptr;         //                      low-passed derivative,
    double* f_x = nullptr;          //                      low-passed value
    unsigned char* sim = nullptr;   // [lanes][P][P]  similar key-points of (current pose, previous pose)
    const float* vars = nullptr;    // [K]  (2 sigma)^2 in float32
};
struct TailParams {
    int mode = 0;                   // 0 off, 1 pose rows only, 2 lanes (frame f -> lane f), 3 sequence (all frames -> lane 0, in order)
    int match_threshold = 3, smooth = 0;
    int stride = 8, ratio = 4, pad_top = 0, pad_left = 0;
    double scale = 1.0;
    double qmax = 0.6931471805599453;   // -ln(similarity_threshold), computed once on the host
};
// un-map + pose rows + confidence + bounding box of frames [0, N); from_rows != 0: the rows are already in ws.t_kp / t_conf / t_n
hipError_t launch_tail_rows(int N, PostWorkspace& ws, const TailParams& p, int from_rows, hipStream_t s);
// one tracking step per frame: lanes mode frame f -> lane lane0 + f (one workgroup each); sequence mode all N frames -> lane lane0, in order
hipError_t launch_tail_track(int N, PostWorkspace& ws, const TailState& st, const TailParams& p, int lane0, hipStream_t s);
hipError_t launch_tail_reset(const TailState& st, int lane0, int count, int next_id, hipStream_t s);

// ---- pose overlay (demo.py:119-124): skeletons, blend and boxes of N uint8 frames, from pose rows that live on the device
struct OverlayParams {
    const unsigned char* src;       // N x H x W x 3, never written
    unsigned char* out;             // N x H x W x 3, must not overlap src
    int N, H, W;
    const int* n_poses;             // [N]  (t_n of a result block, or rows the caller supplied)
    const int* kp;                  // frame f, pose e, type k: kp[f * kp_stride + (e * K + k) * 2 + {0, 1}], x == -1: missing
    const int* bbox;                // frame f, pose e: bbox[f * bbox_stride + e * 4 + {0..3}] = x, y, w, h
    int64_t kp_stride, bbox_stride; // ints per frame
    int P, K;                       // pose slots per frame (a frame's pose count is clamped to it), key-point types
    const int* limbs;               // [L][4] as PostWorkspace::limbs; the first n_limbs rows are drawn
    int n_limbs;
    unsigned char color[3], box_color[3];
    int boxes;
};
// three launches on `s`: the full-frame copy, one wave per (frame, pose slot, limb) for the stamps, one workgroup per
// (frame, pose slot) for the boxes; `poses` bounds the pose slots the grid covers (<= P)
hipError_t launch_overlay(const OverlayParams& p, int poses, hipStream_t s);

// ---- training targets and loss (train_kernels.hip; datasets/coco.py:48,71-159, modules/loss.py)
constexpr int kTrainChunk = 8;      // persons of a frame staged in LDS at a time
constexpr int kLossMaxOuts = 16;    // stage tensors one loss launch reads (more: further launches over the same targets)
constexpr int kLossMaxBlocks = 1024;
struct TrainTargetsParams {
    const double* kpts;             // N x Pmax x K x 3: x, y, visibility
    const int* n_persons;           // [N], clamped to 0..Pmax
    int Pmax, K, L;
    const int* limbs;               // [L][4] as PostWorkspace::limbs
    int h, w, stride;               // map size, H // stride x W // stride
    double sigma, thickness;
    float* keypoint_maps;           // N x (K + 1) x h x w
    float* paf_maps;                // N x 2L x h x w
};
hipError_t launch_train_targets(const TrainTargetsParams& p, int N, hipStream_t s);
hipError_t launch_mask_downsample(const float* src, int N, int H, int W, int stride, float* dst, hipStream_t s);
// ---- training augmentation (augment_kernels.hip; datasets/transformations.py): one thread per crop pixel, then the small mask;
// plans_device: N records whose image / mask pointers are device addresses
hipError_t launch_augment(const lwp_augment_plan* plans_device, int N, int crop_h, int crop_w, int stride, float* image,
                          unsigned char* mask, float* mask_small, hipStream_t s);
// ---- crowd masks (crowd_kernels.hip; datasets/coco.py:17-21): the float32 loss masks of a batch from uncompressed RLEs
constexpr int kCrowdRunsLds = 4096;   // run ends of one image (all its segmentations) a workgroup stages in LDS; more: searched in global memory
constexpr int kCrowdStrip = 8;        // rows of one column a thread renders: consecutive positions of the column-major runs
struct CrowdImage {
    unsigned seg0, n_seg;             // its segmentations: seg_off[seg0] .. seg_off[seg0 + n_seg] bound their run ends
    int h, w;
    long long out;                    // float offset of its h x w row-major mask
};
struct CrowdLaunch {
    const unsigned* ends;             // running sums of the counts, per segmentation
    const unsigned* seg_off;          // [S + 1] first run end of a segmentation
    const CrowdImage* images;         // the images that are rendered
    float* masks;
    int n_images, max_h, max_w;
};
hipError_t launch_crowd_masks(const CrowdLaunch& c, hipStream_t s);
// ---- JPEG decode, device half (jpeg_kernels.hip; libjpeg's default path: jidctint.c, fancy up-sampling, jdcolor.c): stage A
// turns the coefficient blocks of a batch into block-padded uint8 component planes, stage B up-samples, converts and stores BGR.
// The records of this and the next two sections, and the constants their filling needs, are jpeg_batch.h's
struct JpegLaunch {
    const int16_t* coef; const uint16_t* qtables;
    const JpegPlane* planes; const unsigned* plane_block0;    // [n_planes] records; [n_planes + 1] their block0, then the total
    const JpegImage* images; const unsigned* image_unit0;     // [n_images]; [n_images + 1]
    unsigned char* workspace;
    int n_planes, n_images;
    unsigned total_blocks, total_units;
};
hipError_t launch_jpeg_idct(const JpegLaunch& j, hipStream_t s);
hipError_t launch_jpeg_color(const JpegLaunch& j, hipStream_t s);
// ---- JPEG entropy decode on the device (jpeg_entropy_kernels.hip): fills JpegLaunch::coef from the un-stuffed scan
// bytes, segments and flattened tables that jpeg_scan_segments (jpeg_host.h) left.  One lane owns one subsequence of
// subseq_bytes bytes of one segment; a workgroup takes kJpegEntropyGroup consecutive subsequences of ONE file.
struct JpegEntropyLaunch {
    const unsigned* words; unsigned n_words;          // the byte area as dwords
    const JpegHuffFlat* tables;                       // [n_files][kJpegHuffPerFile]
    const JpegEntFile* files; const unsigned* file_wg0;   // [n_files]; [n_files + 1] first workgroups, then the total
    const JpegEntSeg* segs; const unsigned* seg_sub0;     // [n_segs]; [n_segs + 1] first subsequences, then the total
    uint2* rec;                                       // [n_subs] x: exit bit position, y: block starts << 16 | block in MCU << 8 | k
    unsigned* subpos;                                 // [n_subs] block starts in front of the subsequence, counted from the file's first
    uint2* wg_entry; unsigned* wg_dirty;              // [n_wgs] the entry a workgroup's first lane last used; whether it changed
    int16_t* coef;
    int* status;                                      // [n_files] non-zero: refused; then [2] sync rounds taken (in a workgroup, across)
    int n_files; unsigned n_segs, n_subs, n_wgs;
    int subseq_bytes;
};
hipError_t launch_jpeg_entropy(const JpegEntropyLaunch& e, hipStream_t s);
// ---- JPEG encode on the device (jpeg_encode_kernels.hip; libjpeg's default compression path: jccolor.c, box
// down-sampling, jfdctint.c, Annex K's Huffman tables).  Six stages over a whole batch of frames of mixed sizes:
//   A  colour, down-sampling, edges, forward DCT, quantisation -> the coefficient layout of jpeg_host.h (8 lanes a block)
//   B  the bit count of every block, in stream (MCU) order (one lane a block)
//   C  per image, the scan of the counts into bit offsets, every restart interval starting on a byte (one workgroup an image)
//   D  the codes of every block at its offset, OR-ed into the zeroed un-stuffed scan (one lane a block)
//   E  per image, the 0xFF bytes in front of every chunk of the un-stuffed scan (one workgroup an image)
//   F  the stuffed scan: FF 00 for FF, RSTn between the intervals (one lane a chunk)
struct JpegEncLaunch {
    const JpegEncImage* images;               // [n_images]
    const unsigned* block_start;              // [n_images + 1] block0 of every image, then the total
    const unsigned* chunk_start;              // [n_images + 1]
    const uint16_t* qtables;                  // [2][64] natural order
    const unsigned* huff;                     // JpegEncHuff (jpeg_encode_host.h) as words: dc[2][16], ac[2][256]
    int16_t* coef;                            // [total_blocks][64]
    unsigned* bits; unsigned* offs;           // [total_blocks] bit count; bit offset from the image's un-stuffed scan
    unsigned* istart;                         // [intervals] first un-stuffed byte of every restart interval
    unsigned* ulen; unsigned* slen;           // [n_images] un-stuffed and stuffed bytes of the scan
    unsigned* ffbase;                         // [total_chunks] 0xFF bytes of the image in front of the chunk
    unsigned char* workspace;
    int n_images;
    unsigned total_blocks, total_chunks;
};
hipError_t launch_jpeg_enc_dct(const JpegEncLaunch& e, hipStream_t s);
hipError_t launch_jpeg_enc_lengths(const JpegEncLaunch& e, hipStream_t s);
hipError_t launch_jpeg_enc_offsets(const JpegEncLaunch& e, hipStream_t s);
hipError_t launch_jpeg_enc_write(const JpegEncLaunch& e, hipStream_t s);
hipError_t launch_jpeg_enc_stuff_scan(const JpegEncLaunch& e, hipStream_t s);
hipError_t launch_jpeg_enc_stuff(const JpegEncLaunch& e, hipStream_t s);
// ---- COCO key-point evaluation (eval_kernels.hip; COCOeval with iouType 'keypoints' and its default parameters): float64
constexpr int kEvalK = 17;            // key-points of a person
constexpr int kEvalMaxDets = 20;      // detections of an image that count (maxDets)
constexpr int kEvalT = 10, kEvalR = 101, kEvalA = 3;      // IoU thresholds, recall thresholds, area ranges
constexpr int kEvalAT = kEvalA * kEvalT;                  // independent matchings of an image; (range, threshold) = (at / 10, at % 10)
constexpr int kEvalScanChunk = 256;   // detections one step of the accumulate kernel's scans covers (one per thread, then a carry)
struct CocoEvalParams {
    int n_images;
    int64_t NG, NS;                   // ground truths and selected detections (at most 20 an image) of the dataset
    // inputs, CSR over the images: detections [dt_off[i], dt_off[i + 1]), ground truths likewise
    const int64_t *dt_off, *gt_off;
    const int64_t *sel_off, *oks_off; // [n_images + 1]: first selected detection and first OKS entry of an image
    const double *dt_kp, *dt_score;   // [ND][17][3], [ND]
    const double *gt_kp, *gt_area, *gt_bbox;      // [NG][17][3], [NG], [NG][4]
    const int *gt_iscrowd, *gt_ignore;            // [NG]
    // per-image results
    int* sel_idx;                     // [NS] index within its image of the detection at each rank
    double* sel_score;                // [NS]
    double* oks;                      // per image [min(D, 20)][G], columns in input GT order
    unsigned char* gt_flag;           // [NG] bit 0: crowd, bit 1 + a: ignored in range a
    unsigned char* gt_m;              // [30][NG] matched so far (zeroed before the launch)
    unsigned char *dt_m, *dt_ig;      // [30][NS] matched / ignored
    int* npig_img;                    // [n_images][3] GTs not ignored per range
    // accumulate
    const unsigned int* perm;         // [NS] selected detections by descending score, stable
    unsigned long long* tpfp;         // [30][NS] inclusive counts: tp in the low, fp in the high 32 bits
    double* pr;                       // [30][NS] precision, then its reverse running maximum
    double *precision, *recall, *scores;          // [10][101][3], [10][3], [10][101][3]
    long long* npig;                  // [3]
    // COCOeval's default parameters, computed once on the host as NumPy does
    double vars[kEvalK], iou_thr[kEvalT], rec_thr[kEvalR], area_lo[kEvalA], area_hi[kEvalA];
};
void coco_eval_defaults(CocoEvalParams* p);
hipError_t launch_coco_match(const CocoEvalParams& p, hipStream_t s);
// the order of the accumulation: keys and values in, sorted out; tmp / tmp_bytes as coco_sort_temp_bytes says
hipError_t coco_sort_temp_bytes(int64_t NS, size_t* bytes);
hipError_t launch_coco_sort(const double* sel_score, int64_t NS, unsigned long long* keys, unsigned long long* keys_out,
                            unsigned int* vals, unsigned int* perm, void* tmp, size_t tmp_bytes, hipStream_t s);
hipError_t launch_coco_accumulate(const CocoEvalParams& p, hipStream_t s);
// ---- detection store (eval_kernels.hip; val.py:52-78,136-145): the detections of a validation run, kept on the device between
//      the grouping and the evaluation.  Rows lie in the order they were added; an image's rows are [start, start + count).
constexpr int kCocoTypes = 18, kCocoEntry = 20;       // key-point types and doubles per pose row of the default skeleton
enum CocoStatus { COCO_ST_OK = 0, COCO_ST_FLAGS = 1, COCO_ST_UNBOUND = 2, COCO_ST_ROWS = 3, COCO_ST_NONFINITE = 4 };
struct CocoStore {
    double* kp;                       // [row_cap][17][3]
    double* score;                    // [row_cap]
    int* image;                       // [row_cap] position of the row's image in ascending id order
    int* start;                       // [n_images]
    int* count;                       // [n_images] rows written (0: never added, or added without a pose)
    long long* ctl;                   // [4] 0: cursor (rows asked for; beyond row_cap nothing is written), 1: sticky CocoStatus,
                                      //     2: the image index it names, 3: its detail (the overflow bits of a frame)
    int row_cap, n_images;
};
struct CocoAppendParams {             // the result block enqueue_grouping leaves for N frames (ResultLayout, default skeleton)
    const unsigned long long* flags;  // [N][4]
    const double* kpts_out;           // [N][max_rows][4] rows in id order
    const double* entries;            // [N][max_entries][20]
    const int* n_entries;             // [N]
    const int* image_index;           // [N] device
    int N, max_entries, max_rows;
};
// one workgroup walks the N frames in order: no atomic decides a row's position
hipError_t launch_coco_append(const CocoStore& st, const CocoAppendParams& p, hipStream_t s);
// n ready-made rows of one image through the same cursor
hipError_t launch_coco_append_rows(const CocoStore& st, int image, int n, const double* kp, const double* score, hipStream_t s);
// dt_off [n_images + 1] (device) from the store's counts
hipError_t launch_coco_offsets(const CocoStore& st, int64_t* dt_off, hipStream_t s);
// the store in CSR order: destination row r of image i comes from start[i] + (r - dt_off[i]); rows [0, min(ND, dt_off[n_images]));
// dt_image may be null
hipError_t launch_coco_gather(const CocoStore& st, const int64_t* dt_off, int64_t ND, double* dt_kp, double* dt_score, int* dt_image,
                              hipStream_t s);

struct StageLossParams {
    const float* outs[kLossMaxOuts];   // even: N x CH x hw heat-map tensors, odd: N x CP x hw PAF tensors; null = skipped
    int S;
    const float* keypoint_maps;     // N x CH x hw (null when no even tensor is given)
    const float* paf_maps;          // N x CP x hw (null when no odd tensor is given)
    const float* mask;              // N x hw, broadcast over the channels
    int N, CH, CP, hw, batch;
    double* partials;               // [S][stage_loss_blocks(N, hw)]
};
int stage_loss_blocks(int N, int hw);
// losses: p.S doubles, device.  log (or null): p.S doubles that get losses[i] / divisor added; adds (or null): one counter, + 1
hipError_t launch_stage_losses(const StageLossParams& p, double* losses, hipStream_t s, double* log = nullptr, double divisor = 1.0,
                               int64_t* adds = nullptr);

// ---- stage backward (bwd_kernels.hip; train.py:99-103 differentiated): f32, NHWC activations and gradients
struct LossGradParams {
    const float* outs[kLossMaxOuts];   // NHWC windows of the stage tensors, even: heat-maps, odd: PAFs, row stride ld
    float* dst[kLossMaxOuts];          // NHWC gradient windows, row stride ld
    int S, ld;
    const float* keypoint_maps; const float* paf_maps; const float* mask;
    int N, CH, CP, hw;
    float scale;                       // loss_scale / batch_size
};
hipError_t launch_loss_grad(const LossGradParams& p, hipStream_t s);
// g = (y > res ? g : 0) over an M x C window (res null: y > 0): the ReLU of a layer whose retained output is y (= relu(z) + res)
hipError_t launch_relu_mask(float* g, int g_ld, const float* y, int y_ld, const float* res, int res_ld, int64_t M, int C, hipStream_t s);
// dst = (beta ? dst : 0) + src over an M x C window
hipError_t launch_grad_add(float* dst, int dst_ld, const float* src, int src_ld, int64_t M, int C, int beta, hipStream_t s);
struct DgradParams {
    const float* dz; int dz_ld;      // M x cout gradient of the layer's pre-activation output
    const float* w;                  // the forward blob's [taps][cout_pad][cin_pad]
    float* dx; int dx_ld;            // M x cin; channels >= acc_from are added to, the others overwritten
    int N, H, W, cout, cout_pad, cin, cin_pad, ks, dil, acc_from;
};
// lwp_set_backward_precision: the operand type of the two MFMA products (LWP_F32: the f32 kernels) and the power of two dZ is
// multiplied by in front of its rounding (the accumulator by its inverse)
struct BwdPrecision { int dtype = LWP_F32; float scale = 1.0f; };
hipError_t launch_dgrad(const DgradParams& p, hipStream_t s, BwdPrecision bp = BwdPrecision());
struct WgradParams {
    const float* dz; int dz_ld;      // M x cout
    const float* x; int x_ld;        // M x cin, the layer's retained input
    float* partial;                  // [splits][taps][co_pad][ci_pad] weight partials, then [splits][co_pad] bias partials
    int N, H, W, cout, cin, ks, dil;
    int splits, chunk;               // pixel ranges [z * chunk, (z + 1) * chunk), chunk a multiple of 16
    int no_bias;                     // != 0: a conv without bias (the cpm's pointwise layers): no bias row of workgroups, db not written
};
__host__ __device__ inline int wgrad_pad64(int v) { return (v + 63) / 64 * 64; }
void wgrad_plan(int64_t M, int cout, int cin, int ks, int* splits, int* chunk);
inline size_t wgrad_partial_floats(const WgradParams& p) {
    return (size_t)p.splits * wgrad_pad64(p.cout) * ((size_t)p.ks * p.ks * wgrad_pad64(p.cin) + 1);
}
hipError_t launch_wgrad(const WgradParams& p, hipStream_t s, BwdPrecision bp = BwdPrecision());
// fixed-order sum of the partials into OIHW dw [cout][cin][taps] and db [cout]; accumulate: added to what is there
hipError_t launch_wgrad_reduce(const WgradParams& p, float* dw, float* db, int accumulate, hipStream_t s);
// ---- depthwise backward: the ELU gradient of the cpm (with_mobilenet.py:7-21) and the gradients of a depthwise 3x3 with stride
//      1 | 2 and dilation 1 | 2, padding = dilation (the cpm's: 1, 1; the backbone's, with_mobilenet.py:94-104: all four).  C is a
//      multiple of 4, every row stride too, every pointer 16-byte aligned: a lane moves four consecutive channels of a pixel.
// g = g * (y > 0 ? 1 : y + 1) over an M x C window, y the retained ELU output (alpha = 1: elu'(z) = exp(z) = y + 1 for z <= 0)
hipError_t launch_elu_grad(float* g, int g_ld, const float* y, int y_ld, int64_t M, int C, hipStream_t s);
struct DwGradParams {
    const float* dz; int dz_ld;      // N Ho Wo x C gradient of the depthwise conv's pre-activation output
    const float* x; int x_ld;        // wgrad: the retained input, N H W x C
    const float* w;                  // dgrad: the forward blob's [9][C]
    float* dx; int dx_ld;            // dgrad: N H W x C; beta != 0: added to, else overwritten
    float* partial;                  // wgrad: [splits][rows][C], rows = 9 taps, or 10 with the sum of dZ behind them
    int N, H, W, Ho, Wo, C, stride, dil, beta;       // Ho = (H - 1) / stride + 1
    int splits, chunk;               // wgrad: ranges of output pixels [z * chunk, (z + 1) * chunk), chunk a multiple of 16
};
void dw_wgrad_plan(int64_t M, int C, int* splits, int* chunk);      // M = N Ho Wo
hipError_t launch_dw_dgrad(const DwGradParams& p, hipStream_t s);
// sum_dz: the partials carry a tenth row, the sum of dZ per channel (the folded bias gradient a BatchNorm chain rule needs);
// without it stride and dilation are 1 (the cpm's form, the one without BatchNorm)
hipError_t launch_dw_wgrad(const DwGradParams& p, bool sum_dz, hipStream_t s);
// fixed-order sum of the partials into the OIHW (C, 1, 3, 3) gradient and, where g is given, of their tenth row into g (C);
// accumulate: added to what is there
hipError_t launch_dw_wgrad_reduce(const DwGradParams& p, float* dw, float* g, int accumulate, hipStream_t s);
// ---- backbone backward (with_mobilenet.py:93-104): the stem's weight gradient, folded pointwise weights, BatchNorm chain rule
struct StemWgradParams {
    const float* dz; int dz_ld;      // N Ho Wo x 32 gradient of the stem's pre-activation output
    const float* x;                  // N x 3 x H x W, the input the stem kernel read
    float* partial;                  // [splits][28][32]: the 27 weight rows (ci, ky, kx), then the sum of dZ
    int N, H, W, Ho, Wo;
    int splits, chunk;               // ranges of output pixels (stem_wgrad_plan)
};
void stem_wgrad_plan(int64_t M, int* splits, int* chunk);
hipError_t launch_stem_wgrad(const StemWgradParams& p, hipStream_t s);
// fixed-order sum of the partials into G, OIHW (32, 3, 3, 3), and g (32); both overwritten
hipError_t launch_stem_wgrad_reduce(const StemWgradParams& p, float* G, float* g, hipStream_t s);
// out[o][ci] = float(double(w[o][ci]) * gamma[o] / sqrt(double(var[o]) + 1e-5)): a fused block's folded pointwise weights as a plain matrix
hipError_t launch_pw_fold(const float* w, const float* gamma, const float* var, float* out, int cout, int cin, hipStream_t s);
struct BnChainParams {               // BatchNorm at running statistics behind a conv: folded gradients -> raw ones (float64 inside)
    const float* G; const float* g;  // gradient of the folded weight [cout][K] and of the folded bias [cout]
    const float* W; const float* b;  // raw conv weight [cout][K] and bias
    const float* gamma; const float* mean; const float* var;
    float *dW, *db, *dgamma, *dbeta;
    int cout, K, accumulate;
};
hipError_t launch_bn_chain(const BnChainParams& p, hipStream_t s);

// ---- stage fine-tuning step (optim_kernels.hip; train.py:41-55, :106 and pack_weights for the stage layers)
constexpr int kAdamChunk = 1024;     // elements of one parameter a workgroup updates
struct AdamChunk {
    uint32_t goff, roff, n;          // float offset in the gradient array (and in exp_avg / exp_avg_sq), in d_raw, elements
    uint32_t group;                  // bits 0-1: log2 of the learning-rate multiplier (x1, x2, x4, x8), bit 2: weight decay on
};
struct AdamParams {
    const float* grads;              // lwp_stage_grad_spec's layout
    float* raw;                      // the handle's raw parameters
    float* exp_avg; float* exp_avg_sq;
    const AdamChunk* chunks; int n_chunks;
    int vec_ok;                      // every base pointer is 16-byte aligned
    double step_size[4];             // base_lr * {1, 2, 4, 8} / (1 - beta1^t), computed on the host
    double one_minus_b1, b2, one_minus_b2, sqrt_bc2, eps, weight_decay;   // sqrt_bc2 = sqrt(1 - beta2^t)
};
hipError_t launch_stage_adam(const AdamParams& p, hipStream_t s);
struct RepackBlock { int w_raw, b_raw, out_off, in_off, cout, cin; };    // one source conv of a merged head layer (WBlock)
struct RepackLayer {                 // one fp32 L_GEMM layer: where its raw parameters are and where its packed forms go
    uint32_t block_begin;            // first workgroup of the layer (one workgroup = 256 x 16 bytes of the fragment-order copy)
    uint32_t w_off, w2_off, b_off;   // float offsets into the blob
    int cin, cout, cin_pad, cout_pad, taps;
    int w_raw, b_raw, gamma_raw, beta_raw, mean_raw, var_raw;   // float offsets into d_raw, -1: the layer has none
    int n_blocks;                    // 0: a plain layer, else blk[0 .. n_blocks) are its source convs
    RepackBlock blk[2];
};
hipError_t launch_stage_repack(const RepackLayer* tab_device, int n_layers, int n_blocks, const float* raw, float* blob, hipStream_t s);
struct DwRepack {                    // one fp32 L_DW or L_DWPW layer (the cpm trunk; the backbone): float offsets into d_raw / the blob
    int C, cout;                     // cout = 0: L_DW, no pointwise half
    int dw_raw, pw_raw;
    uint32_t w_off, b_off, w2_off, b2_off;
    int dw_gamma, dw_beta, dw_mean, dw_var;   // BatchNorm behind the depthwise half (the backbone), -1: none (the cpm trunk)
    int pw_gamma, pw_beta, pw_mean, pw_var;   // ... behind the pointwise half
};
hipError_t launch_dw_repack(const DwRepack& l, const float* raw, float* blob, hipStream_t s);
struct StemRepack {                  // model.0: float offsets into d_raw / the blob
    int w_raw, gamma, beta, mean, var;
    uint32_t w_off, b_off;
};
hipError_t launch_stem_repack(const StemRepack& l, const float* raw, float* blob, hipStream_t s);

hipError_t init_cubic_tables();
hipError_t launch_reset_ws(int N, PostWorkspace& ws, hipStream_t s);
hipError_t launch_upsample(const MapView& src, int N, int C, int ratio, float* dst, hipStream_t s, const Tuning* tune = nullptr);
// threshold + strict 4-neighbour maximum on the (virtually) up-sampled heat-maps; ratio == 1: src is already full-res
hipError_t launch_find_peaks(const MapView& heat, int N, int ntypes, int ratio, PostWorkspace& ws, hipStream_t s, const Tuning* tune = nullptr);
// record_seen: the debug read-out of peaks per type (ntypes == ws.K)
hipError_t launch_nms(int N, int ntypes, int Hfull, PostWorkspace& ws, hipStream_t s, bool record_seen = false);
hipError_t launch_score_pairs(const MapView& paf, int N, int ratio, int demo, PostWorkspace& ws, hipStream_t s);
hipError_t launch_match(int N, PostWorkspace& ws, hipStream_t s);
hipError_t launch_assemble(int N, PostWorkspace& ws, hipStream_t s);
// u8 frame -> resized, normalised, padded CHW float32 (demo.py:59-64)
struct PreprocParams {
    const unsigned char* src; int Hs, Ws;            // HWC uint8, 3 channels
    const int *xi, *xw, *yi, *yw;                    // per destination index: 4 clamped source indices, 4 fixed-point weights
    int dh, dw, top, left, Hp, Wp;                   // scaled size, its offset inside the padded Hp x Wp frame
    double mean[3], scale;
    float pad_value[3];
    float* out;                                      // 3 x Hp x Wp
};
void build_resize_table_u8(int n_src, int n_dst, double inv_scale, std::vector<int>& idx, std::vector<int>& w);
hipError_t launch_preprocess_u8(const PreprocParams& p, hipStream_t s);
// N same-sized frames (src: N x Hs x Ws x 3, out: N x 3 x Hp x Wp), the tables shared; allow_vec: four pixels per thread with
// 16-byte stores where the geometry permits (false: one thread per pixel)
hipError_t launch_preprocess_u8_batch(const PreprocParams& p, int N, bool allow_vec, hipStream_t s);
// N uint8 frames -> normalised float64 image, cubic resize by a ratio (f32 coefficients, f64 sums), pad, NCHW float32 (val.py:84-93)
struct PreScaleParams {
    const void* src; int N, Hs, Ws;                  // N x Hs x Ws x 3 uint8 (float32 when src_f32)
    bool src_f32 = false;
    const int *xi, *yi;                              // 4 clamped source indices per destination index
    const float *xw, *yw;                            // 4 float32 cubic coefficients per destination index
    int dh, dw, top, left, Hp, Wp;
    double mean[3], scale;
    float pad_value[3];
    float* out;                                      // N x 3 x Hp x Wp
};
void build_resize_table_ratio(int n_src, int n_dst, double ratio, std::vector<int>& idx, std::vector<float>& w);
hipError_t launch_preprocess_scaled(const PreScaleParams& p, hipStream_t s);
hipError_t launch_fetch_host(const void* src_host_mapped, void* dst, size_t bytes, hipStream_t s);
hipError_t launch_publish(int N, PostWorkspace& ws, void* host_block, hipStream_t s);   // used rows -> pinned host block
void build_resize_table(int n_src, int n_dst, std::vector<int>& idx, std::vector<float>& w);
void multiscale_fused_extent(const int* xi, const int* yi, int dst_h, int dst_w, int tx, int* uh_max, int* uw_max);
void multiscale_fused_plan(const int* xi, const int* yi, int dst_h, int dst_w, int R, int* tx_best, int* uh_max, int* uw_max);
hipError_t launch_multiscale_fused(const MapView& src, int N, int C, int ratio, int crop_top, int crop_left, const int* xi, const float* xw,
                                   const int* yi, const float* yw, int dst_h, int dst_w, float divisor, int init, float* accum,
                                   int tx, int uh_max, int uw_max, hipStream_t s, bool* used);
void multiscale_fused_plan_v4(const int* xi, const int* yi, int dst_h, int dst_w, int R, int* tx_best, int* uh_max, int* uw_max);
hipError_t launch_multiscale_fused_v4(const MapView& src, int N, int C, int ratio, int crop_top, int crop_left, const int* xi, const float* xw,
                                      const int* yi, const float* yw, int dst_h, int dst_w, float divisor, int init, float* accum,
                                      int tx, int uh_max, int uw_max, hipStream_t s, bool* used);
hipError_t launch_resize_accum(const float* src, int N, int Hs, int Ws, int C, int crop_top, int crop_left, const int* xi, const float* xw,
                               const int* yi, const float* yw, int dst_h, int dst_w, float divisor, int init, float* accum, hipStream_t s);
hipError_t launch_threshold_inplace(float* map, int64_t n, hipStream_t s);
hipError_t launch_nchw_from_nhwc(const float* src, int src_ld, float* dst, int N, int HW, int C, hipStream_t s);

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) is a per-DEVICE setting: every launcher keeps one flag per device
// (a process may hold handles on several GPUs; the usual deployment is one process per GPU).
constexpr int kMaxDevices = 64;
struct LdsAttrOnce {
    bool done[kMaxDevices] = {};
    hipError_t ensure(const void* fn, int bytes) {
        int dev = 0;
        hipError_t e = hipGetDevice(&dev);
        if (e != hipSuccess) return e;
        if (dev < 0 || dev >= kMaxDevices) return hipErrorInvalidDevice;
        if (done[dev]) return hipSuccess;
        e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
        if (e == hipSuccess) done[dev] = true;
        return e;
    }
};

}  // namespace lwp
