// C-ABI entry points (include/lwpose.h).  Host orchestration only: buffer management, the static
// launch sequence of the layer graph on the handle's HIP stream, result fetch, and event timing.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <system_error>
#include <thread>
#include <vector>

#include "jpeg_batch.h"
#include "lwp_internal.h"
#include "lwp_owners.h"

using namespace lwp;

struct lwp_context {
    int device = 0;
    // The streams come before every buffer and event: members are destroyed in reverse order, so the streams go last.
    Stream stream, post_own;
    hipStream_t post_stream = nullptr;     // unset until the first submit; then post_own, or `stream` itself (LWP_POST_STREAM=0)
    int dtype = LWP_F32;
    Graph g;
    Tuning tune;                           // every LWP_* A/B switch, read from the environment at lwp_create
    std::vector<std::string> variants;     // per layer: the kernel variant its last launch picked (debug / profiling entry points only)
    bool record_variants = false;
    char variant_buf[kVariantCap] = {0};
    DevBuf d_blob, d_zeros;
    bool weights_loaded = false;
    // activations for the current (N, H, W)
    int cur_N = 0, cur_H = 0, cur_W = 0;
    std::vector<DevBuf> bufs;              // grow-only
    DevBuf d_in;
    std::vector<DevBuf> d_outs;            // NCHW staging for host outputs
    DevBuf d_tmp, d_tmp2;                  // generic device staging (upsample / extract / group)
    // resize tables of one geometry, kept on the device: the four host arrays back to back in one allocation
    // (a per-call upload went through SDMA queues: multi-ms stalls on some boxes)
    struct TabKey {
        int cw, ch, dw, dh; double ratio; int up_ratio;
        bool operator==(const TabKey& o) const { return cw == o.cw && ch == o.ch && dw == o.dw && dh == o.dh && ratio == o.ratio && up_ratio == o.up_ratio; }
    };
    struct MsPlan { int uh_max = 0, uw_max = 0, tx = 0, tx4 = 0, uh4 = 0, uw4 = 0; };   // the fused multi-scale kernels' tile extents
    template <class Wt> struct TabArrays { int* xi; Wt* xw; int* yi; Wt* yw; };   // device pointers
    struct ResizeTab {
        TabKey key; DevBuf d; MsPlan plan;
        size_t nx = 0, ny = 0;             // elements of the x and of the y arrays (4 per destination column / row)
        // the four arrays of the allocation, xi | xw | yi | yw; Wt: the weights' type (int: fixed point, float: cubic coefficients)
        template <class Wt> TabArrays<Wt> arrays() const {
            char* t = d.as<char>();
            return {(int*)t, (Wt*)(t + nx * 4), (int*)(t + nx * 8), (Wt*)(t + nx * 8 + ny * 4)};
        }
    };
    typedef std::vector<ResizeTab> TabCache;
    TabCache resize_tabs;                  // cubic tables of the multi-scale path: (cw, ch, dst_w, dst_h, up_ratio)
    TabCache scale_tabs;                   // image-side tables of lwp_preprocess_scaled_u8: (W, H, dw, dh, ratio)
    DevBuf d_imgs;                         // staging of host frames (uint8 pre-processing, multi-scale image side, lwp_draw_poses)
    // host frames travel through one of two pinned buffers (upload_host): a copy from pageable memory is staged by the runtime
    // anyway, at ~100 us per 720 KB frame and with the calling thread blocked until the DMA has finished
    PinBuf pin_buf[2]; Event pin_ev[2]; bool pin_busy[2] = {false, false};
    int pin_next = 0;
    TabCache pre_tabs;                     // fixed-point tables of the uint8 pre-processing, one set per geometry (W, H, dw, dh, scale): never rewritten, so a
                                           // call with a new frame size cannot race the launches of another slot that still read the old ones
    DevBuf d_pipe_in;                      // network input of lwp_pipeline_submit_u8 (written and read on the main stream only)
    DevBuf d_maps[2];                      // bf16 path: f32 NCHW heat / PAF of the last stage
    // post-processing
    PostCaps caps;
    struct WsMem { DevBuf arena, block; };  // the memory behind a PostWorkspace: the scratch arrays (ws_sections), the result block
    PostWorkspace ws; WsMem ws_mem;
    Skeleton skel = default_skeleton();    // grouping tables + options (lwp_set_skeleton); host state, not part of the weights
    DevBuf d_limbs;                        // [kMaxSkelLimbs][4] ints: device copy of skel's limb table (the generic kernels read it)
    // pinned host staging for results
    PinBuf h_stage;
    int last_N = 0;
    // pipelined streaming mode: two result slots, post-processing + fetch of frame k overlap the network of frame k+1
    struct Slot {
        PostWorkspace ws; WsMem ws_mem;
        DevBuf maps[2];
        PinBuf h_stage;
        Event ev_maps, ev_done;
        int N = 0;
        int tail_N = 0;                    // frames with pose rows in h_stage (0: submitted with the tail off)
        bool pending = false;
        // pose overlay (lwp_set_overlay): the slot OWNS the source pixels of host frames until its overlay has run (the shared
        // d_imgs staging is overwritten by the next submit on the main stream while this slot's post stream still reads it)
        DevBuf frames;                     // uploaded host frames of this slot
        DevBuf ov;                         // annotated frames, device
        PinBuf h_ov;                       // mode 2: their pinned host copy
        int ov_N = 0, ov_H = 0, ov_W = 0, ov_mode = 0;              // ov_N == 0: the slot ran without the overlay
    } slots[2];
    // pose tail (lwp_set_tracking): parameters, the lanes' device state and its memory, (2 sigma)^2 of the K key-point types
    TailParams tail;
    TailState tst; DevBuf tst_mem[9];
    DevBuf d_vars;
    // pose overlay (lwp_set_overlay): settings, and the device staging of lwp_draw_poses (pose arrays; frames out for host `out`)
    struct Overlay { int mode = 0, boxes = 1, n_draw_limbs = -1; unsigned char color[3] = {0, 224, 255}, box_color[3] = {0, 255, 0}; } ovl;
    DevBuf d_ov_pose, d_ov_out;
    // training targets and loss (lwp_train_targets / lwp_mask_downsample / lwp_stage_losses): staging of host key-points, person
    // counts and host masks; the loss partials followed by the per-stage sums
    DevBuf d_train, d_loss;
    // the running loss log of lwp_stage_losses_log / lwp_loss_log_read: S doubles and, behind them, the int64 add count
    DevBuf d_loss_log;
    // training augmentation (lwp_augment_batch): [plan records | host images and masks], packed on the host, one upload a batch;
    // lwp_augment_batch_crowd: [.. | run tables] and, behind the upload, the rendered crowd masks; lwp_crowd_masks: [run tables]
    DevBuf d_augment;
    std::vector<unsigned char> augment_stage;
    // stage backward (lwp_train_forward / lwp_stage_backward; f32 handles): the retaining buffer plan, its activation and
    // gradient buffers, the gradient array's layout, the raw stage parameters (the BatchNorm chain rule needs them unfolded)
    TrainPlan tp;
    int scope = LWP_TRAIN_STAGES;                    // lwp_set_train_scope: which parameters the plan, the gradient array and the optimiser cover
    std::vector<DevBuf> tbufs, gbufs;                // (a gradient buffer has the size of its activation buffer)
    DevBuf d_train_in;                               // LWP_TRAIN_ALL: the image of the last retaining forward (the stem's weight gradient reads it)
    int train_N = 0, train_H = 0, train_W = 0;      // frames of the last retaining forward (0: none)
    struct GradSpec { std::string key; int64_t shape[4]; int ndim; size_t off; };
    std::vector<GradSpec> gspec;
    std::map<std::string, size_t> grad_off;          // state-dict key -> float offset in the gradient array
    std::map<std::string, size_t> raw_off;           // the same keys, and the BatchNorm running statistics -> float offset in d_raw
    size_t grad_floats = 0, raw_floats = 0;
    DevBuf d_raw;
    bool raw_loaded = false;                         // false after lwp_weights_blob_import: a blob holds folded weights only
    DevBuf d_bwd; size_t bwd_fold_off = 0;           // wgrad partials, then the folded gradients of one BatchNorm layer,
    size_t bwd_pw_off = 0;                           // then (LWP_TRAIN_ALL) the folded pointwise matrix of one fused backbone block
    BwdPrecision bwd_prec;                           // lwp_set_backward_precision: operand type and dZ scale of dgrad / wgrad
    std::vector<int> bwd_splits;                     // per layer: pixel splits its last wgrad ran with
    std::vector<int> bwd_dw_splits;                  // per layer: pixel splits of its last depthwise wgrad (L_DW, L_DWPW)
    std::vector<DwRepack> dw_repack;                 // the depthwise / fused layers of the repack: the cpm trunk's, the backbone's (LWP_TRAIN_ALL)
    StemRepack stem_repack{}; bool has_stem_repack = false;      // model.0 (LWP_TRAIN_ALL)
    // stage fine-tuning step (lwp_stage_adam_step): exp_avg then exp_avg_sq in one allocation, the step count, and the two
    // device tables the host builds once per handle (parameter chunks of the Adam kernel, layer descriptors of the repack)
    DevBuf d_adam; size_t adam_sq_off = 0;
    int64_t adam_t = 0;
    DevBuf d_adam_chunks; int adam_chunks = 0;
    DevBuf d_repack; int repack_layers = 0, repack_blocks = 0;
    // detection store (lwp_coco_open): the resident ground truth [gt_off | gt_kp | gt_area | gt_bbox | gt_iscrowd | gt_ignore],
    // the rows [kp | score | image], the tables [control words | count | start], and a pinned ring through which host rows and
    // image indices reach the append kernels without a synchronise
    struct CocoStoreMem {
        bool open = false;
        DevBuf gt, rows, meta;
        PinBuf ring; size_t ring_used = 0;
        CocoStore st{};
        int64_t NG = 0;
        size_t o_kp = 0, o_area = 0, o_bbox = 0, o_crowd = 0, o_ignore = 0;     // byte offsets into gt (gt_off is at 0)
        std::vector<int64_t> gt_off;                 // host copy: the OKS offsets of an evaluation need G per image
        std::vector<char> added;                     // per image: rows were appended since the last reset
    } coco;
    // A JPEG batch's device workspace [upload][device-only regions] (jpeg_batch.h lays both out), the pinned staging the upload
    // is built in, and the event behind the staging's last copy: the staging is not rewritten before it (jpeg_stage_begin)
    struct JpegMem { DevBuf dev; PinBuf stage; Event ev; bool copy_pending = false; };
    JpegMem jpeg;                                    // lwp_jpeg_decode_batch, both entropy modes
    // lwp_jpeg_encode_batch; the scans come back through the staging too.  Every encode call ends synchronised, so neither
    // buffer outlives it in use and the event is never recorded
    JpegMem jpeg_enc;
    int jpeg_entropy_mode = LWP_JPEG_ENTROPY_HOST, jpeg_subseq = kJpegSubseqDefault;     // lwp_set_jpeg_entropy
    bool async_pending = false;                      // an lwp_infer_poses_async whose results were not fetched yet
    int tail_first_id = 0;                 // first id of a lane that is created later (lwp_reset_tracking(-1, id))
    int stage_tail_N = 0;                  // frames whose pose rows h_stage holds (0: the last fetch ran without the tail)
    bool run_has_tail = false;             // the tail kernels ran behind the grouping whose results h->ws holds
    // caller-stream ordering (lwp_set_stream): work the caller queued on ITS stream is waited for with an event (no host
    // block), and the caller's stream is made to wait for the handle's results where they stay on the device
    hipStream_t caller_stream = nullptr;
    bool caller_ordered = false;
    bool hand_over = true;                 // lwp_set_stream mode 1: device results are handed to the caller's stream; mode 2: not
    Event ev_in, ev_out, ev_copy;
    // per-launch profiling
    bool profiling = false;
    std::vector<Event> ev;
    std::vector<int> ev_class;
    std::vector<int> ev_layer;             // index of the (first) layer a launch covers, -1: post-processing kernel
    int cur_layer = -1;
    size_t ev_used = 0;
    std::string err;

    float* blob(size_t off) const { return d_blob.as<float>() + off; }   // weights at a float offset of the packed blob
    float* raw(const std::string& key) const { return d_raw.as<float>() + raw_off.at(key); }
};

static std::string g_err;
static std::mutex g_mu;

namespace lwp {
Skeleton default_skeleton() {              // modules/keypoints.py:5-8
    static const int kpt[19][2] = {{1, 2}, {1, 5}, {2, 3}, {3, 4}, {5, 6}, {6, 7}, {1, 8}, {8, 9}, {9, 10}, {1, 11},
                                   {11, 12}, {12, 13}, {1, 0}, {0, 14}, {14, 16}, {0, 15}, {15, 17}, {2, 16}, {5, 17}};
    static const int paf[19][2] = {{12, 13}, {20, 21}, {14, 15}, {16, 17}, {22, 23}, {24, 25}, {0, 1}, {2, 3}, {4, 5}, {6, 7},
                                   {8, 9}, {10, 11}, {28, 29}, {30, 31}, {34, 35}, {32, 33}, {36, 37}, {18, 19}, {26, 27}};
    Skeleton s;
    s.kpt.assign(&kpt[0][0], &kpt[0][0] + 38);
    s.paf.assign(&paf[0][0], &paf[0][0] + 38);
    return s;
}
}  // namespace lwp

// the stage parameters that receive a gradient, in lwp_param_spec order (running statistics and counters excluded)
static bool is_stage_key(const std::string& k) { return k.rfind("initial_stage.", 0) == 0 || k.rfind("refinement_stages.", 0) == 0; }
static bool is_cpm_key(const std::string& k) { return k.rfind("cpm.", 0) == 0; }
static bool is_backbone_key(const std::string& k) { return k.rfind("model.", 0) == 0; }
// parts of the layout: 0 backbone, 1 cpm, 2 stages; a scope's layout is its first part and everything behind it
static int first_part(int scope) { return scope == LWP_TRAIN_ALL ? 0 : scope == LWP_TRAIN_CPM ? 1 : 2; }
static bool in_part(int part, const std::string& k) { return part == 0 ? is_backbone_key(k) : part == 1 ? is_cpm_key(k) : is_stage_key(k); }
// LWP_TRAIN_CPM: the ten cpm.* parameters first, then the stage parameters (the unchanged tail, shifted by the cpm total);
// LWP_TRAIN_ALL: the 69 model.* parameters in front of that
static std::vector<lwp_context::GradSpec> train_grad_spec(int scope, int nref, int C, int NH, int NP, size_t* total) {
    std::vector<lwp_context::GradSpec> v;
    size_t off = 0;
    const std::vector<ParamSpec> table = param_table(nref, C, NH, NP);
    for (int part = first_part(scope); part < 3; ++part)
        for (const ParamSpec& p : table) {
            if (!in_part(part, p.key) || p.role == LWP_ROLE_BN_MEAN || p.role == LWP_ROLE_BN_VAR || p.role == LWP_ROLE_BN_NBT) continue;
            lwp_context::GradSpec s;
            s.key = p.key; s.ndim = p.ndim; s.off = off;
            size_t n = 1;
            for (int d = 0; d < 4; ++d) { s.shape[d] = p.shape[d]; if (d < p.ndim) n *= (size_t)p.shape[d]; }
            off += n;
            v.push_back(s);
        }
    if (total) *total = off;
    return v;
}
static std::vector<lwp_context::GradSpec> stage_grad_spec(int nref, int C, int NH, int NP, size_t* total) {
    return train_grad_spec(LWP_TRAIN_STAGES, nref, C, NH, NP, total);
}

static int fail(lwp_context* h, int code, const std::string& msg) {
    if (h) h->err = msg;
    else { std::lock_guard<std::mutex> l(g_mu); g_err = msg; }
    return code;
}
#define HIP_TRY(h, expr)                                                                       \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess)                                                                  \
            return fail(h, LWP_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));    \
    } while (0)

// caller's stream -> handle's stream: everything the caller has queued so far (producers of our inputs, consumers of the
// buffers we are about to overwrite) is ordered before our next launch.  No-op unless lwp_set_stream enabled it.
static int order_in(lwp_context* h) {
    if (!h->caller_ordered) return LWP_OK;
    // an idle caller stream has nothing to wait for: no event, no cross-queue barrier packet (with the three engine streams of
    // the batch-1 protocol a device-side wait on the shared default stream at every submit cost 20 % of the throughput)
    const hipError_t q = hipStreamQuery(h->caller_stream);
    if (q == hipSuccess) return LWP_OK;
    if (q != hipErrorNotReady) return fail(h, LWP_ERR_HIP, std::string("hipStreamQuery: ") + hipGetErrorString(q));
    (void)hipGetLastError();                         // "not ready" is an answer, not a failure: keep it out of the launchers' error checks
    HIP_TRY(h, hipEventRecord(h->ev_in, h->caller_stream));
    HIP_TRY(h, hipStreamWaitEvent(h->stream, h->ev_in, 0));
    return LWP_OK;
}
// handle's stream `from` -> caller's stream: what the caller queues next sees our device-side results.  Returns true in
// *ordered when the hand-over was done with an event (the legacy host synchronisation is then not needed).
static int order_out(lwp_context* h, hipStream_t from, bool* ordered) {
    *ordered = false;
    if (!h->caller_ordered) return LWP_OK;
    if (!h->hand_over) { *ordered = true; return LWP_OK; }        // mode 2: the result stays on the handle's stream (its next call consumes it)
    HIP_TRY(h, hipEventRecord(h->ev_out, from));
    HIP_TRY(h, hipStreamWaitEvent(h->caller_stream, h->ev_out, 0));
    *ordered = true;
    return LWP_OK;
}

extern "C" int lwp_version(void) { return 109; }

extern "C" int lwp_set_stream(lwp_handle h, void* caller_stream, int enable) {
    if (!h) return LWP_ERR_ARG;
    HIP_TRY(h, hipSetDevice(h->device));
    if (enable) {
        HIP_TRY(h, h->ev_in.ensure(hipEventDisableTiming));
        HIP_TRY(h, h->ev_out.ensure(hipEventDisableTiming));
    }
    h->caller_stream = (hipStream_t)caller_stream;
    h->caller_ordered = enable != 0;
    h->hand_over = enable != 2;
    return LWP_OK;
}

extern "C" int lwp_param_count(int nref, int C, int NH, int NP) {
    if (nref < 0 || C <= 0 || NH <= 0 || NP <= 0) return LWP_ERR_ARG;
    return (int)param_table(nref, C, NH, NP).size();
}

extern "C" int lwp_param_spec(int nref, int C, int NH, int NP, int index, char* name, int name_cap, int64_t shape[4],
                              int* ndim, int* role) {
    if (nref < 0 || C <= 0 || NH <= 0 || NP <= 0 || !name || !shape || !ndim || !role) return fail(nullptr, LWP_ERR_ARG, "bad argument");
    auto t = param_table(nref, C, NH, NP);
    if (index < 0 || index >= (int)t.size()) return fail(nullptr, LWP_ERR_ARG, "index out of range");
    if ((int)t[index].key.size() + 1 > name_cap) return fail(nullptr, LWP_ERR_ARG, "name buffer too small");
    std::strcpy(name, t[index].key.c_str());
    for (int d = 0; d < 4; ++d) shape[d] = t[index].shape[d];
    *ndim = t[index].ndim;
    *role = t[index].role;
    return LWP_OK;
}

extern "C" int lwp_debug_graph_fusions(int nref, int C, int NH, int NP, int dtype, int fuse_dwpw, int merge_heads, int* fuse, char* names,
                                       int name_stride, int cap, int* n_layers) {
    if (nref < 0 || C <= 0 || C % 32 || NH <= 0 || NP <= 0 || !fuse || !n_layers || (names && name_stride <= 0)) return fail(nullptr, LWP_ERR_ARG, "bad argument");
    if (dtype != LWP_F32 && dtype != LWP_BF16 && dtype != LWP_F16) return fail(nullptr, LWP_ERR_ARG, "bad dtype");
    if (dtype != LWP_F32 && !(C % 64 == 0 && dwpw_supported(C, C))) return fail(nullptr, LWP_ERR_ARG, "the 16-bit paths support num_channels 64, 128, 256 or 512 only");
    const Graph g = build_graph(nref, C, NH, NP, fuse_dwpw != 0, dtype, merge_heads != 0);
    TrainPlan tp;                                      // fp32: from cpm.conv on, the marks the retaining plan's copy carries
    if (dtype == LWP_F32) tp = build_train_plan(g);
    *n_layers = (int)g.layers.size();
    if (*n_layers > cap) return fail(nullptr, LWP_ERR_CAPACITY, "fuse array too small");
    for (size_t i = 0; i < g.layers.size(); ++i) {
        fuse[i] = (tp.cpm_conv >= 0 && (int)i >= tp.cpm_conv ? tp.layers[i] : g.layers[i]).fuse;
        if (!names) continue;
        if ((int)g.layers[i].name.size() + 1 > name_stride) return fail(nullptr, LWP_ERR_CAPACITY, "name stride too small");
        std::strcpy(names + i * (size_t)name_stride, g.layers[i].name.c_str());
    }
    return LWP_OK;
}

extern "C" const char* lwp_last_error(lwp_handle h) {
    if (h) return h->err.c_str();
    std::lock_guard<std::mutex> l(g_mu);
    return g_err.c_str();
}

// the retaining plan, its (empty) buffers and the gradient layout of a scope; the caller has made sure nothing still runs on them
static void apply_train_scope(lwp_context* h, int scope) {
    const Graph& g = h->g;
    h->scope = scope;
    h->tp = build_train_plan(g, scope);
    h->tbufs = std::vector<DevBuf>(h->tp.bufs.size());
    h->gbufs = std::vector<DevBuf>(h->tp.bufs.size());
    h->d_train_in = DevBuf();
    h->gspec = train_grad_spec(scope, g.nref, g.C, g.NH, g.NP, &h->grad_floats);
    h->grad_off.clear();
    for (const auto& s : h->gspec) h->grad_off[s.key] = s.off;
    h->bwd_splits.assign(g.layers.size(), 0);
    h->bwd_dw_splits.assign(g.layers.size(), 0);
    h->train_N = h->train_H = h->train_W = 0;
    h->d_adam = DevBuf(); h->adam_sq_off = 0; h->adam_t = 0;
    h->d_adam_chunks = DevBuf(); h->adam_chunks = 0;
    h->d_repack = DevBuf(); h->repack_layers = h->repack_blocks = 0;
    h->dw_repack.clear();
    h->has_stem_repack = false;
}

extern "C" int lwp_create(int device_id, int nref, int C, int NH, int NP, int dtype, lwp_handle* out) {
    if (!out) return fail(nullptr, LWP_ERR_ARG, "out is null");
    *out = nullptr;
    if (nref < 0 || C <= 0 || C % 32 || NH <= 0 || NP <= 0) return fail(nullptr, LWP_ERR_ARG, "bad network shape (num_channels must be a multiple of 32)");
    if (dtype != LWP_F32 && dtype != LWP_BF16 && dtype != LWP_F16) return fail(nullptr, LWP_ERR_ARG, "bad dtype");
    // the 16-bit graph has no stand-alone depthwise kernel and its GEMM walks K in 64-channel steps: cpm.trunk must fuse
    // (C in {64, 128, 256, 512}); any other width would run f32 kernels on 16-bit buffers
    if (dtype != LWP_F32 && !(C % 64 == 0 && dwpw_supported(C, C)))
        return fail(nullptr, LWP_ERR_ARG, std::string(dtype == LWP_F16 ? "fp16" : "bf16") + " path supports num_channels 64, 128, 256 or 512 only");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(nullptr, LWP_ERR_NOGPU, "no HIP device available");
    if (device_id < 0 || device_id >= ndev) return fail(nullptr, LWP_ERR_ARG, "device_id out of range");
    hipError_t e = hipSetDevice(device_id);
    if (e != hipSuccess) return fail(nullptr, LWP_ERR_HIP, std::string("hipSetDevice: ") + hipGetErrorString(e));
    hipDeviceProp_t prop;
    e = hipGetDeviceProperties(&prop, device_id);
    if (e != hipSuccess) return fail(nullptr, LWP_ERR_HIP, std::string("hipGetDeviceProperties: ") + hipGetErrorString(e));
    if (std::string(prop.gcnArchName).find("gfx950") == std::string::npos)
        return fail(nullptr, LWP_ERR_NOGPU, std::string("this library is built for gfx950 only, found ") + prop.gcnArchName);
    lwp_context* h = new lwp_context();
    h->device = device_id;
    h->dtype = dtype;
    h->tune = tuning_from_env();
    h->g = build_graph(nref, C, NH, NP, h->tune.fuse_dwpw != 0, dtype, h->tune.merge_heads != 0);
    h->variants.assign(h->g.layers.size(), std::string());
    e = h->stream.ensure();
    if (e != hipSuccess) { delete h; return fail(nullptr, LWP_ERR_HIP, std::string("stream: ") + hipGetErrorString(e)); }
    e = init_cubic_tables();
    if (e != hipSuccess) { delete h; return fail(nullptr, LWP_ERR_HIP, std::string("init_cubic_tables: ") + hipGetErrorString(e)); }
    e = h->d_blob.ensure(h->g.blob_floats * sizeof(float));
    if (e != hipSuccess) { delete h; return fail(nullptr, LWP_ERR_HIP, std::string("blob: ") + hipGetErrorString(e)); }
    e = h->d_zeros.ensure(4096);
    if (e == hipSuccess) e = hipMemset(h->d_zeros.as<void>(), 0, 4096);
    if (e != hipSuccess) { delete h; return fail(nullptr, LWP_ERR_HIP, std::string("zeros: ") + hipGetErrorString(e)); }
    {
        std::vector<int> t(19 * 4);
        for (int l = 0; l < 19; ++l)
            for (int k = 0; k < 2; ++k) { t[l * 4 + k] = h->skel.kpt[l * 2 + k]; t[l * 4 + 2 + k] = h->skel.paf[l * 2 + k]; }
        e = h->d_limbs.ensure((size_t)kMaxSkelLimbs * 4 * sizeof(int));
        if (e == hipSuccess) e = hipMemcpy(h->d_limbs.as<void>(), t.data(), t.size() * sizeof(int), hipMemcpyHostToDevice);
        if (e != hipSuccess) { delete h; return fail(nullptr, LWP_ERR_HIP, std::string("limbs: ") + hipGetErrorString(e)); }
    }
    h->bufs.resize(h->g.bufs.size());
    if (dtype == LWP_F32) {
        apply_train_scope(h, LWP_TRAIN_STAGES);
        // the raw parameters do not move with the scope: the stage parameters in the stage gradient layout, the BatchNorm
        // running statistics, then (16-byte aligned) the cpm parameters
        h->raw_off = h->grad_off;
        h->raw_floats = h->grad_floats;
        for (const ParamSpec& p : param_table(nref, C, NH, NP))
            if (is_stage_key(p.key) && (p.role == LWP_ROLE_BN_MEAN || p.role == LWP_ROLE_BN_VAR)) { h->raw_off[p.key] = h->raw_floats; h->raw_floats += (size_t)p.shape[0]; }
        h->raw_floats = (h->raw_floats + 3) / 4 * 4;
        for (const auto& s : train_grad_spec(LWP_TRAIN_CPM, nref, C, NH, NP, nullptr)) {
            if (!is_cpm_key(s.key)) continue;
            size_t n = 1;
            for (int d = 0; d < s.ndim; ++d) n *= (size_t)s.shape[d];
            h->raw_off[s.key] = h->raw_floats; h->raw_floats += n;
        }
        // ... then (16-byte aligned) the backbone parameters (LWP_TRAIN_ALL) and their running statistics
        h->raw_floats = (h->raw_floats + 3) / 4 * 4;
        for (const ParamSpec& p : param_table(nref, C, NH, NP)) {
            if (!is_backbone_key(p.key) || p.role == LWP_ROLE_BN_NBT) continue;
            size_t n = 1;
            for (int d = 0; d < p.ndim; ++d) n *= (size_t)p.shape[d];
            h->raw_off[p.key] = h->raw_floats; h->raw_floats += n;
        }
    }
    h->d_outs.resize(2 * (1 + nref));
    *out = h;
    return LWP_OK;
}

static void free_ws_obj(PostWorkspace& w, lwp_context::WsMem& m) {
    (void)m.arena.reset();
    (void)m.block.reset();
    w = PostWorkspace();
}
// every workspace of the handle: its own and the two slots'
static void free_workspaces(lwp_context* h) {
    free_ws_obj(h->ws, h->ws_mem);
    for (auto& sl : h->slots) free_ws_obj(sl.ws, sl.ws_mem);
}
static void free_tail_state(lwp_context* h) {
    for (DevBuf& b : h->tst_mem) (void)b.reset();
    h->tst = TailState();
    h->stage_tail_N = 0;
    for (auto& sl : h->slots) sl.tail_N = 0;
}

extern "C" int lwp_destroy(lwp_handle h) {
    if (!h) return LWP_OK;
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    if (h->post_stream) (void)hipStreamSynchronize(h->post_stream);
    delete h;                                          // every member releases what it owns; the streams go last
    return LWP_OK;
}

extern "C" int lwp_set_capacity(lwp_handle h, int max_peaks, int max_kpts, int max_conn, int max_entries) {
    if (!h) return LWP_ERR_ARG;
    if (max_peaks < 64 || max_peaks > 8192 || max_kpts < 1 || max_kpts > 1024 || max_conn < 1 || max_conn > (1 << 20) ||
        max_entries < 1 || max_entries > 65535)
        return fail(h, LWP_ERR_ARG, "capacity out of range (peaks 64..8192, kpts 1..1024, conns 1..2^20, entries 1..65535)");
    for (auto& sl : h->slots) if (sl.pending) return fail(h, LWP_ERR_STATE, "pipeline slot pending");
    (void)hipSetDevice(h->device);
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    free_workspaces(h);
    if (h->post_stream) HIP_TRY(h, hipStreamSynchronize(h->post_stream));
    free_tail_state(h);                                // the lanes' state is sized by max_entries: every lane starts over
    h->last_N = 0; h->async_pending = false;   // the results of an unfetched lwp_infer_poses_async went with the workspace
    h->caps.max_peaks = max_peaks; h->caps.max_kpts = max_kpts; h->caps.max_conn = max_conn; h->caps.max_entries = max_entries;
    return LWP_OK;
}

// ---------------------------------------------------------------------------------------------- skeleton
extern "C" int lwp_set_skeleton(lwp_handle h, int num_kpt_types, int num_limbs, const int* limb_kpts, const int* limb_pafs,
                                int pose_entry_size, double min_paf_score) {
    if (!h) return LWP_ERR_ARG;
    Skeleton sk = default_skeleton();
    if (limb_kpts) {
        const int K = num_kpt_types, L = num_limbs, E = pose_entry_size;
        char msg[200];
        if (K < 1 || K > kMaxSkelTypes) return fail(h, LWP_ERR_ARG, "num_kpt_types must be 1..64");
        if (K > h->g.NH) {
            snprintf(msg, sizeof msg, "num_kpt_types %d exceeds the network's %d heat-maps", K, h->g.NH);
            return fail(h, LWP_ERR_ARG, msg);
        }
        if (L < 1 || L > kMaxSkelLimbs) return fail(h, LWP_ERR_ARG, "num_limbs must be 1..320");
        if (!limb_pafs) return fail(h, LWP_ERR_ARG, "limb_pafs is null");
        if (E < K + 2 || E > kMaxEntrySize) {
            snprintf(msg, sizeof msg, "pose_entry_size must be num_kpt_types + 2 .. 256 (got %d for %d key-point types)", E, K);
            return fail(h, LWP_ERR_ARG, msg);
        }
        for (int l = 0; l < L; ++l) {
            const int a = limb_kpts[2 * l], b = limb_kpts[2 * l + 1], c0 = limb_pafs[2 * l], c1 = limb_pafs[2 * l + 1];
            if (a < 0 || a >= K || b < 0 || b >= K || a == b) {
                snprintf(msg, sizeof msg, "limb %d: key-point types (%d, %d) must be distinct and in 0..%d", l, a, b, K - 1);
                return fail(h, LWP_ERR_ARG, msg);
            }
            if (c0 < 0 || c0 >= h->g.NP || c1 < 0 || c1 >= h->g.NP) {
                snprintf(msg, sizeof msg, "limb %d: PAF channels (%d, %d) must be in 0..%d", l, c0, c1, h->g.NP - 1);
                return fail(h, LWP_ERR_ARG, msg);
            }
        }
        sk.K = K; sk.L = L; sk.E = E;
        sk.min_paf = min_paf_score;
        sk.kpt.assign(limb_kpts, limb_kpts + 2 * L);
        sk.paf.assign(limb_pafs, limb_pafs + 2 * L);
        const Skeleton d = default_skeleton();
        sk.is_default = K == d.K && L == d.L && E == d.E && min_paf_score == d.min_paf && sk.kpt == d.kpt && sk.paf == d.paf;
    }
    HIP_TRY(h, hipSetDevice(h->device));
    for (auto& sl : h->slots) if (sl.pending) return fail(h, LWP_ERR_STATE, "pipeline slot pending");
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (h->post_stream) HIP_TRY(h, hipStreamSynchronize(h->post_stream));
    std::vector<int> t((size_t)sk.L * 4);
    for (int l = 0; l < sk.L; ++l)
        for (int k = 0; k < 2; ++k) { t[l * 4 + k] = sk.kpt[l * 2 + k]; t[l * 4 + 2 + k] = sk.paf[l * 2 + k]; }
    HIP_TRY(h, hipMemcpy(h->d_limbs.as<void>(), t.data(), t.size() * sizeof(int), hipMemcpyHostToDevice));
    free_workspaces(h);                                // every workspace is sized by K / L / E: re-allocated lazily
    free_tail_state(h);                                // the lanes' state is sized by K: every lane starts over
    if (h->tail.mode >= 2 && sk.K != h->skel.K) h->tail.mode = 0;   // the sigma table was given for the old K: tracking is off until lwp_set_tracking
    h->last_N = 0; h->async_pending = false;   // the results of an unfetched lwp_infer_poses_async went with the workspace
    h->skel = sk;
    return LWP_OK;
}

extern "C" int lwp_get_skeleton(lwp_handle h, int* num_kpt_types, int* num_limbs, int* limb_kpts, int* limb_pafs, int limb_cap,
                                int* pose_entry_size, double* min_paf_score) {
    if (!h) return LWP_ERR_ARG;
    const Skeleton& sk = h->skel;
    if (num_kpt_types) *num_kpt_types = sk.K;
    if (num_limbs) *num_limbs = sk.L;
    if (pose_entry_size) *pose_entry_size = sk.E;
    if (min_paf_score) *min_paf_score = sk.min_paf;
    if (limb_kpts || limb_pafs) {
        if (limb_cap < sk.L) return fail(h, LWP_ERR_CAPACITY, "limb arrays too small");
        if (limb_kpts) std::copy(sk.kpt.begin(), sk.kpt.end(), limb_kpts);
        if (limb_pafs) std::copy(sk.paf.begin(), sk.paf.end(), limb_pafs);
    }
    return LWP_OK;
}

extern "C" int lwp_load_weights(lwp_handle h, const char* const* names, const void* const* ptrs, const int64_t* shapes,
                                const int* ndims, int n) {
    if (!h || !names || !ptrs || !shapes || !ndims || n <= 0) return fail(h, LWP_ERR_ARG, "bad argument");
    std::vector<std::string> nm(n);
    std::vector<HostTensor> ts(n);
    for (int i = 0; i < n; ++i) {
        nm[i] = names[i] ? names[i] : "";
        ts[i].ptr = ptrs[i];
        ts[i].ndim = ndims[i];
        for (int d = 0; d < 4; ++d) ts[i].shape[d] = shapes[i * 4 + d];
    }
    std::vector<float> blob;
    std::string msg = pack_weights(h->g, nm, ts, blob);
    if (!msg.empty()) return fail(h, LWP_ERR_ARG, msg);
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));         // a queued lwp_stage_adam_step still writes the blob and the raw parameters
    HIP_TRY(h, hipMemcpy(h->d_blob.as<float>(), blob.data(), blob.size() * sizeof(float), hipMemcpyHostToDevice));
    h->weights_loaded = true;
    if (h->dtype == LWP_F32) {                           // the stage parameters as given: lwp_stage_backward's BatchNorm chain rule
        std::vector<float> raw(h->raw_floats, 0.0f);
        for (int i = 0; i < n; ++i) {
            auto it = h->raw_off.find(nm[i]);
            if (it == h->raw_off.end()) continue;
            size_t cnt = 1;
            for (int d = 0; d < ts[i].ndim; ++d) cnt *= (size_t)ts[i].shape[d];
            std::memcpy(raw.data() + it->second, ts[i].ptr, cnt * sizeof(float));     // shapes were checked by pack_weights
        }
        HIP_TRY(h, h->d_raw.ensure(std::max<size_t>(h->raw_floats, 1) * sizeof(float)));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        HIP_TRY(h, hipMemcpy(h->d_raw.as<float>(), raw.data(), raw.size() * sizeof(float), hipMemcpyHostToDevice));
        h->raw_loaded = true;
    }
    return LWP_OK;
}

// A bf16 and an fp16 blob of one network have the same packed size, so an fp16 blob carries a 16-byte trailer (tag + packed
// size) that the import checks: a blob of another dtype is refused instead of being reinterpreted.  f32 and bf16 blobs are
// the packed weights alone, as they always were.
static void f16_blob_tag(const lwp_context* h, uint64_t tag[2]) {
    std::memcpy(&tag[0], "lwpF16\0\1", 8);
    tag[1] = (uint64_t)h->g.blob_floats;
}
static size_t blob_bytes(const lwp_context* h) {
    return h->g.blob_floats * sizeof(float) + (h->dtype == LWP_F16 ? 2 * sizeof(uint64_t) : 0);
}
extern "C" int lwp_weights_blob_bytes(lwp_handle h, size_t* bytes) {
    if (!h || !bytes) return LWP_ERR_ARG;
    *bytes = blob_bytes(h);
    return LWP_OK;
}
extern "C" int lwp_weights_blob_export(lwp_handle h, void* dst, size_t bytes) {
    if (!h || !dst || bytes != blob_bytes(h)) return fail(h, LWP_ERR_ARG, "bad blob size");
    if (!h->weights_loaded) return fail(h, LWP_ERR_STATE, "weights not loaded");
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t packed = h->g.blob_floats * sizeof(float);
    HIP_TRY(h, hipStreamSynchronize(h->stream));         // the copy below is not stream-ordered: a queued lwp_stage_adam_step finishes first
    HIP_TRY(h, hipMemcpy(dst, h->d_blob.as<float>(), packed, hipMemcpyDeviceToDevice));
    if (h->dtype == LWP_F16) {
        uint64_t tag[2];
        f16_blob_tag(h, tag);
        HIP_TRY(h, hipMemcpy((char*)dst + packed, tag, sizeof(tag), hipMemcpyHostToDevice));
    }
    return LWP_OK;
}
extern "C" int lwp_weights_blob_import(lwp_handle h, const void* src, size_t bytes) {
    if (!h || !src || bytes != blob_bytes(h)) return fail(h, LWP_ERR_ARG, "bad blob size (a blob of another dtype or network?)");
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t packed = h->g.blob_floats * sizeof(float);
    if (h->dtype == LWP_F16) {
        uint64_t want[2], got[2];
        f16_blob_tag(h, want);
        HIP_TRY(h, hipMemcpy(got, (const char*)src + packed, sizeof(got), hipMemcpyDeviceToHost));
        if (std::memcmp(want, got, sizeof(want)) != 0) return fail(h, LWP_ERR_ARG, "not an fp16 weight blob of this network");
    }
    HIP_TRY(h, hipStreamSynchronize(h->stream));         // a queued repack must not overwrite the imported stage layers
    HIP_TRY(h, hipMemcpy(h->d_blob.as<float>(), src, packed, hipMemcpyDeviceToDevice));
    h->weights_loaded = true;
    h->raw_loaded = false;
    return LWP_OK;
}

// ---------------------------------------------------------------------------------------------- buffers
static void level_dims(int H, int W, int level, int* h, int* w) {
    int hh = H, ww = W;
    for (int l = 0; l < level; ++l) { hh = (hh - 1) / 2 + 1; ww = (ww - 1) / 2 + 1; }
    *h = hh; *w = ww;
}

static int ensure_activations(lwp_context* h, int N, int H, int W) {
    if (h->cur_N == N && h->cur_H == H && h->cur_W == W) return LWP_OK;
    // Buffers only ever GROW: a caller that alternates shapes (the three scales of val.infer) would otherwise free and
    // re-allocate gigabytes on every call — hipFree / hipMalloc of that size took up to 600 ms on some boxes.
    bool synced = false;
    for (size_t i = 0; i < h->bufs.size(); ++i) {
        int bh, bw;
        level_dims(H, W, h->g.bufs[i].level, &bh, &bw);
        const size_t bytes = (size_t)N * bh * bw * h->g.bufs[i].channels * (h->dtype != LWP_F32 ? 2 : 4);
        if (bytes > h->bufs[i].size()) {
            if (!synced) { HIP_TRY(h, hipStreamSynchronize(h->stream)); synced = true; }
            HIP_TRY(h, h->bufs[i].ensure(bytes));
        }
        // the concat buffer's pad channels are read (with zero weights) but never written: they must hold finite values,
        // and a re-used buffer may hold anything at the new geometry's offsets -> cleared, stream-ordered.  Every other
        // buffer is completely overwritten by its producer before it is read.
        if (h->g.bufs[i].has_pad) HIP_TRY(h, hipMemsetAsync(h->bufs[i].as<void>(), 0, bytes, h->stream));
    }
    h->cur_N = N; h->cur_H = H; h->cur_W = W;
    return LWP_OK;
}

// the default skeleton reads 18 heat-maps and PAF channels up to 37; a custom one was checked against the network by lwp_set_skeleton
static bool skeleton_fits(const lwp_context* h) {
    if (!h->skel.is_default) return true;
    return h->g.NH >= 18 && h->g.NP >= 38;
}

// the result-block pointers of `w`, from frame f0 on: the only place that turns the layout into pointers
static void carve_result_block(PostWorkspace& w, const ResultLayout& l, size_t f0) {
    char* b = (char*)w.result_block;
    auto at = [&](const ResultLayout::Sec& s) { return b + s.off + f0 * s.stride; };
    w.flags = (unsigned long long*)at(l.flags); w.kpts_out = (double*)at(l.kpts_out); w.entries = (double*)at(l.entries);
    w.kpt_count = (int*)at(l.kpt_count); w.n_entries = (int*)at(l.n_entries);
    if (!w.tail) return;
    w.t_conf = (double*)at(l.t_conf); w.t_bbox = (int*)at(l.t_bbox); w.t_kp = (int*)at(l.t_kp); w.t_ids = (int*)at(l.t_ids);
    w.t_n = (int*)at(l.t_n); w.t_near = (unsigned*)at(l.t_near); w.t_last = (int*)at(l.t_last);
}

// THE layout of a workspace's scratch arena: f(field, bytes per frame) for every per-frame array outside the result block, in
// arena order.  It sizes and carves the arena (ensure_ws_obj) and moves a view to a later frame (ws_frames).
template <class F>
static void ws_sections(PostWorkspace& w, F f) {
    const PostCaps& c = w.caps;
    const size_t K = (size_t)w.K, L = (size_t)w.L, E = (size_t)w.E;
    f(w.peak_count, K * 4); f(w.peak_key, K * c.max_peaks * 4); f(w.peak_val, K * c.max_peaks * 4);
    f(w.kpt_xy, K * c.max_kpts * 2 * 4); f(w.kpt_score, K * c.max_kpts * 4);
    f(w.conn_count, L * 4); f(w.conn_ij, L * c.max_conn * 4); f(w.conn_ratio, L * c.max_conn * 8);
    f(w.entries_work, (size_t)c.max_entries * E * 8); f(w.sel_count, L * 4); f(w.seen, (K + L) * 4);
    f(w.sel_ij, L * c.max_kpts * 4); f(w.sel_r, L * c.max_kpts * 8); f(w.sel_sa, L * c.max_kpts * 4); f(w.sel_sb, L * c.max_kpts * 4);
}
// every section starts on a 256-byte boundary of the arena: frame 0 of an array is aligned as an allocation of its own was
static size_t ws_section_bytes(int N, size_t per_frame) { return ((size_t)N * per_frame + 255) & ~(size_t)255; }

static int ensure_ws_obj(lwp_context* h, PostWorkspace& w, lwp_context::WsMem& m, int N, hipStream_t stream) {
    if (w.N >= N && w.peak_count && (w.tail != 0) == (h->tail.mode != 0)) return LWP_OK;
    if (h->tail.mode && h->caps.max_entries > kTailMaxPoses)
        return fail(h, LWP_ERR_ARG, "the pose tail (lwp_set_tracking) holds at most 256 poses per frame: lower max_pose_entries or turn it off");
    HIP_TRY(h, hipStreamSynchronize(stream));
    free_ws_obj(w, m);
    w.caps = h->caps;
    w.K = h->skel.K; w.L = h->skel.L; w.E = h->skel.E;
    w.min_paf = h->skel.min_paf;
    w.generic = (!h->skel.is_default || h->tune.post_generic == 1) ? 1 : 0;
    w.limbs = h->d_limbs.as<int>();
    size_t arena = 0;
    ws_sections(w, [&](auto*&, size_t per) { arena += ws_section_bytes(N, per); });
    HIP_TRY(h, m.arena.ensure(arena));
    char* at = m.arena.as<char>();
    ws_sections(w, [&](auto*& p, size_t per) { p = reinterpret_cast<decltype(+p)>(at); at += ws_section_bytes(N, per); });
    // flags / kpt_count / n_entries / kpts_out / entries live in ONE allocation (result_block) so the fetch is one copy
    w.tail = h->tail.mode ? 1 : 0;
    const ResultLayout lay = result_layout(N, w.K, w.E, w.caps, w.tail != 0);
    HIP_TRY(h, m.block.ensure(lay.bytes));
    w.result_block = m.block.as<void>();
    carve_result_block(w, lay, 0);
    if (w.tail) HIP_TRY(h, hipMemsetAsync((char*)w.result_block + lay.tail_off, 0, lay.bytes - lay.tail_off, stream));
    w.N = N;
    HIP_TRY(h, launch_reset_ws(N, w, stream));
    return LWP_OK;
}
static int ensure_ws(lwp_context* h, int N) { return ensure_ws_obj(h, h->ws, h->ws_mem, N, h->stream); }

static int ensure_host_stage(lwp_context* h, size_t bytes) {
    h->stage_tail_N = 0;                               // every user of h_stage comes through here: the pose rows in it are gone
    HIP_TRY(h, h->h_stage.ensure(bytes));
    return LWP_OK;
}

// ---------------------------------------------------------------------------------------------- profiling hooks
static int prof_begin(lwp_context* h, hipStream_t s, int kclass) {
    if (!h->profiling) return LWP_OK;
    if (h->ev_used + 2 > h->ev.size()) {
        for (int i = 0; i < 2; ++i) {
            Event e;
            HIP_TRY(h, e.ensure());
            h->ev.push_back(std::move(e));
        }
        h->ev_class.resize(h->ev.size() / 2);
        h->ev_layer.resize(h->ev.size() / 2);
    }
    h->ev_class[h->ev_used / 2] = kclass;
    h->ev_layer[h->ev_used / 2] = h->cur_layer;
    HIP_TRY(h, hipEventRecord(h->ev[h->ev_used], s));
    return LWP_OK;
}
static int prof_end(lwp_context* h, hipStream_t s) {
    if (!h->profiling) return LWP_OK;
    HIP_TRY(h, hipEventRecord(h->ev[h->ev_used + 1], s));
    h->ev_used += 2;
    return LWP_OK;
}
// a launch on stream `s`, between two events of that stream while the handle is profiling (else a plain HIP_TRY)
#define LAUNCH_ON(h, s, kclass, expr)              \
    do {                                           \
        int rc_ = prof_begin(h, s, kclass);        \
        if (rc_) return rc_;                       \
        HIP_TRY(h, expr);                          \
        rc_ = prof_end(h, s);                      \
        if (rc_) return rc_;                       \
    } while (0)
#define LAUNCH(h, kclass, expr) LAUNCH_ON(h, (h)->stream, kclass, expr)
// reps profiled runs of enqueue(): per class of its launches, their time per run and (from the first run) their number
template <typename F> static int profile_by_class(lwp_context* h, int n_classes, int reps, float* ms, int* launches, F&& enqueue) {
    for (int k = 0; k < n_classes; ++k) { ms[k] = 0.f; launches[k] = 0; }
    for (int r = 0; r < reps; ++r) {
        h->profiling = true;
        h->ev_used = 0;
        const int rc = enqueue();
        h->profiling = false;
        if (rc) return rc;
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        for (size_t i = 0; i < h->ev_used; i += 2) {
            float t = 0.f;
            HIP_TRY(h, hipEventElapsedTime(&t, h->ev[i], h->ev[i + 1]));
            const int k = h->ev_class[i / 2];
            ms[k] += t;
            if (r == 0) launches[k] += 1;
        }
    }
    for (int k = 0; k < n_classes; ++k) ms[k] /= (float)reps;
    return LWP_OK;
}

// ---------------------------------------------------------------------------------------------- batch split
// The kernels address a tensor with 32-bit byte offsets (buffer loads), so one launch sequence takes at most as many frames
// as keep EVERY tensor of the pass below 2 GiB.  Larger batches are processed in equal chunks inside the entry points — the
// reference's forward takes any N (models/with_mobilenet.py:114) and so does this library.
static int frames_per_pass(lwp_context* h, int N, int H, int W) {
    size_t per = (size_t)3 * H * W * sizeof(float);
    for (const BufSpec& b : h->g.bufs) {
        int bh, bw;
        level_dims(H, W, b.level, &bh, &bw);
        per = std::max(per, (size_t)bh * bw * b.channels * (h->dtype != LWP_F32 ? 2 : 4));
    }
    int fh, fw;
    level_dims(H, W, 3, &fh, &fw);
    per = std::max(per, (size_t)fh * fw * std::max(h->g.NH, h->g.NP) * sizeof(float));
    const size_t lim = ((size_t)1 << 31) - 4096;
    int64_t nmax = std::max<int64_t>(1, (int64_t)(lim / per));
    if (h->tune.max_frames_per_pass > 0) nmax = std::min<int64_t>(nmax, h->tune.max_frames_per_pass);   // tests
    if (N <= nmax) return N;
    const int64_t chunks = (N + nmax - 1) / nmax;
    return (int)((N + chunks - 1) / chunks);
}
// fn(f0, n) for every pass of the batch, the activation buffers sized for the pass's n frames (the last one may be ragged)
template <class F>
static int for_each_pass(lwp_context* h, int N, int H, int W, F fn) {
    const int Nc = frames_per_pass(h, N, H, W);
    for (int f0 = 0; f0 < N; f0 += Nc) {
        const int n = std::min(Nc, N - f0);
        int rc = ensure_activations(h, n, H, W);
        if (rc == LWP_OK) rc = fn(f0, n);
        if (rc) return rc;
    }
    return LWP_OK;
}

// milliseconds the handle's stream spends on `iters` calls of fn
template <class F>
static int time_on_stream(lwp_context* h, int iters, F fn, float* ms) {
    Event a, b;
    HIP_TRY(h, a.ensure());
    HIP_TRY(h, b.ensure());
    HIP_TRY(h, hipEventRecord(a, h->stream));
    for (int i = 0; i < iters; ++i) { int rc = fn(); if (rc) return rc; }
    HIP_TRY(h, hipEventRecord(b, h->stream));
    HIP_TRY(h, hipEventSynchronize(b));
    HIP_TRY(h, hipEventElapsedTime(ms, a, b));
    return LWP_OK;
}

// C channel planes of h x w per frame (NCHW)
static MapView nchw_view(const float* base, int C, int h, int w) {
    const int64_t hw = (int64_t)h * w;
    return MapView{base, C * hw, (int64_t)w, 1, hw, h, w};
}

// the per-frame arrays of a post-processing workspace, seen from frame f0 on (every kernel indexes them by frame)
static PostWorkspace ws_frames(const PostWorkspace& w, int f0) {
    if (f0 == 0) return w;
    PostWorkspace v = w;
    v.N = w.N - f0;
    ws_sections(v, [&](auto*& p, size_t per) { p = reinterpret_cast<decltype(+p)>((char*)p + (size_t)f0 * per); });
    carve_result_block(v, result_layout(w), (size_t)f0);
    return v;
}

// ---------------------------------------------------------------------------------------------- forward
// element-addressed window of an activation buffer (f32, bf16 or fp16 storage)
// (an index past the graph's buffers is a buffer of the retaining plan, TrainPlan: f32, at its BufSpec's level)
static inline float* buf_at(lwp_context* h, const BufRef& r) {
    const int nb = (int)h->g.bufs.size();
    char* base = (r.buf < nb ? h->bufs[r.buf] : h->tbufs[r.buf - nb]).as<char>();
    return (float*)(base + (size_t)r.coff * (h->dtype != LWP_F32 ? 2 : 4));
}
static inline int buf_level(const lwp_context* h, int buf) {
    const int nb = (int)h->g.bufs.size();
    return buf < 0 ? 0 : buf < nb ? h->g.bufs[buf].level : h->tp.bufs[buf - nb].level;
}

static int enqueue_layer(lwp_context* h, const Layer& l, const float* d_in, int N, int H, int W, float* const* d_outs_nchw,
                         const Layer* fold = nullptr, bool* folded = nullptr) {
    const bool h16 = h->dtype != LWP_F32;            // bf16 or fp16: the same launchers, the element type rides in the params
    const int f16 = h->dtype == LWP_F16;
    const float* wts = h->blob(l.w_off);
    const float* bias = h->blob(l.b_off);
    int dh, dw;
    level_dims(H, W, buf_level(h, l.dst.buf), &dh, &dw);
    float* dst = buf_at(h, l.dst);
    char* vb = h->record_variants ? h->variant_buf : nullptr;
    if (vb) vb[0] = 0;
    if (l.kind == L_STEM) {
        StemParams p{d_in, wts, bias, dst, N, H, W, dh, dw, f16, h->d_zeros.as<float>()};
        p.tune = &h->tune; p.variant = vb;
        LAUNCH(h, KC_STEM, h16 ? launch_stem_bf16(p, h->stream) : launch_stem(p, h->stream));
    } else if (l.kind == L_DWPW) {
        int sh, sw;
        level_dims(H, W, buf_level(h, l.src.buf), &sh, &sw);
        DwPwParams p;
        p.in = buf_at(h, l.src); p.in_ld = l.src.ld; p.f16 = f16;
        p.dw_w = wts; p.pw_w = h->blob(l.w2_off); p.pw_b = h->blob(l.b2_off);
        p.out = dst; p.out_ld = l.dst.ld;
        p.res = l.res.buf >= 0 ? buf_at(h, l.res) : nullptr; p.res_ld = l.res.ld;
        p.zeros = h->d_zeros.as<float>();
        p.N = N; p.Hi = sh; p.Wi = sw; p.Ho = dh; p.Wo = dw; p.C = l.cin; p.cout = l.cout;
        p.stride = l.stride; p.dil = l.dil; p.act_dw = l.act; p.act_pw = l.act2;
        p.tune = &h->tune; p.variant = vb;
        LAUNCH(h, KC_PW, h16 ? launch_dwpw_bf16(p, h->stream) : launch_dwpw(p, h->stream));
    } else if (l.kind == L_DW) {
        int sh, sw;
        level_dims(H, W, buf_level(h, l.src.buf), &sh, &sw);
        DwParams p{buf_at(h, l.src), l.src.ld, wts, bias, dst, l.dst.ld, N, sh, sw, dh, dw, l.cin, l.stride, l.dil, l.act};
        p.tune = &h->tune; p.variant = vb;
        LAUNCH(h, KC_DW, launch_dw(p, h->stream));
    } else {
        GemmParams p;
        p.in = buf_at(h, l.src); p.in_ld = l.src.ld; p.f16 = f16;
        p.w = wts; p.bias = bias;
        p.wf = h16 ? nullptr : h->blob(l.w2_off);
        p.out = dst; p.out_ld = l.dst.ld;
        p.res = l.res.buf >= 0 ? buf_at(h, l.res) : nullptr; p.res_ld = l.res.ld;
        p.out_nchw = (l.out_index >= 0 && d_outs_nchw) ? d_outs_nchw[l.out_index] : nullptr;
        p.out_nchw2 = (l.out_index2 >= 0 && d_outs_nchw) ? d_outs_nchw[l.out_index2] : nullptr;
        p.out_split = l.out_split;
        p.zeros = h->d_zeros.as<float>();
        p.N = N; p.H = dh; p.W = dw;
        p.cin_pad = l.cin_pad; p.cout = l.cout; p.cout_pad = l.cout_pad; p.ks = l.ks; p.dil = l.dil; p.act = l.act;
        p.tune = &h->tune; p.variant = vb;
        if (fold) {                                     // the next 1x1 rides in this launch's epilogue if the launcher takes it.  Only the walk
                                                        // passes one: from a fold mark (16-bit graphs only), with `folded` non-null
            p.w2 = h->blob(fold->w_off); p.bias2 = h->blob(fold->b_off);
            p.out2 = buf_at(h, fold->dst); p.out2_ld = fold->dst.ld; p.act2 = fold->act;
            p.fused2 = folded;
        }
        LAUNCH(h, l.ks == 1 ? KC_PW : KC_C3, h16 ? launch_gemm_bf16(p, h->stream) : launch_gemm(p, h->stream));
    }
    if (vb && h->cur_layer >= 0 && h->cur_layer < (int)h->variants.size()) h->variants[h->cur_layer] = vb;
    return LWP_OK;
}

// The run-time half of a marked head pair (Layer::fuse == LWP_MARK_HEADS_PAIR on `a`, `b` the layer behind it): the handle's
// switch (LWP_FUSE_HEADS=0 launches the two GEMMs: A/B, tests) and the head kernels' own size limits at M pixels.
static bool heads_pair_runs(const lwp_context* h, const Layer& a, const Layer& b, int64_t M) {
    if (a.fuse != LWP_MARK_HEADS_PAIR || h->tune.fuse_heads == 0) return false;
    return h->dtype != LWP_F32 ? heads_bf16_supported(a.cin_pad, a.cout_pad, b.cout_pad) : heads_f32_supported(a.cin_pad, a.cout_pad, b.cout_pad, M, &h->tune);
}

static int enqueue_heads_pair(lwp_context* h, const Layer& a, const Layer& b, int N, int H, int W, float* const* d_outs_nchw) {
    int dh, dw;
    level_dims(H, W, buf_level(h, b.dst.buf), &dh, &dw);
    HeadsParams p;
    p.in = buf_at(h, a.src); p.in_ld = a.src.ld; p.f16 = h->dtype == LWP_F16;
    p.w0 = h->blob(a.w_off); p.b0 = h->blob(a.b_off);
    if (h->dtype == LWP_F32) p.w0f = h->blob(a.w2_off);
    p.w1 = h->blob(b.w_off); p.b1 = h->blob(b.b_off);
    p.out = buf_at(h, b.dst); p.out_ld = b.dst.ld;
    p.out_nchw = (b.out_index >= 0 && d_outs_nchw) ? d_outs_nchw[b.out_index] : nullptr;
    p.out_nchw2 = (b.out_index2 >= 0 && d_outs_nchw) ? d_outs_nchw[b.out_index2] : nullptr;
    p.out_split = b.out_split;
    p.N = N; p.H = dh; p.W = dw; p.hidden = a.cout_pad; p.cout = b.cout;
    char* vb = h->record_variants ? h->variant_buf : nullptr;
    if (vb) vb[0] = 0;
    p.tune = &h->tune; p.variant = vb;
    LAUNCH(h, KC_PW, h->dtype != LWP_F32 ? launch_heads_bf16(p, h->stream) : launch_heads_f32(p, h->stream));
    if (vb && h->cur_layer >= 0 && h->cur_layer + 1 < (int)h->variants.size()) { h->variants[h->cur_layer] = vb; h->variants[h->cur_layer + 1] = vb; }
    return LWP_OK;
}

// the depthwise half of an L_DWPW block alone, into train buffer `buf` (the retained copy of lwp_train_forward)
static int enqueue_dw_copy(lwp_context* h, const Layer& l, int buf, int N, int H, int W) {
    int sh, sw, dh, dw;
    level_dims(H, W, buf_level(h, l.src.buf), &sh, &sw);
    level_dims(H, W, buf_level(h, buf), &dh, &dw);
    DwParams p{buf_at(h, l.src), l.src.ld, h->blob(l.w_off), h->blob(l.b_off), h->tbufs[buf - (int)h->g.bufs.size()].as<float>(), l.cin,
               N, sh, sw, dh, dw, l.cin, l.stride, l.dil, l.act};
    p.tune = &h->tune;
    LAUNCH(h, KC_DW, launch_dw(p, h->stream));
    return LWP_OK;
}

// THE walk over a layer list: layers [begin, end) of `ls` (the graph's list, or the retaining plan's) on the handle's stream.
// A step the graph marked as fusable (Layer::fuse) is taken as one launch only if all its layers lie inside the range.
// d_outs_nchw: 2*(1+nref) device pointers or null.  retain (lwp_train_forward): a fused head pair is preceded by a stand-alone
// launch of its first layer, whose hidden tensor the pair's kernel keeps on the CU, for the retained copy.
static int enqueue_forward(lwp_context* h, const std::vector<Layer>& ls, int begin, int end, const float* d_in, int N, int H, int W,
                           float* const* d_outs_nchw, bool retain = false) {
    int fh, fw;
    level_dims(H, W, 3, &fh, &fw);
    const int64_t M3 = (int64_t)N * fh * fw;                 // pixels of the stride-8 maps the heads work on
    int rc = LWP_OK;
    for (int i = begin; i < end && rc == LWP_OK; ++i) {
        h->cur_layer = i;
        const bool inside = i + 1 < end;
        if (inside && heads_pair_runs(h, ls[i], ls[i + 1], M3)) {
            if (retain) rc = enqueue_layer(h, ls[i], d_in, N, H, W, nullptr);
            if (!rc) rc = enqueue_heads_pair(h, ls[i], ls[i + 1], N, H, W, d_outs_nchw);
            ++i;
            continue;
        }
        if (retain && &ls == &h->tp.layers) {
            // cpm tensors a fused launch never stores (LWP_TRAIN_CPM): the depthwise half of an L_DWPW block from a stand-alone
            // launch_dw on the block's input, the pointwise output in front of the residual add from the same launch without it
            if (h->tp.dw_copy[i] >= 0) {
                rc = enqueue_dw_copy(h, ls[i], h->tp.dw_copy[i], N, H, W);
                if (rc) break;
            }
            if (h->tp.nores_copy[i] >= 0) {
                Layer c = ls[i];
                c.res = BufRef();
                c.dst.buf = h->tp.nores_copy[i]; c.dst.coff = 0;
                c.out_index = c.out_index2 = -1;
                rc = enqueue_layer(h, c, d_in, N, H, W, nullptr);
                if (rc) break;
            }
        }
        // a marked 1x1 rides in this 3x3's epilogue if the launcher takes it (GemmParams::fused2)
        bool folded = false;
        rc = enqueue_layer(h, ls[i], d_in, N, H, W, d_outs_nchw, inside && ls[i].fuse == LWP_MARK_FOLD_NEXT_1X1 ? &ls[i + 1] : nullptr, &folded);
        if (!rc && folded) {
            if (h->record_variants && (size_t)i + 1 < h->variants.size()) h->variants[i + 1] = h->variants[i];
            ++i;
        }
    }
    h->cur_layer = -1;
    return rc;
}
// the whole network
static int enqueue_network(lwp_context* h, const float* d_in, int N, int H, int W, float* const* d_outs_nchw) {
    return enqueue_forward(h, h->g.layers, 0, (int)h->g.layers.size(), d_in, N, H, W, d_outs_nchw);
}

static int check_frame_shape(lwp_context* h, int N, int H, int W) {
    if (N <= 0 || H <= 0 || W <= 0) return fail(h, LWP_ERR_ARG, "bad frame shape");
    if (H < 8 || W < 8) return fail(h, LWP_ERR_ARG, "frame too small (H, W >= 8)");
    if (!h->weights_loaded) return fail(h, LWP_ERR_STATE, "weights not loaded (call lwp_load_weights first)");
    return LWP_OK;
}

static int stage_input(lwp_context* h, const float* in, int in_mem, size_t bytes, const float** d_in) {
    if (in_mem == LWP_MEM_DEVICE) { *d_in = in; return LWP_OK; }
    HIP_TRY(h, h->d_in.ensure(bytes));
    HIP_TRY(h, hipMemcpyAsync(h->d_in.as<float>(), in, bytes, hipMemcpyHostToDevice, h->stream));
    *d_in = h->d_in.as<float>();
    return LWP_OK;
}

extern "C" int lwp_forward(lwp_handle h, const float* in, int in_mem, int N, int H, int W, float* const* outs, int out_mem) {
    if (!h || !in || !outs) return fail(h, LWP_ERR_ARG, "null argument");
    int rc = check_frame_shape(h, N, H, W);
    if (rc) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    rc = ensure_activations(h, frames_per_pass(h, N, H, W), H, W);   // frames per launch sequence: N unless a tensor would reach 2 GiB
    if (rc) return rc;
    if (in_mem == LWP_MEM_DEVICE || out_mem == LWP_MEM_DEVICE) { rc = order_in(h); if (rc) return rc; }
    const float* d_in = nullptr;
    rc = stage_input(h, in, in_mem, (size_t)N * 3 * H * W * sizeof(float), &d_in);
    if (rc) return rc;
    const int nout = 2 * (1 + h->g.nref);
    int fh, fw;
    level_dims(H, W, 3, &fh, &fw);               // three stride-2 stages: out = (in - 1) / 2 + 1 each
    std::vector<float*> d_outs(nout), d_chunk(nout);
    for (int i = 0; i < nout; ++i) {
        if (!outs[i]) return fail(h, LWP_ERR_ARG, "null output pointer");
        if (out_mem == LWP_MEM_DEVICE) { d_outs[i] = outs[i]; continue; }
        const size_t bytes = (size_t)N * (i % 2 ? h->g.NP : h->g.NH) * fh * fw * sizeof(float);
        HIP_TRY(h, h->d_outs[i].ensure(bytes));
        d_outs[i] = h->d_outs[i].as<float>();
    }
    rc = for_each_pass(h, N, H, W, [&](int f0, int n) {
        for (int i = 0; i < nout; ++i) d_chunk[i] = d_outs[i] + (size_t)f0 * (i % 2 ? h->g.NP : h->g.NH) * fh * fw;
        return enqueue_network(h, d_in + (size_t)f0 * 3 * H * W, n, H, W, d_chunk.data());
    });
    if (rc) return rc;
    if (out_mem == LWP_MEM_HOST) {
        for (int i = 0; i < nout; ++i) {
            const size_t bytes = (size_t)N * (i % 2 ? h->g.NP : h->g.NH) * fh * fw * sizeof(float);
            HIP_TRY(h, hipMemcpyAsync(outs[i], d_outs[i], bytes, hipMemcpyDeviceToHost, h->stream));
        }
        HIP_TRY(h, hipStreamSynchronize(h->stream));
    } else {
        bool ordered = false;
        rc = order_out(h, h->stream, &ordered);          // the caller's stream waits for the outputs; without lwp_set_stream the
        if (rc) return rc;                               // caller synchronises (lwp_synchronize) before touching them
    }
    return LWP_OK;
}

// ---------------------------------------------------------------------------------------------- upsample
extern "C" int lwp_upsample(lwp_handle h, const float* src, int src_mem, int N, int C, int hs, int ws, int ratio, float* dst, int dst_mem) {
    if (!h || !src || !dst || N <= 0 || C <= 0 || hs <= 0 || ws <= 0) return fail(h, LWP_ERR_ARG, "bad argument");
    if (ratio != 4 && ratio != 8) return fail(h, LWP_ERR_ARG, "upsample ratio must be 4 or 8");
    HIP_TRY(h, hipSetDevice(h->device));
    if (src_mem == LWP_MEM_DEVICE || dst_mem == LWP_MEM_DEVICE) { int rc0 = order_in(h); if (rc0) return rc0; }
    const size_t sb = (size_t)N * C * hs * ws * sizeof(float), db = sb * ratio * ratio;
    const float* d_src = src;
    if (src_mem == LWP_MEM_HOST) {
        HIP_TRY(h, h->d_tmp.ensure(sb));
        HIP_TRY(h, hipMemcpyAsync(h->d_tmp.as<float>(), src, sb, hipMemcpyHostToDevice, h->stream));
        d_src = h->d_tmp.as<float>();
    }
    float* d_dst = dst;
    if (dst_mem == LWP_MEM_HOST) {
        HIP_TRY(h, h->d_tmp2.ensure(db));
        d_dst = h->d_tmp2.as<float>();
    }
    const MapView v = nchw_view(d_src, C, hs, ws);
    LAUNCH(h, KC_POST, launch_upsample(v, N, C, ratio, d_dst, h->stream, &h->tune));
    if (dst_mem == LWP_MEM_HOST) {
        HIP_TRY(h, hipMemcpyAsync(dst, d_dst, db, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
    } else {
        bool ordered = false;
        int rc1 = order_out(h, h->stream, &ordered);
        if (rc1) return rc1;
    }
    return LWP_OK;
}

// ---------------------------------------------------------------------------------------------- resize-table cache
constexpr size_t kTabCacheMax = 16;
static lwp_context::ResizeTab* find_tab(lwp_context::TabCache& cache, const lwp_context::TabKey& key) {
    for (auto& rt : cache) if (rt.key == key) return &rt;
    return nullptr;
}
// A new geometry's tables: the four host arrays (4-byte elements; nx = 4 * destination width, ny = 4 * destination height),
// uploaded back to back into one allocation (blocking copies: a steady-state call issues none).  The cache is bounded: the
// oldest geometry goes first, once nothing queued can read it.  The entry is inserted only after the upload succeeded.
static int add_tab(lwp_context* h, lwp_context::TabCache& cache, const lwp_context::TabKey& key, const lwp_context::MsPlan& plan,
                   size_t nx, size_t ny, const void* xi, const void* xw, const void* yi, const void* yw, lwp_context::ResizeTab** out) {
    if (cache.size() >= kTabCacheMax) {
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        cache.erase(cache.begin());
    }
    lwp_context::ResizeTab rt{key, DevBuf(), plan, nx, ny};
    HIP_TRY(h, rt.d.ensure((nx + ny) * 8));
    const auto t = rt.arrays<int>();                     // (4-byte elements whatever the weights' type)
    HIP_TRY(h, hipMemcpy(t.xi, xi, nx * 4, hipMemcpyHostToDevice));
    HIP_TRY(h, hipMemcpy(t.xw, xw, nx * 4, hipMemcpyHostToDevice));
    HIP_TRY(h, hipMemcpy(t.yi, yi, ny * 4, hipMemcpyHostToDevice));
    HIP_TRY(h, hipMemcpy(t.yw, yw, ny * 4, hipMemcpyHostToDevice));
    cache.push_back(std::move(rt));
    *out = &cache.back();
    return LWP_OK;
}

// ---------------------------------------------------------------------------------------------- multi-scale accumulate
extern "C" int lwp_multiscale_accumulate(lwp_handle h, const float* maps, int maps_mem, int N, int C, int hs, int ws, int up_ratio,
                                         const int* pad, int dst_h, int dst_w, int n_scales, float* accum, int accum_mem, int init) {
    if (!h || !maps || !pad || !accum || N <= 0 || C <= 0 || hs <= 0 || ws <= 0 || dst_h <= 0 || dst_w <= 0 || n_scales <= 0)
        return fail(h, LWP_ERR_ARG, "bad argument");
    if (up_ratio != 4 && up_ratio != 8) return fail(h, LWP_ERR_ARG, "upsample ratio must be 4 or 8");
    const int Hs = hs * up_ratio, Ws = ws * up_ratio;
    const int ch = Hs - pad[0] - pad[2], cw = Ws - pad[1] - pad[3];
    if (pad[0] < 0 || pad[1] < 0 || pad[2] < 0 || pad[3] < 0 || ch <= 0 || cw <= 0) return fail(h, LWP_ERR_ARG, "bad crop");
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t sb = (size_t)N * C * hs * ws * sizeof(float), ub = sb * up_ratio * up_ratio, ab = (size_t)N * dst_h * dst_w * C * sizeof(float);
    const float* d_src = maps;
    int rc;
    if (maps_mem == LWP_MEM_DEVICE || accum_mem == LWP_MEM_DEVICE) { rc = order_in(h); if (rc) return rc; }
    if (maps_mem == LWP_MEM_HOST) {
        HIP_TRY(h, h->d_tmp.ensure(sb));
        HIP_TRY(h, hipMemcpyAsync(h->d_tmp.as<float>(), maps, sb, hipMemcpyHostToDevice, h->stream));
        d_src = h->d_tmp.as<float>();
    }
    float* d_acc = accum;
    if (accum_mem == LWP_MEM_HOST) {
        HIP_TRY(h, h->d_maps[0].ensure(ab));
        if (!init) HIP_TRY(h, hipMemcpyAsync(h->d_maps[0].as<float>(), accum, ab, hipMemcpyHostToDevice, h->stream));
        d_acc = h->d_maps[0].as<float>();
    }
    // per-geometry tables, uploaded once (blocking copy) and kept: steady-state calls issue no host->device copy
    const lwp_context::TabKey key{cw, ch, dst_w, dst_h, 0.0, up_ratio};
    lwp_context::ResizeTab* tab = find_tab(h->resize_tabs, key);
    if (!tab) {
        std::vector<int> xi, yi;
        std::vector<float> xw, yw;
        build_resize_table(cw, dst_w, xi, xw);
        build_resize_table(ch, dst_h, yi, yw);
        lwp_context::MsPlan pl;
        if (h->tune.ms_tx >= 8 && h->tune.ms_tx <= 40) {   // LWP_MS_TX: a forced tile width (tests, A/B)
            pl.tx = h->tune.ms_tx;
            multiscale_fused_extent(xi.data(), yi.data(), dst_h, dst_w, pl.tx, &pl.uh_max, &pl.uw_max);
            pl.tx4 = pl.tx; pl.uh4 = pl.uh_max; pl.uw4 = pl.uw_max;
        } else {
            multiscale_fused_plan(xi.data(), yi.data(), dst_h, dst_w, up_ratio, &pl.tx, &pl.uh_max, &pl.uw_max);
            multiscale_fused_plan_v4(xi.data(), yi.data(), dst_h, dst_w, up_ratio, &pl.tx4, &pl.uh4, &pl.uw4);
        }
        rc = add_tab(h, h->resize_tabs, key, pl, (size_t)dst_w * 4, (size_t)dst_h * 4, xi.data(), xw.data(), yi.data(), yw.data(), &tab);
        if (rc) return rc;
    }
    const lwp_context::MsPlan& pl = tab->plan;
    const auto t = tab->arrays<float>();
    const MapView v = nchw_view(d_src, C, hs, ws);
    bool fused = false;
    if (h->tune.ms_fused != 0 && h->tune.ms_vec != 0) {      // four channels per lane (LWP_MS_VEC=0: the scalar fused kernel)
        LAUNCH(h, KC_POST, launch_multiscale_fused_v4(v, N, C, up_ratio, pad[0], pad[1], t.xi, t.xw, t.yi, t.yw, dst_h, dst_w, (float)n_scales, init ? 1 : 0,
                                                      d_acc, pl.tx4, pl.uh4, pl.uw4, h->stream, &fused));
    }
    if (!fused && h->tune.ms_fused != 0) {                   // LWP_MS_FUSED=0: the two-kernel form (A/B, tests)
        LAUNCH(h, KC_POST, launch_multiscale_fused(v, N, C, up_ratio, pad[0], pad[1], t.xi, t.xw, t.yi, t.yw, dst_h, dst_w, (float)n_scales, init ? 1 : 0,
                                                   d_acc, pl.tx, pl.uh_max, pl.uw_max, h->stream, &fused));
    }
    if (!fused) {
        HIP_TRY(h, h->d_tmp2.ensure(ub));
        LAUNCH(h, KC_POST, launch_upsample(v, N, C, up_ratio, h->d_tmp2.as<float>(), h->stream, &h->tune));
        LAUNCH(h, KC_POST, launch_resize_accum(h->d_tmp2.as<float>(), N, Hs, Ws, C, pad[0], pad[1], t.xi, t.xw, t.yi, t.yw, dst_h, dst_w, (float)n_scales, init ? 1 : 0, d_acc, h->stream));
    }
    if (accum_mem == LWP_MEM_HOST) HIP_TRY(h, hipMemcpyAsync(accum, d_acc, ab, hipMemcpyDeviceToHost, h->stream));
    bool ordered = false;
    if (accum_mem == LWP_MEM_DEVICE) { rc = order_out(h, h->stream, &ordered); if (rc) return rc; }
    // without lwp_set_stream the results are complete on return (callers read accum on other streams)
    if (!ordered) HIP_TRY(h, hipStreamSynchronize(h->stream));
    return LWP_OK;
}

// ---------------------------------------------------------------------------------------------- pre-processing
// THE padding rule, val.py:36-49 with min_dims = [base, max(dw, base)] (demo.py:61, val.py:90): the scaled dh x dw frame centred
// in base x max(dw, base), both rounded up to the stride
static void pad_rule(int dh, int dw, int base, int stride, int* pad, int* out_h, int* out_w) {
    const int h = dh < base ? dh : base;
    const int min0 = (int)ceil(base / (double)stride) * stride;
    const int m1 = dw > base ? dw : base;
    const int min1 = (int)ceil(m1 / (double)stride) * stride;
    pad[0] = (int)floor((min0 - h) / 2.0);
    pad[1] = (int)floor((min1 - dw) / 2.0);
    pad[2] = min0 - h - pad[0];
    pad[3] = min1 - dw - pad[1];
    *out_h = dh + pad[0] + pad[2];
    *out_w = dw + pad[1] + pad[3];
}

extern "C" int lwp_preprocess_dims(int H, int W, int net_input_height, int stride, int* scaled_h, int* scaled_w,
                                   int* out_h, int* out_w, int* pad, double* scale) {
    if (H <= 0 || W <= 0 || net_input_height <= 0 || stride <= 0 || !scaled_h || !scaled_w || !out_h || !out_w || !pad || !scale)
        return fail(nullptr, LWP_ERR_ARG, "bad argument");
    const double sc = (double)net_input_height / (double)H;                       // demo.py:57
    const int dw = (int)nearbyint((double)W * sc), dh = (int)nearbyint((double)H * sc);   // cv2 dsize: round half to even
    if (dw <= 0 || dh <= 0) return fail(nullptr, LWP_ERR_ARG, "scaled frame is empty");
    pad_rule(dh, dw, net_input_height, stride, pad, out_h, out_w);
    *scaled_h = dh; *scaled_w = dw;
    *scale = sc;
    return LWP_OK;
}

// Host frames -> the device buffer `dst` on the handle's stream.  Up to kPinLimit bytes: memcpy (calling thread) into one of two
// pinned staging buffers, then an asynchronous DMA — the caller's buffer is free when this returns (*consumed = true) and the
// call need not wait for the copy; the staging buffer is reused only after the DMA that read it has finished (its event).
// Larger batches: a plain asynchronous copy from the caller's memory (*consumed = false: the caller must wait for ev_copy).
constexpr size_t kPinLimit = (size_t)64 << 20;
static int upload_host(lwp_context* h, const void* src, size_t bytes, void* dst, bool* consumed) {
    *consumed = false;
    if (bytes <= kPinLimit) {
        const int k = h->pin_next;
        h->pin_next ^= 1;
        if (h->pin_busy[k]) { HIP_TRY(h, hipEventSynchronize(h->pin_ev[k])); h->pin_busy[k] = false; }
        HIP_TRY(h, h->pin_buf[k].ensure(bytes));
        HIP_TRY(h, h->pin_ev[k].ensure(hipEventDisableTiming));
        void* pin = h->pin_buf[k].as<void>();
        std::memcpy(pin, src, bytes);
        if (h->tune.host_fetch_dma == 1) {                   // LWP_HOST_FETCH_DMA=1: the copy engine instead of the fetch kernel (A/B)
            HIP_TRY(h, hipMemcpyAsync(dst, pin, bytes, hipMemcpyHostToDevice, h->stream));
        } else {
            void* mapped = nullptr;
            HIP_TRY(h, hipHostGetDevicePointer(&mapped, pin, 0));
            HIP_TRY(h, launch_fetch_host(mapped, dst, bytes, h->stream));
        }
        HIP_TRY(h, hipEventRecord(h->pin_ev[k], h->stream));
        h->pin_busy[k] = true;
        *consumed = true;
        return LWP_OK;
    }
    HIP_TRY(h, h->ev_copy.ensure(hipEventDisableTiming));
    HIP_TRY(h, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipEventRecord(h->ev_copy, h->stream));
    return LWP_OK;
}

// Frames for a kernel on the main stream: device frames are read where they are; host frames go through upload_host (which
// reports *consumed) into the shared staging, read on the main stream only, or into own_dst, a device buffer of the caller's.
// *consumed is written for host frames only: the caller initialises it to what its epilogue needs for device frames
static int stage_frames(lwp_context* h, const void* imgs, int img_mem, size_t ib, const void** d_src, bool* consumed,
                        unsigned char* own_dst = nullptr) {
    *d_src = imgs;
    if (img_mem != LWP_MEM_HOST) return LWP_OK;
    if (!own_dst && h->d_imgs.size() < ib) {
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        HIP_TRY(h, h->d_imgs.ensure(ib));
    }
    unsigned char* dst = own_dst ? own_dst : h->d_imgs.as<unsigned char>();
    *d_src = dst;
    return upload_host(h, imgs, ib, dst, consumed);
}

// ---- the uint8 front end (demo.py:57-64): geometry, device tables, kernel parameters and epilogue of lwp_preprocess_u8,
//      lwp_preprocess_u8_batch and lwp_pipeline_submit_u8
struct PreGeom { int dh, dw, Hp, Wp, pad[4]; double sc; };

// device tables of a geometry, built and uploaded once and then only read
static int pre_tables(lwp_context* h, int H, int W, const PreGeom& g, const lwp_context::ResizeTab** tab) {
    const lwp_context::TabKey key{W, H, g.dw, g.dh, g.sc, 0};
    lwp_context::ResizeTab* rt = find_tab(h->pre_tabs, key);
    if (!rt) {
        std::vector<int> xi, xw, yi, yw;
        build_resize_table_u8(W, g.dw, g.sc, xi, xw);
        build_resize_table_u8(H, g.dh, g.sc, yi, yw);
        int rc = add_tab(h, h->pre_tabs, key, {}, (size_t)g.dw * 4, (size_t)g.dh * 4, xi.data(), xw.data(), yi.data(), yw.data(), &rt);
        if (rc) return rc;
    }
    *tab = rt;
    return LWP_OK;
}

static PreprocParams preproc_params(const void* d_src, int H, int W, const PreGeom& g, const lwp_context::ResizeTab& tab,
                                    const double* pad_value, const double* img_mean, double img_scale, float* out) {
    const auto t = tab.arrays<int>();
    PreprocParams p;
    p.src = (const unsigned char*)d_src; p.Hs = H; p.Ws = W;
    p.xi = t.xi; p.xw = t.xw; p.yi = t.yi; p.yw = t.yw;
    p.dh = g.dh; p.dw = g.dw; p.top = g.pad[0]; p.left = g.pad[1]; p.Hp = g.Hp; p.Wp = g.Wp;
    for (int c = 0; c < 3; ++c) { p.mean[c] = img_mean[c]; p.pad_value[c] = (float)pad_value[c]; }
    p.scale = img_scale;
    p.out = out;
    return p;
}

// The caller may reuse its host frame buffer on return: it has been copied into the pinned staging buffer already (or, for
// very large batches, the COPY is waited for); the kernel's output is stream-ordered (consumed by this handle's next call, or
// by the caller's stream after the event hand-over).  Without a declared caller stream the call completes on return.
static int finish_u8(lwp_context* h, int img_mem, bool consumed) {
    bool ordered = false;
    int rc = order_out(h, h->stream, &ordered);
    if (rc) return rc;
    if (img_mem == LWP_MEM_HOST) {
        if (!ordered) HIP_TRY(h, hipStreamSynchronize(h->stream));
        else if (!consumed) HIP_TRY(h, hipEventSynchronize(h->ev_copy));
    }
    return LWP_OK;
}

extern "C" int lwp_preprocess_u8(lwp_handle h, const unsigned char* img, int img_mem, int H, int W, int net_input_height,
                                 int stride, const double* pad_value, const double* img_mean, double img_scale, float* out_device) {
    if (!h || !img || !pad_value || !img_mean || !out_device) return fail(h, LWP_ERR_ARG, "null argument");
    PreGeom g;
    int rc = lwp_preprocess_dims(H, W, net_input_height, stride, &g.dh, &g.dw, &g.Hp, &g.Wp, g.pad, &g.sc);
    if (rc) return fail(h, rc, "bad frame / network size");
    if (g.pad[0] < 0 || g.pad[1] < 0 || g.pad[2] < 0 || g.pad[3] < 0) return fail(h, LWP_ERR_ARG, "negative padding");
    HIP_TRY(h, hipSetDevice(h->device));
    rc = order_in(h);                                    // device frame produced / output buffer last used on the caller's stream
    if (rc) return rc;
    const void* d_src = nullptr;
    bool consumed = false;
    rc = stage_frames(h, img, img_mem, (size_t)H * W * 3, &d_src, &consumed);
    if (rc) return rc;
    const lwp_context::ResizeTab* tab = nullptr;
    rc = pre_tables(h, H, W, g, &tab);
    if (rc) return rc;
    LAUNCH(h, KC_POST, launch_preprocess_u8(preproc_params(d_src, H, W, g, *tab, pad_value, img_mean, img_scale, out_device), h->stream));
    return finish_u8(h, img_mem, consumed);
}

// ---------------------------------------------------------------------------------------------- multi-scale image side
extern "C" int lwp_scale_dims(int H, int W, double ratio, int base_height, int stride, int* scaled_h, int* scaled_w,
                              int* out_h, int* out_w, int* pad) {
    if (H <= 0 || W <= 0 || !(ratio > 0.0) || base_height <= 0 || stride <= 0 || !scaled_h || !scaled_w || !out_h || !out_w || !pad)
        return fail(nullptr, LWP_ERR_ARG, "bad argument");
    const double fw = nearbyint((double)W * ratio), fh = nearbyint((double)H * ratio);   // cv2 dsize: round half to even
    if (!(fw >= 1.0 && fh >= 1.0 && fw <= 65535.0 && fh <= 65535.0)) return fail(nullptr, LWP_ERR_ARG, "scaled frame is empty or too large");
    const int dw = (int)fw, dh = (int)fh;
    pad_rule(dh, dw, base_height, stride, pad, out_h, out_w);
    *scaled_h = dh; *scaled_w = dw;
    return LWP_OK;
}

static int preprocess_scaled_impl(lwp_handle h, const void* imgs, int elem, int img_mem, int N, int H, int W, double ratio,
                                  int base_height, int stride, const double* pad_value, const double* img_mean,
                                  double img_scale, float* out_device);
extern "C" int lwp_preprocess_scaled_u8(lwp_handle h, const unsigned char* imgs, int img_mem, int N, int H, int W, double ratio,
                                        int base_height, int stride, const double* pad_value, const double* img_mean,
                                        double img_scale, float* out_device) {
    return preprocess_scaled_impl(h, imgs, 1, img_mem, N, H, W, ratio, base_height, stride, pad_value, img_mean, img_scale, out_device);
}
extern "C" int lwp_preprocess_scaled_f32(lwp_handle h, const float* imgs, int img_mem, int N, int H, int W, double ratio,
                                         int base_height, int stride, const double* pad_value, const double* img_mean,
                                         double img_scale, float* out_device) {
    return preprocess_scaled_impl(h, imgs, 4, img_mem, N, H, W, ratio, base_height, stride, pad_value, img_mean, img_scale, out_device);
}
static int preprocess_scaled_impl(lwp_handle h, const void* imgs, int elem, int img_mem, int N, int H, int W, double ratio,
                                  int base_height, int stride, const double* pad_value, const double* img_mean,
                                  double img_scale, float* out_device) {
    if (!h || !imgs || !pad_value || !img_mean || !out_device || N <= 0) return fail(h, LWP_ERR_ARG, "bad argument");
    int dh, dw, Hp, Wp, pad[4];
    int rc = lwp_scale_dims(H, W, ratio, base_height, stride, &dh, &dw, &Hp, &Wp, pad);
    if (rc) return fail(h, rc, "bad frame size / scale ratio");
    if (pad[0] < 0 || pad[1] < 0 || pad[2] < 0 || pad[3] < 0) return fail(h, LWP_ERR_ARG, "negative padding");
    HIP_TRY(h, hipSetDevice(h->device));
    rc = order_in(h);
    if (rc) return rc;
    const void* d_src = nullptr;
    bool consumed = false;
    rc = stage_frames(h, imgs, img_mem, (size_t)N * H * W * 3 * elem, &d_src, &consumed);
    if (rc) return rc;
    const lwp_context::TabKey key{W, H, dw, dh, ratio, 0};
    lwp_context::ResizeTab* tab = find_tab(h->scale_tabs, key);
    if (!tab) {                                          // per-geometry tables, uploaded once and kept
        std::vector<int> xi, yi;
        std::vector<float> xw, yw;
        build_resize_table_ratio(W, dw, ratio, xi, xw);
        build_resize_table_ratio(H, dh, ratio, yi, yw);
        rc = add_tab(h, h->scale_tabs, key, {}, (size_t)dw * 4, (size_t)dh * 4, xi.data(), xw.data(), yi.data(), yw.data(), &tab);
        if (rc) return rc;
    }
    const auto t = tab->arrays<float>();
    PreScaleParams p;
    p.src = d_src; p.src_f32 = elem == 4; p.N = N; p.Hs = H; p.Ws = W;
    p.xi = t.xi; p.xw = t.xw; p.yi = t.yi; p.yw = t.yw;
    p.dh = dh; p.dw = dw; p.top = pad[0]; p.left = pad[1]; p.Hp = Hp; p.Wp = Wp;
    for (int c = 0; c < 3; ++c) { p.mean[c] = img_mean[c]; p.pad_value[c] = (float)pad_value[c]; }
    p.scale = img_scale;
    p.out = out_device;
    LAUNCH(h, KC_POST, launch_preprocess_scaled(p, h->stream));
    bool ordered = false;
    rc = order_out(h, h->stream, &ordered);
    if (rc) return rc;
    if (!ordered) HIP_TRY(h, hipStreamSynchronize(h->stream));                    // no declared caller stream: complete on return
    else if (img_mem == LWP_MEM_HOST && !consumed) HIP_TRY(h, hipEventSynchronize(h->ev_copy));   // host frames may be reused: the copy only
    return LWP_OK;
}

// ---------------------------------------------------------------------------------------------- extract_keypoints
extern "C" int lwp_extract_keypoints(lwp_handle h, float* heatmap, int H, int W, int64_t row_stride, int64_t pix_stride,
                                     int64_t* xs, int64_t* ys, float* scores, int cap, int* count) {
    if (!h || !heatmap || !xs || !ys || !scores || !count || H <= 0 || W <= 0 || cap < 0) return fail(h, LWP_ERR_ARG, "bad argument");
    if (H > 65535 || W > 65535) return fail(h, LWP_ERR_ARG, "map too large");
    HIP_TRY(h, hipSetDevice(h->device));
    int rc = ensure_ws(h, 1);
    if (rc) return rc;
    const size_t bytes = (size_t)H * W * sizeof(float);
    rc = ensure_host_stage(h, bytes + (size_t)h->caps.max_kpts * 12 + 64);
    if (rc) return rc;
    HIP_TRY(h, h->d_tmp.ensure(bytes));
    float* hs = h->h_stage.as<float>();
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) hs[(size_t)y * W + x] = heatmap[y * row_stride + x * pix_stride];
    HIP_TRY(h, hipMemcpyAsync(h->d_tmp.as<float>(), hs, bytes, hipMemcpyHostToDevice, h->stream));
    LAUNCH(h, KC_POST, launch_reset_ws(1, h->ws, h->stream));
    LAUNCH(h, KC_POST, launch_threshold_inplace(h->d_tmp.as<float>(), (int64_t)H * W, h->stream));
    MapView v{h->d_tmp.as<float>(), 0, (int64_t)W, 1, 0, H, W};
    LAUNCH(h, KC_POST, launch_find_peaks(v, 1, 1, 1, h->ws, h->stream, &h->tune));
    LAUNCH(h, KC_POST, launch_nms(1, 1, H, h->ws, h->stream));
    HIP_TRY(h, hipMemcpyAsync(hs, h->d_tmp.as<float>(), bytes, hipMemcpyDeviceToHost, h->stream));
    int* h_xy = (int*)(h->h_stage.as<char>() + bytes);
    float* h_sc = (float*)(h_xy + (size_t)h->caps.max_kpts * 2);
    int n = 0;
    unsigned long long fl = 0;
    HIP_TRY(h, hipMemcpyAsync(h_xy, h->ws.kpt_xy, (size_t)h->caps.max_kpts * 2 * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipMemcpyAsync(h_sc, h->ws.kpt_score, (size_t)h->caps.max_kpts * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipMemcpyAsync(&n, h->ws.kpt_count, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipMemcpyAsync(&fl, h->ws.flags, sizeof(fl), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, launch_reset_ws(1, h->ws, h->stream));   // leave the append counters zeroed (the fused path relies on it)
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) heatmap[y * row_stride + x * pix_stride] = hs[(size_t)y * W + x];
    if (fl & 3ull) return fail(h, LWP_ERR_CAPACITY, "extract_keypoints: peak or key-point capacity exceeded (lwp_set_capacity)");
    if (n > cap) return fail(h, LWP_ERR_CAPACITY, "extract_keypoints: output arrays too small");
    for (int i = 0; i < n; ++i) { xs[i] = h_xy[2 * i]; ys[i] = h_xy[2 * i + 1]; scores[i] = h_sc[i]; }
    *count = n;
    return LWP_OK;
}

// ---------------------------------------------------------------------------------------------- results
static int parse_results(lwp_context* h, const PostWorkspace& ws, const void* host_block, int N, int* kpt_counts, double* kpts,
                         int kpt_cap, double* entries, int entry_cap, int* n_entries);

static int fetch_results(lwp_context* h, int N, int* kpt_counts, double* kpts, int kpt_cap, double* entries, int entry_cap, int* n_entries) {
    int rc = ensure_host_stage(h, result_layout(h->ws).bytes + 64);
    if (rc) return rc;
    h->stage_tail_N = 0;
    HIP_TRY(h, launch_publish(N, h->ws, h->h_stage.as<void>(), h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    rc = parse_results(h, h->ws, h->h_stage.as<void>(), N, kpt_counts, kpts, kpt_cap, entries, entry_cap, n_entries);
    if (rc == LWP_OK && h->ws.tail && h->run_has_tail) h->stage_tail_N = N;
    return rc;
}

static int parse_results(lwp_context* h, const PostWorkspace& ws, const void* host_block, int N, int* kpt_counts, double* kpts,
                         int kpt_cap, double* entries, int entry_cap, int* n_entries) {
    const PostCaps& c = ws.caps;
    const ResultLayout l = result_layout(ws);    // the block is laid out for the workspace's frame capacity
    const char* p = (const char*)host_block;
    const unsigned long long* h_fl = (const unsigned long long*)(p + l.flags.off);
    const int K = ws.K, E = ws.E;
    const double* h_k = (const double*)(p + l.kpts_out.off);
    const double* h_e = (const double*)(p + l.entries.off);
    const int* h_cnt = (const int*)(p + l.kpt_count.off);
    const int* h_ne = (const int*)(p + l.n_entries.off);
    for (int f = 0; f < N; ++f) {
        if (h_fl[f * 4 + 0]) {
            char msg[160];
            snprintf(msg, sizeof msg, "frame %d: post-processing capacity exceeded (bits 0x%llx: 1 peaks, 2 key-points, 4 connections/entries)", f, h_fl[f * 4]);
            return fail(h, LWP_ERR_CAPACITY, msg);
        }
        if (h_fl[f * 4 + 1] < h_fl[f * 4 + 2])
            return fail(h, LWP_ERR_UNBOUND, "local variable 'ratio' referenced before assignment");
        int total = 0;
        for (int t = 0; t < K; ++t) { kpt_counts[f * K + t] = h_cnt[f * K + t]; total += h_cnt[f * K + t]; }
        if (total > kpt_cap || h_ne[f] > entry_cap) return fail(h, LWP_ERR_CAPACITY, "result arrays too small");
        std::memcpy(kpts + (size_t)f * kpt_cap * 4, h_k + (size_t)f * K * c.max_kpts * 4, (size_t)total * 4 * sizeof(double));
        std::memcpy(entries + (size_t)f * entry_cap * E, h_e + (size_t)f * c.max_entries * E, (size_t)h_ne[f] * E * sizeof(double));
        n_entries[f] = h_ne[f];
    }
    return LWP_OK;
}

// ---------------------------------------------------------------------------------------------- group_keypoints
extern "C" int lwp_group_keypoints(lwp_handle h, const double* kpts, const int* type_counts, const float* pafs, int pafs_mem,
                                   int H, int W, int demo, double* pose_entries, int cap_entries, int* n_entries) {
    if (!h || !type_counts || !pafs || !pose_entries || !n_entries || H <= 0 || W <= 0) return fail(h, LWP_ERR_ARG, "bad argument");
    HIP_TRY(h, hipSetDevice(h->device));
    int rc = ensure_ws(h, 1);
    if (rc) return rc;
    const PostCaps& c = h->ws.caps;
    const int K = h->ws.K;
    int total = 0;
    for (int t = 0; t < K; ++t) {
        if (type_counts[t] < 0) return fail(h, LWP_ERR_ARG, "negative type count");
        if (type_counts[t] > c.max_kpts) return fail(h, LWP_ERR_CAPACITY, "group_keypoints: more key-points of one type than max_kpts_per_type");
        total += type_counts[t];
    }
    if (total > 0 && !kpts) return fail(h, LWP_ERR_ARG, "kpts is null");
    std::vector<int> xy((size_t)K * c.max_kpts * 2, 0), cnt(K);
    std::vector<float> sc((size_t)K * c.max_kpts, 0.f);
    int r = 0;
    for (int t = 0; t < K; ++t) {
        cnt[t] = type_counts[t];
        for (int i = 0; i < type_counts[t]; ++i, ++r) {
            const double x = kpts[r * 4], y = kpts[r * 4 + 1];
            if (!(x >= 0 && x < W && y >= 0 && y < H)) return fail(h, LWP_ERR_ARG, "key-point outside the PAF map");
            if (kpts[r * 4 + 3] != (double)r) return fail(h, LWP_ERR_ARG, "key-point ids must be the running index 0..K-1");
            xy[((size_t)t * c.max_kpts + i) * 2] = (int)x;
            xy[((size_t)t * c.max_kpts + i) * 2 + 1] = (int)y;
            sc[(size_t)t * c.max_kpts + i] = (float)kpts[r * 4 + 2];
        }
    }
    const int NPc = h->g.NP;
    const float* d_paf = pafs;
    if (pafs_mem == LWP_MEM_HOST) {
        const size_t pb = (size_t)H * W * NPc * sizeof(float);
        HIP_TRY(h, h->d_tmp2.ensure(pb));
        HIP_TRY(h, hipMemcpyAsync(h->d_tmp2.as<float>(), pafs, pb, hipMemcpyHostToDevice, h->stream));
        d_paf = h->d_tmp2.as<float>();
    }
    h->run_has_tail = false;                           // entries only: lwp_get_poses has nothing to return after this call
    h->last_N = 1; h->async_pending = false;   // the workspace holds this one frame now (lwp_debug_post_counts reads it)
    LAUNCH(h, KC_POST, launch_reset_ws(1, h->ws, h->stream));
    HIP_TRY(h, hipMemcpyAsync(h->ws.kpt_xy, xy.data(), xy.size() * sizeof(int), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipMemcpyAsync(h->ws.kpt_score, sc.data(), sc.size() * sizeof(float), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipMemcpyAsync(h->ws.kpt_count, cnt.data(), K * sizeof(int), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));   // the host vectors above go out of scope
    MapView v{d_paf, 0, (int64_t)W * NPc, (int64_t)NPc, 1, H, W};
    LAUNCH(h, KC_POST, launch_score_pairs(v, 1, 1, demo, h->ws, h->stream));
    LAUNCH(h, KC_POST, launch_match(1, h->ws, h->stream));
    LAUNCH(h, KC_POST, launch_assemble(1, h->ws, h->stream));
    std::vector<int> kc(K);
    std::vector<double> kout((size_t)std::max(total, 1) * 4);
    return fetch_results(h, 1, kc.data(), kout.data(), std::max(total, 1), pose_entries, cap_entries, n_entries);
}

// ---------------------------------------------------------------------------------------------- pose tail
// device state of `lanes` lanes (grow-only; the lanes that exist keep their state)
static int ensure_tail_state(lwp_context* h, int lanes) {
    TailState& t = h->tst;
    const int P = h->caps.max_entries, K = h->skel.K;
    if (t.lanes >= lanes && t.P == P && t.K == K) return LWP_OK;
    if (P > kTailMaxPoses) return fail(h, LWP_ERR_ARG, "the pose tail (lwp_set_tracking) holds at most 256 poses per frame: lower max_pose_entries");
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (h->post_stream) HIP_TRY(h, hipStreamSynchronize(h->post_stream));
    const int keep = (t.P == P && t.K == K) ? t.lanes : 0;
    TailState n;
    n.lanes = std::max(lanes, keep); n.P = P; n.K = K; n.vars = h->d_vars.as<float>();
    const size_t L = (size_t)n.lanes, PK2 = (size_t)P * K * 2;
    struct Arr { void** dst; size_t per_lane; };
    Arr arrs[9] = {{(void**)&n.hdr, sizeof(int4)}, {(void**)&n.kp, 2 * PK2 * 4}, {(void**)&n.bbox, (size_t)2 * P * 16},
                   {(void**)&n.ids, (size_t)2 * P * 4}, {(void**)&n.f_xprev, 2 * PK2 * 4}, {(void**)&n.f_init, 2 * PK2 * 4},
                   {(void**)&n.f_dx, 2 * PK2 * 8}, {(void**)&n.f_x, 2 * PK2 * 8}, {(void**)&n.sim, (size_t)P * P}};
    DevBuf fresh[9];                                   // the old arrays stay until all nine new ones exist
    for (int i = 0; i < 9; ++i) {
        const size_t bytes = L * arrs[i].per_lane;
        HIP_TRY(h, fresh[i].ensure(bytes));
        *arrs[i].dst = fresh[i].as<void>();
        HIP_TRY(h, hipMemset(*arrs[i].dst, 0, bytes));
        if (keep && h->tst_mem[i]) HIP_TRY(h, hipMemcpy(*arrs[i].dst, h->tst_mem[i].as<void>(), (size_t)keep * arrs[i].per_lane, hipMemcpyDeviceToDevice));
    }
    for (int i = 0; i < 9; ++i) h->tst_mem[i] = std::move(fresh[i]);
    h->tst = n;
    HIP_TRY(h, launch_tail_reset(h->tst, keep, n.lanes - keep, h->tail_first_id, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return LWP_OK;
}

// the tail's launches for the N frames of `ws`, behind assemble_kernel on the same stream
// (unmap: the geometry of THIS run, passed to the launch by value — lwp_pipeline_submit_u8; null: the handle's lwp_set_unmap state)
static int enqueue_tail(lwp_context* h, PostWorkspace& ws, int N, int ratio, hipStream_t s, const TailParams* unmap = nullptr) {
    if (&ws == &h->ws) h->run_has_tail = ws.tail != 0; // (the serial path; a pipeline slot keeps its own tail_N)
    if (!ws.tail) return LWP_OK;
    TailParams p = unmap ? *unmap : h->tail;
    p.ratio = ratio;
    if (p.mode >= 2) { int rc = ensure_tail_state(h, p.mode == 2 ? N : 1); if (rc) return rc; }
    LAUNCH_ON(h, s, KC_POST, launch_tail_rows(N, ws, p, 0, s));
    if (p.mode >= 2) LAUNCH_ON(h, s, KC_POST, launch_tail_track(N, ws, h->tst, p, 0, s));
    return LWP_OK;
}

// the grouping kernels for N frames of stride-8 maps, on stream `s`; the tail follows once all frames of `ws` are grouped
static int enqueue_grouping(lwp_context* h, const MapView& heat, const MapView& paf, int N, int ratio, int demo, PostWorkspace& ws, hipStream_t s) {
    LAUNCH_ON(h, s, KC_POST, launch_find_peaks(heat, N, ws.K, ratio, ws, s, &h->tune));
    LAUNCH_ON(h, s, KC_POST, launch_nms(N, ws.K, heat.h * ratio, ws, s, true));
    LAUNCH_ON(h, s, KC_POST, launch_score_pairs(paf, N, ratio, demo, ws, s));
    LAUNCH_ON(h, s, KC_POST, launch_match(N, ws, s));
    LAUNCH_ON(h, s, KC_POST, launch_assemble(N, ws, s));
    return LWP_OK;
}

static int check_pose_args(lwp_context* h, int ratio, bool allow_ratio1, int64_t full_h, int64_t full_w) {
    if (ratio != 4 && ratio != 8 && !(allow_ratio1 && ratio == 1))
        return fail(h, LWP_ERR_ARG, allow_ratio1 ? "upsample ratio must be 1, 4 or 8" : "upsample ratio must be 4 or 8");
    if (!skeleton_fits(h)) return fail(h, LWP_ERR_ARG, "pose grouping needs >= 18 heat-maps and >= 38 PAFs (or a custom skeleton: lwp_set_skeleton)");
    if (full_h > 65535 || full_w > 65535) return fail(h, LWP_ERR_ARG, "map too large");   // peak coordinates are packed x << 16 | y
    return LWP_OK;
}
// the same for the network's maps of an H x W frame (H / 8 + 1 bounds the stride-8 height from above)
static int check_pose_frame(lwp_context* h, int H, int W, int ratio) {
    return check_pose_args(h, ratio, false, ((int64_t)H / 8 + 1) * ratio, ((int64_t)W / 8 + 1) * ratio);
}

// ---------------------------------------------------------------------------------------------- fused pipeline
static int enqueue_poses_chunk(lwp_context* h, const float* d_in, int N, int H, int W, int ratio, int demo, bool with_post, PostWorkspace ws) {
    const Graph& g = h->g;
    int fh, fw;
    level_dims(H, W, 3, &fh, &fw);
    const int cc = g.cat_channels;
    MapView heat, paf;
    // bf16 / fp16: the concat buffer is 16-bit, so the last stage's heads ALSO write f32 NCHW maps for the post-processing.  f32: the maps
    // could be read in place from the (NHWC) concat buffer, but the 4 x 4 footprint of a cubic sample is 4 cache lines in a
    // channel plane and 16 in channels-last rows: pair scoring at batch 32 runs 255 us on the concat buffer and ~80 on planes
    // (LWP_POST_NCHW=0: the in-place form, A/B)
    if (h->dtype != LWP_F32 || (with_post && h->tune.post_nchw != 0)) {
        const int nout = 2 * (1 + g.nref);
        std::vector<float*> outs(nout, nullptr);
        const size_t hb = (size_t)N * g.NH * fh * fw * sizeof(float), pb = (size_t)N * g.NP * fh * fw * sizeof(float);
        HIP_TRY(h, h->d_maps[0].ensure(hb));
        HIP_TRY(h, h->d_maps[1].ensure(pb));
        outs[nout - 2] = h->d_maps[0].as<float>();
        outs[nout - 1] = h->d_maps[1].as<float>();
        const int rc = enqueue_network(h, d_in, N, H, W, outs.data());
        if (rc || !with_post) return rc;
        heat = nchw_view(h->d_maps[0].as<float>(), g.NH, fh, fw);
        paf = nchw_view(h->d_maps[1].as<float>(), g.NP, fh, fw);
    } else {
        int rc = enqueue_network(h, d_in, N, H, W, nullptr);
        if (rc || !with_post) return rc;
        const float* cat = h->bufs[g.cat_buf].as<float>();
        heat = MapView{cat + g.C, (int64_t)fh * fw * cc, (int64_t)fw * cc, (int64_t)cc, 1, fh, fw};
        paf = MapView{cat + g.C + g.NH, (int64_t)fh * fw * cc, (int64_t)fw * cc, (int64_t)cc, 1, fh, fw};
    }
    return enqueue_grouping(h, heat, paf, N, ratio, demo, ws, h->stream);
}

// the whole batch, in as many equal launch sequences as keep every tensor below the 2 GiB addressing limit (one for any
// batch the BASELINE configs use); the results of all frames land in h->ws
static int enqueue_poses(lwp_context* h, const float* d_in, int N, int H, int W, int ratio, int demo, bool with_post) {
    int rc = for_each_pass(h, N, H, W, [&](int f0, int n) {
        return enqueue_poses_chunk(h, d_in + (size_t)f0 * 3 * H * W, n, H, W, ratio, demo, with_post, ws_frames(h->ws, f0));
    });
    if (rc) return rc;
    if (!with_post) { h->run_has_tail = false; return LWP_OK; }
    return enqueue_tail(h, h->ws, N, ratio, h->stream);
}

// the lanes' state belongs to one stream at a time: the serial path runs the tail on the main stream, a pipeline slot on the post stream
static int tail_serial_allowed(lwp_context* h) {
    if (h->tail.mode >= 2)
        for (auto& sl : h->slots) if (sl.pending) return fail(h, LWP_ERR_STATE, "tracking is on and a pipeline slot is pending: fetch it first");
    return LWP_OK;
}

static int prepare_poses(lwp_context* h, int N, int H, int W, int ratio) {
    int rc = check_frame_shape(h, N, H, W);
    if (rc) return rc;
    rc = tail_serial_allowed(h);
    if (rc) return rc;
    rc = check_pose_frame(h, H, W, ratio);
    if (rc) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    rc = ensure_activations(h, frames_per_pass(h, N, H, W), H, W);
    if (rc) return rc;
    return ensure_ws(h, N);
}

extern "C" int lwp_infer_poses_async(lwp_handle h, const float* in_device, int N, int H, int W, int ratio, int demo) {
    if (!h || !in_device) return fail(h, LWP_ERR_ARG, "null argument");
    int rc = prepare_poses(h, N, H, W, ratio);
    if (rc) return rc;
    rc = order_in(h);
    if (rc) return rc;
    h->last_N = N; h->async_pending = false;
    rc = enqueue_poses(h, in_device, N, H, W, ratio, demo, true);
    h->async_pending = rc == LWP_OK;
    return rc;
}

extern "C" int lwp_fetch_poses(lwp_handle h, int* kpt_counts, double* kpts, int kpt_cap, double* entries, int entry_cap, int* n_entries) {
    if (!h || !kpt_counts || !kpts || !entries || !n_entries) return fail(h, LWP_ERR_ARG, "null argument");
    if (h->last_N <= 0 || !h->ws.result_block || h->ws.N < h->last_N) return fail(h, LWP_ERR_STATE, "no pipeline run to fetch");
    HIP_TRY(h, hipSetDevice(h->device));
    h->async_pending = false;
    return fetch_results(h, h->last_N, kpt_counts, kpts, kpt_cap, entries, entry_cap, n_entries);
}

extern "C" int lwp_infer_poses(lwp_handle h, const float* in, int in_mem, int N, int H, int W, int ratio, int demo,
                               int* kpt_counts, double* kpts, int kpt_cap, double* entries, int entry_cap, int* n_entries) {
    if (!h || !in || !kpt_counts || !kpts || !entries || !n_entries) return fail(h, LWP_ERR_ARG, "null argument");
    int rc = prepare_poses(h, N, H, W, ratio);
    if (rc) return rc;
    if (in_mem == LWP_MEM_DEVICE) { rc = order_in(h); if (rc) return rc; }
    const float* d_in = nullptr;
    rc = stage_input(h, in, in_mem, (size_t)N * 3 * H * W * sizeof(float), &d_in);
    if (rc) return rc;
    h->last_N = N; h->async_pending = false;
    rc = enqueue_poses(h, d_in, N, H, W, ratio, demo, true);
    if (rc) return rc;
    return fetch_results(h, N, kpt_counts, kpts, kpt_cap, entries, entry_cap, n_entries);
}

// ---------------------------------------------------------------------------------------------- pipelined streaming
struct OverlayJob { const unsigned char* src; int H, W; };   // the uint8 frames a submit draws on (device memory the slot may read until it is fetched)
static int pipeline_submit_impl(lwp_context* h, const float* in_device, int N, int H, int W, int ratio, int demo, int slot, const TailParams* unmap,
                                const OverlayJob* overlay = nullptr);
extern "C" int lwp_pipeline_submit(lwp_handle h, const float* in_device, int N, int H, int W, int ratio, int demo, int slot) {
    return pipeline_submit_impl(h, in_device, N, H, W, ratio, demo, slot, nullptr);
}
// the settings of lwp_set_overlay as launch parameters (the pose arrays are filled in by the caller)
static OverlayParams overlay_params(const lwp_context* h, const unsigned char* src, unsigned char* out, int N, int H, int W) {
    OverlayParams p{};
    p.src = src; p.out = out; p.N = N; p.H = H; p.W = W;
    p.K = h->skel.K;
    p.limbs = h->d_limbs.as<int>();
    const int L = h->skel.L, nd = h->ovl.n_draw_limbs;
    p.n_limbs = nd < 0 ? std::max(L - 2, 0) : std::min(nd, L);      // -1: BODY_PARTS_KPT_IDS[:-2] (pose.py:51); a later, shorter skeleton clamps
    for (int c = 0; c < 3; ++c) { p.color[c] = h->ovl.color[c]; p.box_color[c] = h->ovl.box_color[c]; }
    p.boxes = h->ovl.boxes;
    return p;
}

// a slot's overlay buffers for `bytes` of frames.  Growing one waits for every stream that may still read the old one: the
// post stream (this slot's last overlay) and the main stream (an lwp_get_overlay copy, the last upload)
static int ensure_slot_overlay(lwp_context* h, lwp_context::Slot& sl, size_t bytes, bool host_frames) {
    const bool pinned = h->ovl.mode == 2;
    if (sl.ov.size() >= bytes && (!host_frames || sl.frames.size() >= bytes) && (!pinned || sl.h_ov.size() >= bytes)) return LWP_OK;
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (h->post_stream) HIP_TRY(h, hipStreamSynchronize(h->post_stream));
    sl.ov_N = 0;
    HIP_TRY(h, sl.ov.ensure(bytes));
    if (host_frames) HIP_TRY(h, sl.frames.ensure(bytes));
    if (pinned) HIP_TRY(h, sl.h_ov.ensure(bytes));
    return LWP_OK;
}

// the overlay of a slot's N frames behind its tail on stream `s`: the kernels read the frame's pose count, rows and boxes from
// the slot's result block, so nothing returns to the host in between; mode 2 adds the copy into the slot's pinned frames
static int enqueue_slot_overlay(lwp_context* h, lwp_context::Slot& sl, const OverlayJob& job, int N, hipStream_t s) {
    const PostWorkspace& w = sl.ws;
    const size_t bytes = (size_t)N * job.H * job.W * 3;
    if (!w.tail || !sl.ov || sl.ov.size() < bytes) return fail(h, LWP_ERR_STATE, "overlay without its buffers or the pose tail");
    OverlayParams p = overlay_params(h, job.src, sl.ov.as<unsigned char>(), N, job.H, job.W);
    const int P = w.caps.max_entries;
    p.n_poses = w.t_n; p.kp = w.t_kp; p.bbox = w.t_bbox;
    p.kp_stride = (int64_t)P * w.K * 2; p.bbox_stride = (int64_t)P * 4;
    p.P = P; p.K = w.K;
    LAUNCH_ON(h, s, KC_POST, launch_overlay(p, P, s));
    if (h->ovl.mode == 2) {
        void* mapped = nullptr;
        HIP_TRY(h, hipHostGetDevicePointer(&mapped, sl.h_ov.as<void>(), 0));
        HIP_TRY(h, launch_fetch_host(sl.ov.as<void>(), mapped, bytes, s));    // (the 16-byte copy kernel; here device -> pinned host)
    }
    sl.ov_N = N; sl.ov_H = job.H; sl.ov_W = job.W; sl.ov_mode = h->ovl.mode;
    return LWP_OK;
}

// unmap != null: the pose tail of this submit un-maps with these values instead of the handle's (lwp_pipeline_submit_u8);
// overlay != null: the overlay kernels follow the tail
static int pipeline_submit_impl(lwp_context* h, const float* in_device, int N, int H, int W, int ratio, int demo, int slot, const TailParams* unmap,
                                const OverlayJob* overlay) {
    if (!h || !in_device || slot < 0 || slot > 1) return fail(h, LWP_ERR_ARG, "bad argument");
    int rc = check_frame_shape(h, N, H, W);
    if (rc == LWP_OK) rc = check_pose_frame(h, H, W, ratio);
    if (rc) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    lwp_context::Slot& sl = h->slots[slot];
    if (sl.pending) return fail(h, LWP_ERR_STATE, "slot still pending: call lwp_pipeline_fetch first");
    sl.ov_N = 0;
    if (!h->post_stream) {
        if (h->tune.post_stream != 0) HIP_TRY(h, h->post_own.ensure());
        h->post_stream = h->tune.post_stream != 0 ? h->post_own : h->stream;
    }
    HIP_TRY(h, sl.ev_maps.ensure(hipEventDisableTiming));
    HIP_TRY(h, sl.ev_done.ensure(hipEventDisableTiming));
    rc = ensure_activations(h, frames_per_pass(h, N, H, W), H, W);
    if (rc) return rc;
    rc = order_in(h);
    if (rc) return rc;
    if (sl.ws.caps.max_peaks != h->caps.max_peaks || sl.ws.caps.max_kpts != h->caps.max_kpts) sl.ws.N = 0;   // (re)allocate lazily
    rc = ensure_ws_obj(h, sl.ws, sl.ws_mem, N, h->post_stream);
    if (rc) return rc;
    const Graph& g = h->g;
    int fh, fw;
    level_dims(H, W, 3, &fh, &fw);               // three stride-2 stages: out = (in - 1) / 2 + 1 each
    const size_t hb = (size_t)N * g.NH * fh * fw * sizeof(float), pb = (size_t)N * g.NP * fh * fw * sizeof(float);
    HIP_TRY(h, sl.maps[0].ensure(hb));
    HIP_TRY(h, sl.maps[1].ensure(pb));
    HIP_TRY(h, sl.h_stage.ensure(result_layout(sl.ws).bytes));
    // network on the main stream: the last stage's heads also write f32 NCHW maps into this slot
    const int nout = 2 * (1 + g.nref);
    std::vector<float*> outs(nout, nullptr);
    rc = for_each_pass(h, N, H, W, [&](int f0, int n) {   // one launch sequence unless a tensor would reach 2 GiB
        outs[nout - 2] = sl.maps[0].as<float>() + (size_t)f0 * g.NH * fh * fw;
        outs[nout - 1] = sl.maps[1].as<float>() + (size_t)f0 * g.NP * fh * fw;
        return enqueue_network(h, in_device + (size_t)f0 * 3 * H * W, n, H, W, outs.data());
    });
    if (rc) return rc;
    HIP_TRY(h, hipEventRecord(sl.ev_maps, h->stream));
    // post-processing + result copy on the second stream
    if (h->post_stream != h->stream) HIP_TRY(h, hipStreamWaitEvent(h->post_stream, sl.ev_maps, 0));
    rc = enqueue_grouping(h, nchw_view(sl.maps[0].as<float>(), g.NH, fh, fw), nchw_view(sl.maps[1].as<float>(), g.NP, fh, fw), N, ratio, demo, sl.ws, h->post_stream);
    if (rc == LWP_OK) rc = enqueue_tail(h, sl.ws, N, ratio, h->post_stream, unmap);
    if (rc == LWP_OK && overlay) rc = enqueue_slot_overlay(h, sl, *overlay, N, h->post_stream);
    if (rc) return rc;
    sl.tail_N = sl.ws.tail ? N : 0;
    HIP_TRY(h, launch_publish(N, sl.ws, sl.h_stage.as<void>(), h->post_stream));
    HIP_TRY(h, hipEventRecord(sl.ev_done, h->post_stream));
    sl.pending = true;
    sl.N = N;
    return LWP_OK;
}

extern "C" int lwp_pipeline_fetch(lwp_handle h, int slot, int* kpt_counts, double* kpts, int kpt_cap, double* entries, int entry_cap,
                                  int* n_entries) {
    if (!h || slot < 0 || slot > 1 || !kpt_counts || !kpts || !entries || !n_entries) return fail(h, LWP_ERR_ARG, "bad argument");
    lwp_context::Slot& sl = h->slots[slot];
    if (!sl.pending) return fail(h, LWP_ERR_STATE, "nothing submitted on this slot");
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipEventSynchronize(sl.ev_done));
    sl.pending = false;
    return parse_results(h, sl.ws, sl.h_stage.as<void>(), sl.N, kpt_counts, kpts, kpt_cap, entries, entry_cap, n_entries);
}

// ---------------------------------------------------------------------------------------------- batched uint8 front end
// the argument checks of the two batched uint8 entry points: host arithmetic only, so they run with h == NULL too
static int check_u8_batch_args(lwp_context* h, const void* imgs, int img_mem, int N, int H, int W, int net_input_height, int stride,
                               const double* pad_value, const double* img_mean, PreGeom* g) {
    if (!imgs) return fail(h, LWP_ERR_ARG, "imgs is null");
    if (!pad_value || !img_mean) return fail(h, LWP_ERR_ARG, "pad_value / img_mean is null");
    if (img_mem != LWP_MEM_HOST && img_mem != LWP_MEM_DEVICE) return fail(h, LWP_ERR_ARG, "img_mem must be LWP_MEM_HOST or LWP_MEM_DEVICE");
    if (N < 1) return fail(h, LWP_ERR_ARG, "N must be at least 1");
    if (N > 65535) return fail(h, LWP_ERR_ARG, "at most 65535 frames per call");
    int rc = lwp_preprocess_dims(H, W, net_input_height, stride, &g->dh, &g->dw, &g->Hp, &g->Wp, g->pad, &g->sc);
    if (rc) return fail(h, rc, "bad frame / network size");
    if (g->pad[0] < 0 || g->pad[1] < 0 || g->pad[2] < 0 || g->pad[3] < 0) return fail(h, LWP_ERR_ARG, "negative padding");
    if (g->Hp < 8 || g->Wp < 8) {
        char msg[160];
        snprintf(msg, sizeof msg, "frame too small: the padded network input is %d x %d, the network needs at least 8 x 8", g->Hp, g->Wp);
        return fail(h, LWP_ERR_ARG, msg);
    }
    return LWP_OK;
}

// upload (host frames) + the batched kernel on the main stream; *consumed as upload_host reports it.  own_dst: a device buffer
// of the caller's for the uploaded frames (a slot that draws on them later) instead of the shared staging
static int enqueue_u8_batch(lwp_context* h, const unsigned char* imgs, int img_mem, int N, int H, int W, const PreGeom& g,
                            const double* pad_value, const double* img_mean, double img_scale, float* out, bool* consumed,
                            unsigned char* own_dst = nullptr) {
    *consumed = true;
    const void* d_src = nullptr;
    int rc = stage_frames(h, imgs, img_mem, (size_t)N * H * W * 3, &d_src, consumed, own_dst);
    if (rc) return rc;
    const lwp_context::ResizeTab* tab = nullptr;
    rc = pre_tables(h, H, W, g, &tab);
    if (rc) return rc;
    LAUNCH(h, KC_POST, launch_preprocess_u8_batch(preproc_params(d_src, H, W, g, *tab, pad_value, img_mean, img_scale, out), N, h->tune.pre_batch_vec == 1, h->stream));
    return LWP_OK;
}

extern "C" int lwp_preprocess_u8_batch(lwp_handle h, const unsigned char* imgs, int img_mem, int N, int H, int W, int net_input_height,
                                       int stride, const double* pad_value, const double* img_mean, double img_scale, float* out_device) {
    PreGeom g;
    int rc = check_u8_batch_args(h, imgs, img_mem, N, H, W, net_input_height, stride, pad_value, img_mean, &g);
    if (rc) return rc;
    if (!out_device) return fail(h, LWP_ERR_ARG, "out_device is null");
    if (!h) return fail(h, LWP_ERR_ARG, "handle is null");
    HIP_TRY(h, hipSetDevice(h->device));
    rc = order_in(h);                                    // device frames produced / output buffer last used on the caller's stream
    if (rc) return rc;
    bool consumed = true;
    rc = enqueue_u8_batch(h, imgs, img_mem, N, H, W, g, pad_value, img_mean, img_scale, out_device, &consumed);
    if (rc) return rc;
    return finish_u8(h, img_mem, consumed);
}

extern "C" int lwp_pipeline_submit_u8(lwp_handle h, const unsigned char* imgs, int img_mem, int N, int H, int W, int net_input_height,
                                      int stride, const double* pad_value, const double* img_mean, double img_scale, int ratio,
                                      int demo, int slot) {
    PreGeom g;
    int rc = check_u8_batch_args(h, imgs, img_mem, N, H, W, net_input_height, stride, pad_value, img_mean, &g);
    if (rc) return rc;
    if (slot < 0 || slot > 1) return fail(h, LWP_ERR_ARG, "slot must be 0 or 1");
    if (ratio != 4 && ratio != 8) return fail(h, LWP_ERR_ARG, "upsample ratio must be 4 or 8");
    if (!h) return fail(h, LWP_ERR_ARG, "handle is null");
    rc = check_frame_shape(h, N, g.Hp, g.Wp);
    if (rc == LWP_OK) rc = check_pose_frame(h, g.Hp, g.Wp, ratio);
    if (rc) return rc;
    if (h->slots[slot].pending) return fail(h, LWP_ERR_STATE, "slot still pending: call lwp_pipeline_fetch first");
    if (h->tail.mode && h->caps.max_entries > kTailMaxPoses)
        return fail(h, LWP_ERR_ARG, "the pose tail (lwp_set_tracking) holds at most 256 poses per frame: lower max_pose_entries or turn it off");
    const bool overlay = h->ovl.mode != 0;
    if (overlay && !h->tail.mode)
        return fail(h, LWP_ERR_STATE, "the overlay (lwp_set_overlay) draws the pose tail's rows: lwp_set_tracking mode >= 1 first");
    HIP_TRY(h, hipSetDevice(h->device));
    rc = order_in(h);
    if (rc) return rc;
    const size_t xb = (size_t)N * 3 * g.Hp * g.Wp * sizeof(float);
    if (h->d_pipe_in.size() < xb) {                       // the network of the other slot may still read the old tensor
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        HIP_TRY(h, h->d_pipe_in.ensure(xb));
    }
    // with the overlay on, host frames are uploaded into a buffer of the SLOT: its overlay reads them on the post stream after
    // the next submit has overwritten the shared staging on the main stream
    lwp_context::Slot& sl = h->slots[slot];
    const bool own = overlay && img_mem == LWP_MEM_HOST;
    if (overlay) {
        rc = ensure_slot_overlay(h, sl, (size_t)N * H * W * 3, own);
        if (rc) return rc;
    }
    bool consumed = true;
    rc = enqueue_u8_batch(h, imgs, img_mem, N, H, W, g, pad_value, img_mean, img_scale, h->d_pipe_in.as<float>(), &consumed, own ? sl.frames.as<unsigned char>() : nullptr);
    if (rc) return rc;
    if (!consumed) HIP_TRY(h, hipEventSynchronize(h->ev_copy));    // (batches beyond the pinned staging limit: the copy is waited for)
    TailParams um = h->tail;                             // this submit's un-map, by value: the handle's lwp_set_unmap state is not touched
    um.stride = stride; um.scale = g.sc; um.pad_top = g.pad[0]; um.pad_left = g.pad[1];
    const OverlayJob job{own ? sl.frames.as<unsigned char>() : imgs, H, W};
    return pipeline_submit_impl(h, h->d_pipe_in.as<float>(), N, g.Hp, g.Wp, ratio, demo, slot, &um, overlay ? &job : nullptr);
}

extern "C" int lwp_poses_from_maps(lwp_handle h, const float* heat, const float* paf, int mem, int layout, int N, int hs, int ws, int ratio,
                                   int demo, int* kpt_counts, double* kpts, int kpt_cap, double* entries, int entry_cap,
                                   int* n_entries) {
    if (!h || !heat || !paf || !kpt_counts || !kpts || !entries || !n_entries || N <= 0 || hs <= 0 || ws <= 0)
        return fail(h, LWP_ERR_ARG, "bad argument");
    if (layout != LWP_LAYOUT_NCHW && layout != LWP_LAYOUT_NHWC) return fail(h, LWP_ERR_ARG, "layout must be LWP_LAYOUT_NCHW or LWP_LAYOUT_NHWC");
    int rc = check_pose_args(h, ratio, true, (int64_t)hs * ratio, (int64_t)ws * ratio);
    if (rc) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    rc = tail_serial_allowed(h);
    if (rc) return rc;
    rc = ensure_ws(h, N);
    if (rc) return rc;
    if (mem == LWP_MEM_DEVICE) { rc = order_in(h); if (rc) return rc; }
    const size_t hb = (size_t)N * h->g.NH * hs * ws * sizeof(float), pb = (size_t)N * h->g.NP * hs * ws * sizeof(float);
    const float *d_heat = heat, *d_paf = paf;
    if (mem == LWP_MEM_HOST) {
        HIP_TRY(h, h->d_tmp.ensure(hb));
        HIP_TRY(h, h->d_tmp2.ensure(pb));
        HIP_TRY(h, hipMemcpyAsync(h->d_tmp.as<float>(), heat, hb, hipMemcpyHostToDevice, h->stream));
        HIP_TRY(h, hipMemcpyAsync(h->d_tmp2.as<float>(), paf, pb, hipMemcpyHostToDevice, h->stream));
        d_heat = h->d_tmp.as<float>(); d_paf = h->d_tmp2.as<float>();
    }
    MapView hv = nchw_view(d_heat, h->g.NH, hs, ws), pv = nchw_view(d_paf, h->g.NP, hs, ws);
    if (layout == LWP_LAYOUT_NHWC) {                 // the averaged maps of val.infer are H x W x C
        hv.ys = (int64_t)ws * h->g.NH; hv.xs = h->g.NH; hv.cs = 1;
        pv.ys = (int64_t)ws * h->g.NP; pv.xs = h->g.NP; pv.cs = 1;
    }
    rc = enqueue_grouping(h, hv, pv, N, ratio, demo, h->ws, h->stream);
    if (rc == LWP_OK) rc = enqueue_tail(h, h->ws, N, ratio, h->stream);
    if (rc) return rc;
    h->last_N = N; h->async_pending = false;
    return fetch_results(h, N, kpt_counts, kpts, kpt_cap, entries, entry_cap, n_entries);
}

// ---------------------------------------------------------------------------------------------- pose tail: C ABI
static const float kCocoSigmas[18] = {.26f, .79f, .79f, .72f, .62f, .79f, .72f, .62f, 1.07f, .87f, .89f, 1.07f, .87f, .89f, .25f, .25f, .35f, .35f};

extern "C" int lwp_set_tracking(lwp_handle h, int mode, int match_threshold, double similarity_threshold, int smooth,
                                const float* sigmas, int n_sigmas) {
    const int K = h ? h->skel.K : 18;                  // the argument checks run without a handle too (against the default skeleton)
    char msg[200];
    if (mode < 0 || mode > 3) return fail(h, LWP_ERR_ARG, "tracking mode must be 0 (off), 1 (pose rows), 2 (lanes) or 3 (sequence)");
    if (mode >= 2) {
        if (!(similarity_threshold > 0.0 && similarity_threshold < 1.0))
            return fail(h, LWP_ERR_ARG, "similarity_threshold must lie inside (0, 1)");
        if (!sigmas) {
            if (n_sigmas != 0 && n_sigmas != 18) {
                snprintf(msg, sizeof msg, "sigmas is NULL (the COCO table of 18) but n_sigmas is %d", n_sigmas);
                return fail(h, LWP_ERR_ARG, msg);
            }
            if (K != 18) {
                snprintf(msg, sizeof msg, "sigmas is NULL (the COCO table of 18) but the skeleton has %d key-point types", K);
                return fail(h, LWP_ERR_ARG, msg);
            }
        } else if (n_sigmas != K) {
            snprintf(msg, sizeof msg, "n_sigmas is %d but the skeleton has %d key-point types", n_sigmas, K);
            return fail(h, LWP_ERR_ARG, msg);
        }
    }
    if (!h) return fail(h, LWP_ERR_ARG, "handle is null");
    for (auto& sl : h->slots) if (sl.pending) return fail(h, LWP_ERR_STATE, "pipeline slot pending");
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (h->post_stream) HIP_TRY(h, hipStreamSynchronize(h->post_stream));
    if (mode >= 2) {
        // Pose.vars (pose.py:15-17): sigmas float32 / 10.0, then (sigmas * 2) ** 2, every step rounded to float32
        float vars[kMaxSkelTypes] = {0};
        for (int k = 0; k < K; ++k) {
            volatile float sg = sigmas ? sigmas[k] : kCocoSigmas[k] / 10.0f;
            volatile float t = sg * 2.0f;
            vars[k] = t * t;
            if (!(vars[k] > 0.f)) return fail(h, LWP_ERR_ARG, "sigmas must be positive");
        }
        HIP_TRY(h, h->d_vars.ensure(kMaxSkelTypes * sizeof(float)));
        HIP_TRY(h, hipMemcpy(h->d_vars.as<float>(), vars, sizeof vars, hipMemcpyHostToDevice));
    }
    if ((mode != 0) != (h->tail.mode != 0)) free_workspaces(h);   // the result block gains or loses its tail section: re-allocated lazily
    free_tail_state(h);                                // every lane starts over
    h->last_N = 0; h->async_pending = false;
    h->tail_first_id = 0;
    h->tail.mode = mode;
    h->tail.match_threshold = match_threshold;
    h->tail.smooth = smooth ? 1 : 0;
    if (mode >= 2) h->tail.qmax = -std::log(similarity_threshold);
    return LWP_OK;
}

extern "C" int lwp_set_unmap(lwp_handle h, int stride, double scale, int pad_top, int pad_left) {
    if (stride <= 0) return fail(h, LWP_ERR_ARG, "stride must be positive");
    if (!(scale > 0.0) || !std::isfinite(scale)) return fail(h, LWP_ERR_ARG, "scale must be positive and finite");
    if (!h) return fail(h, LWP_ERR_ARG, "handle is null");
    h->tail.stride = stride; h->tail.scale = scale; h->tail.pad_top = pad_top; h->tail.pad_left = pad_left;
    return LWP_OK;
}

constexpr int kTailMaxLanes = 4096;

extern "C" int lwp_reset_tracking(lwp_handle h, int lane, int next_id) {
    if (lane < -1 || lane >= kTailMaxLanes) return fail(h, LWP_ERR_ARG, "lane must be -1 (all) or 0..4095");
    if (next_id < 0) return fail(h, LWP_ERR_ARG, "next_id must not be negative");
    if (!h) return fail(h, LWP_ERR_ARG, "handle is null");
    if (h->tail.mode < 2) return fail(h, LWP_ERR_STATE, "tracking is off (lwp_set_tracking mode 2 or 3)");
    for (auto& sl : h->slots) if (sl.pending) return fail(h, LWP_ERR_STATE, "pipeline slot pending");
    HIP_TRY(h, hipSetDevice(h->device));
    if (lane < 0) h->tail_first_id = next_id;
    int rc = ensure_tail_state(h, lane < 0 ? std::max(h->tst.lanes, 1) : lane + 1);
    if (rc) return rc;
    if (h->post_stream) HIP_TRY(h, hipStreamSynchronize(h->post_stream));
    HIP_TRY(h, launch_tail_reset(h->tst, lane < 0 ? 0 : lane, lane < 0 ? h->tst.lanes : 1, next_id, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return LWP_OK;
}

// host view of the tail section of a published result block
struct TailHost { const int *n, *last, *ids, *bbox, *kp; const unsigned* near_; const double* conf; };
static TailHost tail_host(const PostWorkspace& ws, const void* host_block) {
    const ResultLayout l = result_layout(ws);
    auto hp = [&](const ResultLayout::Sec& s) { return (const void*)((const char*)host_block + s.off); };
    return TailHost{(const int*)hp(l.t_n), (const int*)hp(l.t_last), (const int*)hp(l.t_ids), (const int*)hp(l.t_bbox),
                    (const int*)hp(l.t_kp), (const unsigned*)hp(l.t_near), (const double*)hp(l.t_conf)};
}
static int tail_source(lwp_context* h, int slot, const PostWorkspace** ws, const void** block, int* N) {
    if (slot < -1 || slot > 1) return fail(h, LWP_ERR_ARG, "slot must be -1 (the last serial call), 0 or 1");
    if (slot < 0) { *ws = &h->ws; *block = h->h_stage.as<void>(); *N = h->stage_tail_N; }
    else {
        if (h->slots[slot].pending) return fail(h, LWP_ERR_STATE, "slot still pending: call lwp_pipeline_fetch first");
        *ws = &h->slots[slot].ws; *block = h->slots[slot].h_stage.as<void>(); *N = h->slots[slot].tail_N;
    }
    if (*N <= 0 || !(*ws)->tail || !*block) return fail(h, LWP_ERR_STATE, "no pose rows: the pose tail was off for that run (lwp_set_tracking), or nothing was fetched");
    return LWP_OK;
}

extern "C" int lwp_get_poses(lwp_handle h, int slot, int* n_poses, int* keypoints, double* confidence, int* bbox, int* ids,
                             int* last_ids, int pose_cap) {
    if (!h || !n_poses || !keypoints || !confidence || !bbox || !ids || pose_cap < 0) return fail(h, LWP_ERR_ARG, "bad argument");
    const PostWorkspace* ws; const void* block; int N;
    int rc = tail_source(h, slot, &ws, &block, &N);
    if (rc) return rc;
    const TailHost t = tail_host(*ws, block);
    const size_t P = (size_t)ws->caps.max_entries, K = (size_t)ws->K;
    for (int f = 0; f < N; ++f) {
        if (t.n[f] < 0 || (size_t)t.n[f] > P) return fail(h, LWP_ERR_STATE, "the staged result block holds no valid pose rows");
        if (t.n[f] > pose_cap) return fail(h, LWP_ERR_CAPACITY, "pose arrays too small (pose_cap)");
    }
    for (int f = 0; f < N; ++f) {
        const size_t n = (size_t)t.n[f];
        n_poses[f] = t.n[f];
        std::memcpy(keypoints + (size_t)f * pose_cap * K * 2, t.kp + f * P * K * 2, n * K * 2 * sizeof(int));
        std::memcpy(confidence + (size_t)f * pose_cap, t.conf + f * P, n * sizeof(double));
        std::memcpy(bbox + (size_t)f * pose_cap * 4, t.bbox + f * P * 4, n * 4 * sizeof(int));
        std::memcpy(ids + (size_t)f * pose_cap, t.ids + f * P, n * sizeof(int));
        if (last_ids) last_ids[f] = t.last[f];
    }
    return LWP_OK;
}

extern "C" int lwp_debug_tracking_near(lwp_handle h, int slot, unsigned* counts, int cap) {
    if (!h || !counts) return fail(h, LWP_ERR_ARG, "bad argument");
    const PostWorkspace* ws; const void* block; int N;
    int rc = tail_source(h, slot, &ws, &block, &N);
    if (rc) return rc;
    if (cap < N) return fail(h, LWP_ERR_CAPACITY, "counts array too small");
    const TailHost t = tail_host(*ws, block);
    for (int f = 0; f < N; ++f) counts[f] = t.near_[f];
    return LWP_OK;
}

extern "C" int lwp_track_poses(lwp_handle h, int lane, int n, const int* keypoints, const double* confidence, int* out_keypoints,
                               int* out_bbox, int* out_ids, int* last_id, unsigned* near_count) {
    if (lane < 0 || lane >= kTailMaxLanes) return fail(h, LWP_ERR_ARG, "lane must be 0..4095");
    if (n < 0) return fail(h, LWP_ERR_ARG, "negative pose count");
    if (n > 0 && (!keypoints || !confidence || !out_keypoints || !out_bbox || !out_ids)) return fail(h, LWP_ERR_ARG, "null argument");
    for (int i = 0; i < n; ++i)
        if (!std::isfinite(confidence[i])) return fail(h, LWP_ERR_ARG, "confidences must be finite (sorting poses by a NaN has no defined order)");
    if (!h) return fail(h, LWP_ERR_ARG, "handle is null");
    if (h->tail.mode < 2) return fail(h, LWP_ERR_STATE, "tracking is off (lwp_set_tracking mode 2 or 3)");
    for (auto& sl : h->slots) if (sl.pending) return fail(h, LWP_ERR_STATE, "pipeline slot pending");
    if (n > h->caps.max_entries) return fail(h, LWP_ERR_CAPACITY, "more poses than max_pose_entries");
    HIP_TRY(h, hipSetDevice(h->device));
    int rc = ensure_ws(h, 1);
    if (rc) return rc;
    rc = ensure_tail_state(h, lane + 1);
    if (rc) return rc;
    rc = ensure_host_stage(h, result_layout(h->ws).bytes + 64);
    if (rc) return rc;
    h->stage_tail_N = 0;                               // frame 0 of the workspace is reused: the rows of the last run are gone,
    h->run_has_tail = false;                           // and so is an lwp_infer_poses_async run that was not fetched yet
    h->last_N = 0; h->async_pending = false;
    if (h->post_stream) HIP_TRY(h, hipStreamSynchronize(h->post_stream));
    const size_t K = (size_t)h->ws.K;
    if (n > 0) {
        HIP_TRY(h, hipMemcpyAsync(h->ws.t_kp, keypoints, (size_t)n * K * 2 * sizeof(int), hipMemcpyHostToDevice, h->stream));
        HIP_TRY(h, hipMemcpyAsync(h->ws.t_conf, confidence, (size_t)n * sizeof(double), hipMemcpyHostToDevice, h->stream));
    }
    HIP_TRY(h, hipMemcpyAsync(h->ws.t_n, &n, sizeof(int), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    TailParams p = h->tail;
    p.mode = 3;                                        // one frame of one lane
    HIP_TRY(h, launch_tail_rows(1, h->ws, p, 1, h->stream));
    HIP_TRY(h, launch_tail_track(1, h->ws, h->tst, p, lane, h->stream));
    HIP_TRY(h, launch_publish(1, h->ws, h->h_stage.as<void>(), h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    const TailHost t = tail_host(h->ws, h->h_stage.as<void>());
    if (n > 0) {
        std::memcpy(out_keypoints, t.kp, (size_t)n * K * 2 * sizeof(int));
        std::memcpy(out_bbox, t.bbox, (size_t)n * 4 * sizeof(int));
        std::memcpy(out_ids, t.ids, (size_t)n * sizeof(int));
    }
    if (last_id) *last_id = t.last[0];
    if (near_count) *near_count = t.near_[0];
    return LWP_OK;
}

// ---------------------------------------------------------------------------------------------- pose overlay: C ABI
extern "C" int lwp_set_overlay(lwp_handle h, int mode, const unsigned char* color, const unsigned char* box_color, int boxes,
                               int n_draw_limbs) {
    const int L = h ? h->skel.L : 19;                  // the argument checks run without a handle too (against the default skeleton)
    char msg[160];
    if (mode < 0 || mode > 2) return fail(h, LWP_ERR_ARG, "overlay mode must be 0 (off), 1 (frames on the device) or 2 (also copied to pinned host memory)");
    if (n_draw_limbs < -1 || n_draw_limbs > L) {
        snprintf(msg, sizeof msg, "n_draw_limbs must be -1 (all but the last two) or 0..%d (the skeleton's limbs), got %d", L, n_draw_limbs);
        return fail(h, LWP_ERR_ARG, msg);
    }
    if (!h) return fail(h, LWP_ERR_ARG, "handle is null");
    for (auto& sl : h->slots) if (sl.pending) return fail(h, LWP_ERR_STATE, "pipeline slot pending");
    static const unsigned char kColor[3] = {0, 224, 255}, kBoxColor[3] = {0, 255, 0};      // Pose.color (pose.py:21), demo.py:124
    for (int c = 0; c < 3; ++c) { h->ovl.color[c] = (color ? color : kColor)[c]; h->ovl.box_color[c] = (box_color ? box_color : kBoxColor)[c]; }
    h->ovl.mode = mode;
    h->ovl.boxes = boxes ? 1 : 0;
    h->ovl.n_draw_limbs = n_draw_limbs;
    return LWP_OK;
}

extern "C" int lwp_get_overlay(lwp_handle h, int slot, unsigned char* dst, int dst_mem, int N, int H, int W) {
    if (!dst) return fail(h, LWP_ERR_ARG, "dst is null");
    if (dst_mem != LWP_MEM_HOST && dst_mem != LWP_MEM_DEVICE) return fail(h, LWP_ERR_ARG, "dst_mem must be LWP_MEM_HOST or LWP_MEM_DEVICE");
    if (slot < 0 || slot > 1) return fail(h, LWP_ERR_ARG, "slot must be 0 or 1");
    if (!h) return fail(h, LWP_ERR_ARG, "handle is null");
    lwp_context::Slot& sl = h->slots[slot];
    if (sl.pending) return fail(h, LWP_ERR_STATE, "slot still pending: call lwp_pipeline_fetch first");
    if (sl.ov_N <= 0) return fail(h, LWP_ERR_STATE, "no annotated frames: the slot ran without the overlay (lwp_set_overlay), or nothing was fetched");
    if (N != sl.ov_N || H != sl.ov_H || W != sl.ov_W) {
        char msg[160];
        snprintf(msg, sizeof msg, "the slot holds %d annotated frames of %d x %d, asked for %d of %d x %d", sl.ov_N, sl.ov_H, sl.ov_W, N, H, W);
        return fail(h, LWP_ERR_ARG, msg);
    }
    const size_t bytes = (size_t)N * H * W * 3;
    HIP_TRY(h, hipSetDevice(h->device));
    if (dst_mem == LWP_MEM_HOST) {                     // the fetch has waited for the slot's stream: both copies are complete
        if (sl.ov_mode == 2) std::memcpy(dst, sl.h_ov.as<void>(), bytes);
        else HIP_TRY(h, hipMemcpy(dst, sl.ov.as<void>(), bytes, hipMemcpyDeviceToHost));
        return LWP_OK;
    }
    int rc = order_in(h);                              // dst last used on the caller's stream
    if (rc) return rc;
    HIP_TRY(h, hipMemcpyAsync(dst, sl.ov.as<void>(), bytes, hipMemcpyDeviceToDevice, h->stream));
    bool ordered = false;
    rc = order_out(h, h->stream, &ordered);
    if (rc) return rc;
    if (!ordered) HIP_TRY(h, hipStreamSynchronize(h->stream));
    return LWP_OK;
}

extern "C" int lwp_draw_poses(lwp_handle h, const unsigned char* imgs, int img_mem, int N, int H, int W, const int* n_poses,
                              const int* keypoints, const int* bbox, int pose_cap, unsigned char* out, int out_mem) {
    char msg[160];
    if (!imgs || !out) return fail(h, LWP_ERR_ARG, "imgs / out is null");
    if (imgs == out) return fail(h, LWP_ERR_ARG, "out must not be imgs: the blend reads the source pixels");
    if ((img_mem != LWP_MEM_HOST && img_mem != LWP_MEM_DEVICE) || (out_mem != LWP_MEM_HOST && out_mem != LWP_MEM_DEVICE))
        return fail(h, LWP_ERR_ARG, "img_mem / out_mem must be LWP_MEM_HOST or LWP_MEM_DEVICE");
    if (N < 1) return fail(h, LWP_ERR_ARG, "N must be at least 1");
    if (N > 65535) return fail(h, LWP_ERR_ARG, "at most 65535 frames per call");
    if (H < 1 || W < 1) return fail(h, LWP_ERR_ARG, "empty frame");
    if (!n_poses) return fail(h, LWP_ERR_ARG, "n_poses is null");
    if (pose_cap < 0 || pose_cap > 65535) return fail(h, LWP_ERR_ARG, "pose_cap must be 0..65535");
    int most = 0;
    for (int f = 0; f < N; ++f) {
        if (n_poses[f] < 0 || n_poses[f] > pose_cap) {
            snprintf(msg, sizeof msg, "frame %d has %d poses but pose_cap is %d", f, n_poses[f], pose_cap);
            return fail(h, LWP_ERR_ARG, msg);
        }
        most = std::max(most, n_poses[f]);
    }
    if (most > 0 && (!keypoints || !bbox)) return fail(h, LWP_ERR_ARG, "keypoints / bbox is null");
    if (!h) return fail(h, LWP_ERR_ARG, "handle is null");
    HIP_TRY(h, hipSetDevice(h->device));
    int rc = LWP_OK;
    if (img_mem == LWP_MEM_DEVICE || out_mem == LWP_MEM_DEVICE) { rc = order_in(h); if (rc) return rc; }
    const size_t K = (size_t)h->skel.K, ib = (size_t)N * H * W * 3;
    // the pose arrays in one device buffer: [n_poses | key-points | boxes], each section 16-byte aligned
    const size_t nb = ((size_t)N * 4 + 15) & ~(size_t)15, kb = ((size_t)N * pose_cap * K * 2 * 4 + 15) & ~(size_t)15, bb = (size_t)N * pose_cap * 4 * 4;
    if (h->d_ov_pose.size() < nb + kb + bb + 16 || (out_mem == LWP_MEM_HOST && h->d_ov_out.size() < ib)) {
        HIP_TRY(h, hipStreamSynchronize(h->stream));   // an earlier launch may still read the old buffers
        HIP_TRY(h, h->d_ov_pose.ensure(nb + kb + bb + 16));
        if (out_mem == LWP_MEM_HOST) HIP_TRY(h, h->d_ov_out.ensure(ib));
    }
    char* dp = h->d_ov_pose.as<char>();
    HIP_TRY(h, hipMemcpyAsync(dp, n_poses, (size_t)N * 4, hipMemcpyHostToDevice, h->stream));
    if (most > 0) {
        HIP_TRY(h, hipMemcpyAsync(dp + nb, keypoints, (size_t)N * pose_cap * K * 2 * 4, hipMemcpyHostToDevice, h->stream));
        HIP_TRY(h, hipMemcpyAsync(dp + nb + kb, bbox, (size_t)N * pose_cap * 4 * 4, hipMemcpyHostToDevice, h->stream));
    }
    HIP_TRY(h, hipStreamSynchronize(h->stream));       // the caller's pose arrays are free from here on
    const void* d_src = nullptr;
    bool consumed = true;
    rc = stage_frames(h, imgs, img_mem, ib, &d_src, &consumed);
    if (rc) return rc;
    if (!consumed) HIP_TRY(h, hipEventSynchronize(h->ev_copy));
    unsigned char* d_out = out_mem == LWP_MEM_HOST ? h->d_ov_out.as<unsigned char>() : out;
    OverlayParams p = overlay_params(h, (const unsigned char*)d_src, d_out, N, H, W);
    p.n_poses = (const int*)dp; p.kp = (const int*)(dp + nb); p.bbox = (const int*)(dp + nb + kb);
    p.kp_stride = (int64_t)pose_cap * (int64_t)K * 2; p.bbox_stride = (int64_t)pose_cap * 4;
    p.P = pose_cap;
    LAUNCH(h, KC_POST, launch_overlay(p, most, h->stream));
    if (out_mem == LWP_MEM_HOST) {
        HIP_TRY(h, hipMemcpyAsync(out, d_out, ib, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        return LWP_OK;
    }
    bool ordered = false;
    rc = order_out(h, h->stream, &ordered);
    if (rc) return rc;
    if (!ordered) HIP_TRY(h, hipStreamSynchronize(h->stream));
    return LWP_OK;
}

// ---------------------------------------------------------------------------------------------- training targets and loss
// argument checks, upload of the counts (and of host key-points) and the kernel's parameters: everything of lwp_train_targets
// before its launch, shared with lwp_time_train_targets
static int train_targets_prepare(lwp_handle h, const double* kpts, int kpts_mem, const int* n_persons, int N, int Pmax, int H, int W,
                                 int stride, double sigma, double paf_thickness, float* keypoint_maps_device, float* paf_maps_device,
                                 TrainTargetsParams* out) {
    char msg[200];
    if (!keypoint_maps_device || !paf_maps_device) return fail(h, LWP_ERR_ARG, "keypoint_maps_device / paf_maps_device is null");
    if (kpts_mem != LWP_MEM_HOST && kpts_mem != LWP_MEM_DEVICE) return fail(h, LWP_ERR_ARG, "kpts_mem must be LWP_MEM_HOST or LWP_MEM_DEVICE");
    if (N < 1 || N > 65535) return fail(h, LWP_ERR_ARG, "N must be 1..65535");
    if (Pmax < 0 || Pmax > 65535) return fail(h, LWP_ERR_ARG, "Pmax must be 0..65535");
    if (stride < 1 || stride > 1024) return fail(h, LWP_ERR_ARG, "stride must be 1..1024");
    if (H < stride || W < stride || H > (1 << 20) || W > (1 << 20)) return fail(h, LWP_ERR_ARG, "the frame must hold at least one stride x stride cell (and at most 2^20 pixels a side)");
    if ((int64_t)(H / stride) * (W / stride) > (1 << 28)) return fail(h, LWP_ERR_ARG, "oversized map: more than 2^28 cells");
    if (!(sigma > 0) || !std::isfinite(sigma)) return fail(h, LWP_ERR_ARG, "sigma must be positive and finite");
    if (!(paf_thickness >= 0) || !std::isfinite(paf_thickness)) return fail(h, LWP_ERR_ARG, "paf_thickness must be finite and not negative");
    if (!n_persons) return fail(h, LWP_ERR_ARG, "n_persons is null");
    int most = 0;
    for (int f = 0; f < N; ++f) {
        if (n_persons[f] < 0 || n_persons[f] > Pmax) {
            snprintf(msg, sizeof msg, "frame %d has %d persons but Pmax is %d", f, n_persons[f], Pmax);
            return fail(h, LWP_ERR_ARG, msg);
        }
        most = std::max(most, n_persons[f]);
    }
    if (most > 0 && !kpts) return fail(h, LWP_ERR_ARG, "kpts is null");
    if (!h) return fail(h, LWP_ERR_ARG, "handle is null");
    const Skeleton& sk = h->skel;
    const int K = sk.K, L = sk.L;
    // the kernel walks the limbs inside each chunk of persons, the reference all persons of a limb before the next limb: the
    // two orders agree only while no target channel belongs to two limbs
    std::vector<char> used((size_t)2 * L, 0);
    for (int l = 0; l < L; ++l)
        for (int c = 0; c < 2; ++c) {
            const int ch = sk.paf[2 * l + c];
            if (ch < 0 || ch >= 2 * L) {
                snprintf(msg, sizeof msg, "limb %d: PAF channels (%d, %d) lie outside the %d target channels (2 x num_limbs)", l, sk.paf[2 * l], sk.paf[2 * l + 1], 2 * L);
                return fail(h, LWP_ERR_ARG, msg);
            }
            if (used[ch]) {
                snprintf(msg, sizeof msg, "limb %d: PAF channel %d is already written by another limb", l, ch);
                return fail(h, LWP_ERR_ARG, msg);
            }
            used[ch] = 1;
        }
    const size_t kd = (size_t)N * Pmax * K * 3;
    if (kpts_mem == LWP_MEM_HOST)                      // int() of a NaN or an infinity raises in the reference
        for (int f = 0; f < N; ++f)
            for (size_t i = 0; i < (size_t)n_persons[f] * K * 3; ++i)
                if (!std::isfinite(kpts[(size_t)f * Pmax * K * 3 + i])) {
                    snprintf(msg, sizeof msg, "frame %d: a key-point value is not finite", f);
                    return fail(h, LWP_ERR_ARG, msg);
                }
    HIP_TRY(h, hipSetDevice(h->device));
    int rc = order_in(h);
    if (rc) return rc;
    // [n_persons | key-points]: the counts always travel, the key-points only from host memory
    const size_t nb = ((size_t)N * 4 + 15) & ~(size_t)15, kb = kpts_mem == LWP_MEM_HOST ? kd * sizeof(double) : 0;
    if (h->d_train.size() < nb + kb + 16) {
        HIP_TRY(h, hipStreamSynchronize(h->stream));   // an earlier launch may still read the old buffer
        HIP_TRY(h, h->d_train.ensure(nb + kb + 16));
    }
    char* dp = h->d_train.as<char>();
    HIP_TRY(h, hipMemcpyAsync(dp, n_persons, (size_t)N * 4, hipMemcpyHostToDevice, h->stream));
    if (kb && most > 0) HIP_TRY(h, hipMemcpyAsync(dp + nb, kpts, kb, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));       // the caller's arrays are free from here on
    TrainTargetsParams p{};
    p.kpts = kpts_mem == LWP_MEM_HOST ? (const double*)(dp + nb) : kpts;
    p.n_persons = (const int*)dp;
    p.Pmax = most > 0 ? Pmax : 0; p.K = K; p.L = L;
    p.limbs = h->d_limbs.as<int>();
    p.h = H / stride; p.w = W / stride; p.stride = stride;
    p.sigma = sigma; p.thickness = paf_thickness;
    p.keypoint_maps = keypoint_maps_device; p.paf_maps = paf_maps_device;
    *out = p;
    return LWP_OK;
}

extern "C" int lwp_train_targets(lwp_handle h, const double* kpts, int kpts_mem, const int* n_persons, int N, int Pmax, int H, int W,
                                 int stride, double sigma, double paf_thickness, float* keypoint_maps_device, float* paf_maps_device) {
    TrainTargetsParams p{};
    int rc = train_targets_prepare(h, kpts, kpts_mem, n_persons, N, Pmax, H, W, stride, sigma, paf_thickness, keypoint_maps_device,
                                   paf_maps_device, &p);
    if (rc) return rc;
    LAUNCH(h, KC_OTHER, launch_train_targets(p, N, h->stream));
    bool ordered = false;
    rc = order_out(h, h->stream, &ordered);
    if (rc) return rc;
    if (!ordered) HIP_TRY(h, hipStreamSynchronize(h->stream));
    return LWP_OK;
}

extern "C" int lwp_mask_downsample(lwp_handle h, const float* mask, int mem, int N, int H, int W, int stride, float* out_device) {
    if (!mask || !out_device) return fail(h, LWP_ERR_ARG, "mask / out_device is null");
    if (mem != LWP_MEM_HOST && mem != LWP_MEM_DEVICE) return fail(h, LWP_ERR_ARG, "mem must be LWP_MEM_HOST or LWP_MEM_DEVICE");
    if (N < 1 || N > 65535) return fail(h, LWP_ERR_ARG, "N must be 1..65535");
    if (stride < 1 || stride > 1024) return fail(h, LWP_ERR_ARG, "stride must be 1..1024");
    if (H < stride || W < stride || H > (1 << 20) || W > (1 << 20)) return fail(h, LWP_ERR_ARG, "the mask must hold at least one stride x stride block (and at most 2^20 pixels a side)");
    if ((int64_t)(H / stride) * (W / stride) > (1 << 28)) return fail(h, LWP_ERR_ARG, "oversized map: more than 2^28 cells");
    if (H % stride || W % stride) {
        char msg[160];
        snprintf(msg, sizeof msg, "a %d x %d mask is not a whole number of %d x %d blocks: only exact block means are supported", H, W, stride, stride);
        return fail(h, LWP_ERR_ARG, msg);
    }
    if (!h) return fail(h, LWP_ERR_ARG, "handle is null");
    HIP_TRY(h, hipSetDevice(h->device));
    int rc = order_in(h);
    if (rc) return rc;
    const float* d_src = mask;
    if (mem == LWP_MEM_HOST) {
        const size_t mb = (size_t)N * H * W * sizeof(float);
        if (h->d_train.size() < mb) {
            HIP_TRY(h, hipStreamSynchronize(h->stream));
            HIP_TRY(h, h->d_train.ensure(mb));
        }
        HIP_TRY(h, hipMemcpyAsync(h->d_train.as<float>(), mask, mb, hipMemcpyHostToDevice, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        d_src = h->d_train.as<float>();
    }
    LAUNCH(h, KC_OTHER, launch_mask_downsample(d_src, N, H, W, stride, out_device, h->stream));
    bool ordered = false;
    rc = order_out(h, h->stream, &ordered);
    if (rc) return rc;
    if (!ordered) HIP_TRY(h, hipStreamSynchronize(h->stream));
    return LWP_OK;
}

// ---------------------------------------------------------------------------------------------- crowd masks
// the RLEs of a batch as the entry points take them: image n owns segmentations image_seg_off[n] .. image_seg_off[n + 1] - 1,
// segmentation s the counts seg_off[s] .. seg_off[s + 1] - 1
struct CrowdRuns { const int64_t *counts, *seg_off, *image_seg_off; };
// what crowd_check leaves for crowd_pack: the sizes, and the layout of [run ends | segment offsets | image records]
struct CrowdTables {
    int64_t S = 0, runs = 0;
    int n_rec = 0, max_h = 0, max_w = 0;
    size_t segs_at = 0, recs_at = 0, bytes = 0;
};

// every check that needs no GPU.  size_of(n, &h, &w): the image's size; rendered(n): whether image n gets a record
template <class SizeOf, class Rendered>
static int crowd_check(lwp_context* h, const CrowdRuns& r, int N, SizeOf size_of, Rendered rendered, CrowdTables* t) {
    char msg[200];
    if (!r.seg_off || !r.image_seg_off) return fail(h, LWP_ERR_ARG, "seg_off / image_seg_off is null");
    if (N < 1 || N > 65535) return fail(h, LWP_ERR_ARG, "N must be 1..65535");
    auto bad = [&](int f, const char* what) {
        snprintf(msg, sizeof msg, "sample %d: %s", f, what);
        return fail(h, LWP_ERR_ARG, msg);
    };
    if (r.image_seg_off[0] != 0) return fail(h, LWP_ERR_ARG, "image_seg_off must start at 0");
    for (int f = 0; f < N; ++f)
        if (r.image_seg_off[f + 1] < r.image_seg_off[f]) return bad(f, "image_seg_off descends");
    const int64_t S = r.image_seg_off[N];
    if (S >= ((int64_t)1 << 31)) return fail(h, LWP_ERR_ARG, "2^31 segmentations or more");
    if (r.seg_off[0] != 0) return fail(h, LWP_ERR_ARG, "seg_off must start at 0");
    for (int f = 0; f < N; ++f)
        for (int64_t s = r.image_seg_off[f]; s < r.image_seg_off[f + 1]; ++s)
            if (r.seg_off[s + 1] < r.seg_off[s]) return bad(f, "seg_off descends");
    const int64_t runs = r.seg_off[S];
    if (runs >= ((int64_t)1 << 31)) return fail(h, LWP_ERR_ARG, "2^31 counts or more");
    if (runs > 0 && !r.counts) return fail(h, LWP_ERR_ARG, "counts is null");
    *t = CrowdTables();
    for (int f = 0; f < N; ++f) {
        int ih = 0, iw = 0;
        size_of(f, &ih, &iw);
        if (ih < 1 || iw < 1 || ih >= 32768 || iw >= 32768) return bad(f, "the image size is outside 1..32767");
        const int64_t hw = (int64_t)ih * iw;
        for (int64_t s = r.image_seg_off[f]; s < r.image_seg_off[f + 1]; ++s) {
            int64_t sum = 0;
            for (int64_t i = r.seg_off[s]; i < r.seg_off[s + 1]; ++i) {
                const int64_t c = r.counts[i];
                if (c < 0) return bad(f, "a segmentation holds a negative count");
                if (c > hw - sum) return bad(f, "the counts of a segmentation sum to more than height * width");
                sum += c;
            }
        }
        if (!rendered(f)) continue;
        t->n_rec += 1;
        t->max_h = std::max(t->max_h, ih);
        t->max_w = std::max(t->max_w, iw);
    }
    t->S = S; t->runs = runs;
    t->segs_at = ((size_t)runs * sizeof(unsigned) + 15) & ~(size_t)15;
    t->recs_at = t->segs_at + ((((size_t)S + 1) * sizeof(unsigned) + 15) & ~(size_t)15);
    t->bytes = t->recs_at + (((size_t)t->n_rec * sizeof(CrowdImage) + 15) & ~(size_t)15);
    return LWP_OK;
}

// the tables at `host`, which will live at `dev`: the counts become run ends (h * w < 2^30, so a running sum fits 32 bits);
// out_of(n): the float offset of image n's mask in `masks`
template <class SizeOf, class Rendered, class OutOf>
static CrowdLaunch crowd_pack(const CrowdTables& t, const CrowdRuns& r, int N, SizeOf size_of, Rendered rendered, OutOf out_of,
                              unsigned char* host, unsigned char* dev, float* masks) {
    unsigned* ends = reinterpret_cast<unsigned*>(host);
    unsigned* segs = reinterpret_cast<unsigned*>(host + t.segs_at);
    CrowdImage* recs = reinterpret_cast<CrowdImage*>(host + t.recs_at);
    for (int64_t s = 0; s < t.S; ++s) {
        unsigned e = 0;
        for (int64_t i = r.seg_off[s]; i < r.seg_off[s + 1]; ++i) ends[i] = (e += (unsigned)r.counts[i]);
    }
    for (int64_t s = 0; s <= t.S; ++s) segs[s] = (unsigned)r.seg_off[s];
    int k = 0;
    for (int f = 0; f < N; ++f) {
        if (!rendered(f)) continue;
        CrowdImage& im = recs[k++];
        size_of(f, &im.h, &im.w);
        im.seg0 = (unsigned)r.image_seg_off[f];
        im.n_seg = (unsigned)(r.image_seg_off[f + 1] - r.image_seg_off[f]);
        im.out = (long long)out_of(f);
    }
    CrowdLaunch c;
    c.ends = reinterpret_cast<const unsigned*>(dev);
    c.seg_off = reinterpret_cast<const unsigned*>(dev + t.segs_at);
    c.images = reinterpret_cast<const CrowdImage*>(dev + t.recs_at);
    c.masks = masks;
    c.n_images = t.n_rec; c.max_h = t.max_h; c.max_w = t.max_w;
    return c;
}

// argument checks and the one upload of lwp_crowd_masks and its timing twin; the tables share the augmentation's staging
static int crowd_masks_prepare(lwp_handle h, const CrowdRuns& r, const int* heights, const int* widths, int N, const int64_t* out_off,
                               float* masks_device, CrowdLaunch* launch) {
    char msg[200];
    if (!heights || !widths || !out_off || !masks_device) return fail(h, LWP_ERR_ARG, "heights / widths / out_off / masks_device is null");
    auto size_of = [&](int f, int* ih, int* iw) { *ih = heights[f]; *iw = widths[f]; };
    auto every = [](int) { return true; };            // an image without segmentations is all ones
    CrowdTables t;
    int rc = crowd_check(h, r, N, size_of, every, &t);
    if (rc) return rc;
    if (out_off[0] != 0) return fail(h, LWP_ERR_ARG, "out_off must start at 0");
    for (int f = 0; f < N; ++f)
        if (out_off[f + 1] - out_off[f] < (int64_t)heights[f] * widths[f]) {
            snprintf(msg, sizeof msg, "sample %d: out_off leaves fewer than height * width floats", f);
            return fail(h, LWP_ERR_ARG, msg);
        }
    if (!h) return fail(h, LWP_ERR_ARG, "handle is null");
    HIP_TRY(h, hipSetDevice(h->device));
    rc = order_in(h);
    if (rc) return rc;
    if (h->d_augment.size() < t.bytes) {
        HIP_TRY(h, hipStreamSynchronize(h->stream));   // an earlier launch may still read the old buffer
        HIP_TRY(h, h->d_augment.ensure(t.bytes));
    }
    h->augment_stage.resize(t.bytes);
    unsigned char* dev = h->d_augment.as<unsigned char>();
    *launch = crowd_pack(t, r, N, size_of, every, [&](int f) { return out_off[f]; }, h->augment_stage.data(), dev, masks_device);
    HIP_TRY(h, hipMemcpyAsync(dev, h->augment_stage.data(), t.bytes, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));       // the staging vector and the caller's arrays are free from here on
    return LWP_OK;
}

extern "C" int lwp_crowd_masks(lwp_handle h, const int64_t* counts, const int64_t* seg_off, const int64_t* image_seg_off,
                               const int* heights, const int* widths, int N, const int64_t* out_off, float* masks_device) {
    CrowdLaunch c{};
    int rc = crowd_masks_prepare(h, CrowdRuns{counts, seg_off, image_seg_off}, heights, widths, N, out_off, masks_device, &c);
    if (rc) return rc;
    LAUNCH(h, KC_OTHER, launch_crowd_masks(c, h->stream));
    bool ordered = false;
    rc = order_out(h, h->stream, &ordered);
    if (rc) return rc;
    if (!ordered) HIP_TRY(h, hipStreamSynchronize(h->stream));
    return LWP_OK;
}

// ---------------------------------------------------------------------------------------------- JPEG decode
extern "C" int lwp_jpeg_info(const unsigned char* data, size_t len, lwp_jpeg_header* out) {
    if (!data || !out) return fail(nullptr, LWP_ERR_ARG, "data / out is null");
    char msg[256] = {0};
    if (jpeg_parse_header(data, len, out, msg, sizeof msg) != JPEG_OK) return fail(nullptr, LWP_ERR_ARG, msg);
    return LWP_OK;
}

extern "C" int lwp_debug_jpeg_blocks(const unsigned char* data, size_t len, int16_t* coef, size_t coef_cap, uint16_t* qtables) {
    if (!data || !coef || !qtables) return fail(nullptr, LWP_ERR_ARG, "data / coef / qtables is null");
    char msg[256] = {0};
    lwp_jpeg_header hd;
    const int rc = jpeg_decode_blocks(data, len, &hd, coef, coef_cap, qtables, msg, sizeof msg);
    if (rc == JPEG_CAPACITY) return fail(nullptr, LWP_ERR_CAPACITY, msg);
    if (rc != JPEG_OK) return fail(nullptr, LWP_ERR_ARG, msg);
    return LWP_OK;
}

// ---- device entropy mode (lwp_set_jpeg_entropy; jpeg_entropy_kernels.hip)
static bool jpeg_subseq_ok(int v) { return v >= 4 && v <= 1024 && v % 4 == 0; }

extern "C" int lwp_set_jpeg_entropy(lwp_handle h, int mode, int subseq_bytes) {
    if (!h) return fail(h, LWP_ERR_ARG, "handle is null");
    if (mode != LWP_JPEG_ENTROPY_HOST && mode != LWP_JPEG_ENTROPY_DEVICE) return fail(h, LWP_ERR_ARG, "mode must be LWP_JPEG_ENTROPY_HOST or LWP_JPEG_ENTROPY_DEVICE");
    if (subseq_bytes != 0 && !jpeg_subseq_ok(subseq_bytes)) return fail(h, LWP_ERR_ARG, "subseq_bytes must be 0 (the default) or a multiple of 4 from 4 to 1024");
    h->jpeg_entropy_mode = mode;
    h->jpeg_subseq = subseq_bytes ? subseq_bytes : kJpegSubseqDefault;
    return LWP_OK;
}

extern "C" int lwp_debug_jpeg_scan(const unsigned char* data, size_t len, unsigned char* bytes_out, size_t bytes_cap, size_t* n_bytes,
                                   uint32_t* segs_out, size_t segs_cap, size_t* n_segs, unsigned char* tables_out, uint16_t* qtables_out,
                                   int* status_out) {
    if (!data || !bytes_out || !n_bytes || !segs_out || !n_segs || !status_out) return fail(nullptr, LWP_ERR_ARG, "data / bytes_out / n_bytes / segs_out / n_segs / status_out is null");
    char msg[256] = {0};
    lwp_jpeg_header hd;
    if (jpeg_parse_header(data, len, &hd, msg, sizeof msg) != JPEG_OK) return fail(nullptr, LWP_ERR_ARG, msg);
    if (jpeg_expected_segments(hd) > segs_cap) return fail(nullptr, LWP_ERR_CAPACITY, "jpeg: segs_cap is below the segments the header promises");
    std::vector<JpegHuffFlat> tables(kJpegHuffPerFile);
    uint16_t qt[kJpegQuantSlots * 64];
    static_assert(sizeof(JpegScanSeg) == 4 * sizeof(uint32_t), "segs_out is four uint32 a segment");
    *status_out = jpeg_scan_segments(data, len, &hd, bytes_out, bytes_cap, n_bytes, reinterpret_cast<JpegScanSeg*>(segs_out), segs_cap, n_segs,
                                     tables.data(), qt);
    if (tables_out) memcpy(tables_out, tables.data(), kJpegHuffPerFile * sizeof(JpegHuffFlat));
    if (qtables_out) memcpy(qtables_out, qt, sizeof qt);
    return LWP_OK;
}

// ---- batches.  The checks of the files, the layout of the workspace and the records are jpeg_batch.cpp's; here is what needs
// the handle.  A refusal of jpeg_batch.cpp as the call's error:
static int jpeg_fail(lwp_handle h, int rc, const char* msg) { return fail(h, rc == JPEG_CAPACITY ? LWP_ERR_CAPACITY : LWP_ERR_ARG, msg); }

// files shared among up to kJpegHostThreads threads (file i goes to thread i mod T; the result does not depend on T): the
// files are independent of each other, each works into its own part of the staging
template <class F>
static void jpeg_share_files(int N, size_t in_bytes, F per_file) {
    int T = std::min({kJpegHostThreads, N, (int)std::max(1u, std::thread::hardware_concurrency())});
    if (in_bytes < kJpegThreadedFromBytes) T = 1;
    std::vector<std::thread> pool;
    int started = 1;                                   // this thread is the first
    try {
        for (; started < T; ++started) pool.emplace_back([&, t = started]() { for (int i = t; i < N; i += T) per_file(i); });
    } catch (const std::system_error&) {}              // no more threads to be had: this one takes the rest below
    for (int i = 0; i < N; i += T) per_file(i);
    for (std::thread& th : pool) th.join();
    for (int t = started; t < T; ++t)
        for (int i = t; i < N; i += T) per_file(i);
}

// begins a staged batch: `bytes` of pinned staging, which the copy of the call before may still read
static int jpeg_stage_begin(lwp_handle h, lwp_context::JpegMem& m, size_t bytes, unsigned char** host) {
    HIP_TRY(h, hipSetDevice(h->device));
    if (m.copy_pending) {
        HIP_TRY(h, hipEventSynchronize(m.ev));
        m.copy_pending = false;
    }
    HIP_TRY(h, m.stage.ensure(bytes));
    *host = m.stage.as<unsigned char>();
    return LWP_OK;
}

// sends it: a workspace of `total` bytes at *dev, the staging's first `upload` bytes into its front on the handle's stream and,
// with `event`, the event behind the copy (a call that ends synchronised needs none).  finish(*dev) runs in front of the copy:
// the records that hold device addresses
template <class F>
static int jpeg_stage_send(lwp_handle h, lwp_context::JpegMem& m, size_t upload, size_t total, bool event, unsigned char** dev, F finish) {
    int rc = order_in(h);
    if (rc) return rc;
    if (m.dev.size() < total) {
        HIP_TRY(h, hipStreamSynchronize(h->stream));   // an earlier launch may still read the old buffer
        HIP_TRY(h, m.dev.ensure(total));
    }
    *dev = m.dev.as<unsigned char>();
    finish(*dev);
    if (event) HIP_TRY(h, m.ev.ensure(hipEventDisableTiming));
    HIP_TRY(h, hipMemcpyAsync(*dev, m.stage.as<unsigned char>(), upload, hipMemcpyHostToDevice, h->stream));
    if (event) {
        HIP_TRY(h, hipEventRecord(m.ev, h->stream));
        m.copy_pending = true;
    }
    return LWP_OK;
}

static JpegLaunch jpeg_launch(unsigned char* dev, const JpegHeaders& H, const JpegDecodePlan& P) {
    JpegLaunch j{};
    j.coef = reinterpret_cast<const int16_t*>(dev + P.coef); j.qtables = reinterpret_cast<const uint16_t*>(dev + P.qt);
    j.planes = reinterpret_cast<const JpegPlane*>(dev + P.planes); j.plane_block0 = reinterpret_cast<const unsigned*>(dev + P.pstart);
    j.images = reinterpret_cast<const JpegImage*>(dev + P.images); j.image_unit0 = reinterpret_cast<const unsigned*>(dev + P.istart);
    j.workspace = dev;
    j.n_planes = H.n_planes; j.n_images = (int)H.hd.size();
    j.total_blocks = (unsigned)H.blocks; j.total_units = (unsigned)H.units;
    return j;
}

static JpegEntropyLaunch jpeg_entropy_launch(unsigned char* dev, const JpegHeaders& H, const JpegEntropyPlan& P, int subseq) {
    JpegEntropyLaunch e{};
    e.words = reinterpret_cast<const unsigned*>(dev + P.bytes); e.n_words = (unsigned)((P.tab - P.bytes) / 4);
    e.tables = reinterpret_cast<const JpegHuffFlat*>(dev + P.tab);
    e.files = reinterpret_cast<const JpegEntFile*>(dev + P.files); e.file_wg0 = reinterpret_cast<const unsigned*>(dev + P.fwg);
    e.segs = reinterpret_cast<const JpegEntSeg*>(dev + P.segs); e.seg_sub0 = reinterpret_cast<const unsigned*>(dev + P.ssub);
    e.rec = reinterpret_cast<uint2*>(dev + P.rec); e.subpos = reinterpret_cast<unsigned*>(dev + P.subpos);
    e.wg_entry = reinterpret_cast<uint2*>(dev + P.wg_entry); e.wg_dirty = reinterpret_cast<unsigned*>(dev + P.wg_dirty);
    e.coef = reinterpret_cast<int16_t*>(dev + P.d.coef); e.status = reinterpret_cast<int*>(dev + P.status);
    e.n_files = (int)H.hd.size(); e.n_segs = P.n_segs; e.n_subs = P.n_subs; e.n_wgs = P.n_wgs;
    e.subseq_bytes = subseq;
    return e;
}

// the host decoder's verdict on one file, decoded only for that: its message words every refusal, whichever mode met it
static int jpeg_host_verdict(const unsigned char* data, size_t len, const lwp_jpeg_header& hd, char* why, size_t why_cap) {
    std::vector<int16_t> coef((size_t)hd.total_blocks * 64);
    uint16_t qt[kJpegQuantSlots * 64];
    lwp_jpeg_header now;
    why[0] = 0;
    return jpeg_decode_blocks(data, len, &now, coef.data(), coef.size(), qt, why, why_cap);
}

// host entropy mode: checks, the host half of every file and the batch's one upload.  Nothing is enqueued before every file
// has been decoded: a refusal leaves the outputs untouched.
static int jpeg_prepare(lwp_handle h, int N, const unsigned char* const* data, const size_t* len, unsigned char* const* out, JpegLaunch* launch) {
    char msg[kJpegMsg];
    if (!data || !len || !out) return fail(h, LWP_ERR_ARG, "data / len / out is null");
    if (N < 1 || N > 65535) return fail(h, LWP_ERR_ARG, "N must be 1..65535");
    JpegHeaders H;
    int rc = jpeg_batch_headers(N, data, len, out, false, &H, msg);
    if (rc) return jpeg_fail(h, rc, msg);
    if (!h) return fail(h, LWP_ERR_ARG, "handle is null");
    JpegDecodePlan P;
    jpeg_decode_plan(H, &P);
    unsigned char *host = nullptr, *dev = nullptr;
    rc = jpeg_stage_begin(h, h->jpeg, P.upload, &host);
    if (rc) return rc;
    // the entropy decode of the files.  The first refused file in index order is the one reported.
    std::vector<uint64_t> first_block((size_t)N + 1, 0);
    for (int i = 0; i < N; ++i) first_block[i + 1] = first_block[i] + (uint64_t)H.hd[i].total_blocks;
    std::vector<std::string> bad((size_t)N);
    jpeg_share_files(N, H.in_bytes, [&](int i) {
        lwp_jpeg_header now;
        char w[256] = {0};
        const int r = jpeg_decode_blocks(data[i], len[i], &now, reinterpret_cast<int16_t*>(host + P.coef) + first_block[i] * 64,
                                         (size_t)H.hd[i].total_blocks * 64, reinterpret_cast<uint16_t*>(host + P.qt) + (size_t)i * kJpegQuantSlots * 64,
                                         w, sizeof w);
        if (r != JPEG_OK || now.total_blocks != H.hd[i].total_blocks) { H.verdict[i] = JPEG_REFUSED; bad[i] = r != JPEG_OK ? w : "the file changed during the call"; }
    });
    for (int i = 0; i < N; ++i)
        if (H.verdict[i]) {
            snprintf(msg, sizeof msg, "image %d: %s", i, bad[i].c_str());
            return fail(h, LWP_ERR_ARG, msg);
        }
    jpeg_decode_fill(H, P, out, host);
    rc = jpeg_stage_send(h, h->jpeg, P.upload, P.total, true, &dev, [](unsigned char*) {});
    if (rc) return rc;
    *launch = jpeg_launch(dev, H, P);
    return LWP_OK;
}

// the call's error for file i, which the pre-pass (by_kernels false) or the kernels refused: the host decoder's message, so
// both modes word a refusal alike; a file the host accepts is an internal error, never a silent repair
static int jpeg_device_refusal(lwp_handle h, int i, const unsigned char* data, size_t len, const lwp_jpeg_header& hd, int verdict, bool by_kernels) {
    char msg[kJpegMsg], why[256];
    if (verdict == JPEG_CAPACITY) {
        snprintf(msg, sizeof msg, "image %d: jpeg: the scan's un-stuffed length is 2^28 bytes or more, which the device entropy mode does not take: decode it in host mode", i);
        return fail(h, LWP_ERR_CAPACITY, msg);
    }
    if (jpeg_host_verdict(data, len, hd, why, sizeof why) != JPEG_OK) {
        snprintf(msg, sizeof msg, "image %d: %s", i, why);
        return fail(h, LWP_ERR_ARG, msg);
    }
    snprintf(msg, sizeof msg, "image %d: the device entropy decoder's %s refused a file that the host decoder accepts", i, by_kernels ? "kernels" : "pre-pass");
    return fail(h, LWP_ERR_INTERNAL, msg);
}

struct JpegDeviceBatch {
    JpegHeaders H;                                     // verdict: per file JPEG_OK, or why it takes no part (tolerant calls only)
    JpegLaunch j{};
    JpegEntropyLaunch e{};
    const uint16_t* qt_host = nullptr;                 // the quantisation tables in the staging
    int* status_host = nullptr;                        // [N + 2] in the staging, filled by jpeg_device_entropy
    size_t memset_bytes = 0;                           // coefficients and status words, from e.coef on
};

// Device mode's front half: headers, the pre-pass on the host threads, the one upload.  `tolerant`
// (lwp_debug_jpeg_entropy_batch): a refused file takes no part instead of failing the call.
static int jpeg_device_prepare(lwp_handle h, int N, const unsigned char* const* data, const size_t* len, unsigned char* const* out,
                               int subseq, bool tolerant, JpegDeviceBatch* B) {
    char msg[kJpegMsg], why[256];
    if (!data || !len) return fail(h, LWP_ERR_ARG, "data / len is null");        // out: null where the call writes no pixels
    if (N < 1 || N > 65535) return fail(h, LWP_ERR_ARG, "N must be 1..65535");
    JpegHeaders& H = B->H;
    JpegEntropyPlan P;
    int rc = jpeg_batch_headers(N, data, len, out, tolerant, &H, msg);
    if (!rc) rc = jpeg_entropy_plan(H, len, &P, msg);
    if (rc) return jpeg_fail(h, rc, msg);
    if (!h) return fail(h, LWP_ERR_ARG, "handle is null");
    unsigned char *host = nullptr, *dev = nullptr;
    rc = jpeg_stage_begin(h, h->jpeg, P.stage_bytes, &host);
    if (rc) return rc;
    JpegHuffFlat* tables = reinterpret_cast<JpegHuffFlat*>(host + P.tab);
    uint16_t* qt = reinterpret_cast<uint16_t*>(host + P.d.qt);
    std::vector<JpegScanSeg> scan((size_t)P.seg_at[N] + 1);
    std::vector<size_t> n_scan((size_t)N, 0);
    jpeg_share_files(N, H.in_bytes, [&](int i) {
        if (H.verdict[i]) {
            memset(tables + (size_t)i * kJpegHuffPerFile, 0, kJpegHuffPerFile * sizeof(JpegHuffFlat));
            memset(qt + (size_t)i * kJpegQuantSlots * 64, 0, kJpegQuantSlots * 128);
            return;
        }
        size_t nb = 0;
        H.verdict[i] = jpeg_scan_segments(data[i], len[i], &H.hd[i], host + P.bytes + P.byte_at[i], (size_t)(P.byte_at[i + 1] - P.byte_at[i]), &nb,
                                          scan.data() + P.seg_at[i], (size_t)(P.seg_at[i + 1] - P.seg_at[i]), &n_scan[i],
                                          tables + (size_t)i * kJpegHuffPerFile, qt + (size_t)i * kJpegQuantSlots * 64);
    });
    memset(host + P.bytes + P.byte_at[N], 0, P.tab - P.byte_at[N]);
    if (!tolerant)
        for (int i = 0; i < N; ++i)
            if (H.verdict[i]) {
                // the call names the LOWEST refused file, and a file in front of this one may be one the kernels would refuse:
                // nothing has been enqueued yet, so the host decoder gives their verdicts (this path is a failing call's only)
                for (int j = 0; j < i; ++j)
                    if (jpeg_host_verdict(data[j], len[j], H.hd[j], why, sizeof why) != JPEG_OK) {
                        snprintf(msg, sizeof msg, "image %d: %s", j, why);
                        return fail(h, LWP_ERR_ARG, msg);
                    }
                return jpeg_device_refusal(h, i, data[i], len[i], H.hd[i], H.verdict[i], false);
            }
    rc = jpeg_entropy_fill(H, &P, scan.data(), n_scan.data(), subseq, host, msg);
    if (rc) return jpeg_fail(h, rc, msg);
    jpeg_entropy_place(H, &P);
    jpeg_decode_fill(H, P.d, out, host);
    rc = jpeg_stage_send(h, h->jpeg, P.d.upload, P.d.total, true, &dev, [](unsigned char*) {});
    if (rc) return rc;
    B->j = jpeg_launch(dev, H, P.d);
    B->e = jpeg_entropy_launch(dev, H, P, subseq);
    B->qt_host = qt;
    B->status_host = reinterpret_cast<int*>(host + P.d.upload);
    B->memset_bytes = P.status + ((size_t)N + 2) * 4 - P.d.coef;
    return LWP_OK;
}

// the memset and the four entropy kernels
static int jpeg_entropy_enqueue(lwp_handle h, const JpegDeviceBatch& B) {
    HIP_TRY(h, hipMemsetAsync(B.e.coef, 0, B.memset_bytes, h->stream));
    LAUNCH(h, KC_OTHER, launch_jpeg_entropy(B.e, h->stream));
    return LWP_OK;
}

// ... then the status words back to the host, and the wait for them
static int jpeg_device_entropy(lwp_handle h, JpegDeviceBatch& B) {
    int rc = jpeg_entropy_enqueue(h, B);
    if (rc) return rc;
    HIP_TRY(h, hipMemcpyAsync(B.status_host, B.e.status, ((size_t)B.e.n_files + 2) * 4, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return LWP_OK;
}

// device mode up to the coefficients: fails the call for the lowest refused file before stage A is enqueued
static int jpeg_prepare_device(lwp_handle h, int N, const unsigned char* const* data, const size_t* len, unsigned char* const* out, JpegLaunch* launch) {
    if (!data || !len || !out) return fail(h, LWP_ERR_ARG, "data / len / out is null");
    JpegDeviceBatch B;
    int rc = jpeg_device_prepare(h, N, data, len, out, h->jpeg_subseq, false, &B);
    if (rc) return rc;
    rc = jpeg_device_entropy(h, B);
    if (rc) return rc;
    for (int i = 0; i < N; ++i)
        if (B.status_host[i]) return jpeg_device_refusal(h, i, data[i], len[i], B.H.hd[i], JPEG_REFUSED, true);
    *launch = B.j;
    return LWP_OK;
}

extern "C" int lwp_debug_jpeg_entropy_batch(lwp_handle h, int N, const unsigned char* const* data, const size_t* len, int subseq_bytes,
                                            int16_t* const* coef_out, uint16_t* const* qtables_out, int* status_out) {
    if (!coef_out || !qtables_out || !status_out) return fail(h, LWP_ERR_ARG, "coef_out / qtables_out / status_out is null");
    if (subseq_bytes != 0 && !jpeg_subseq_ok(subseq_bytes)) return fail(h, LWP_ERR_ARG, "subseq_bytes must be 0 (the default) or a multiple of 4 from 4 to 1024");
    if (!h) return fail(h, LWP_ERR_ARG, "handle is null");
    JpegDeviceBatch B;
    int rc = jpeg_device_prepare(h, N, data, len, nullptr, subseq_bytes ? subseq_bytes : h->jpeg_subseq, true, &B);
    if (rc) return rc;
    rc = jpeg_device_entropy(h, B);
    if (rc) return rc;
    size_t b0 = 0;
    for (int i = 0; i < N; ++i) {
        const size_t n = (size_t)B.H.hd[i].total_blocks;
        status_out[i] = B.H.verdict[i] ? B.H.verdict[i] : B.status_host[i] ? JPEG_REFUSED : JPEG_OK;
        if (!status_out[i]) {
            if (!coef_out[i] || !qtables_out[i]) return fail(h, LWP_ERR_ARG, "coef_out[i] / qtables_out[i] is null");
            HIP_TRY(h, hipMemcpyAsync(coef_out[i], B.j.coef + b0 * 64, n * 128, hipMemcpyDeviceToHost, h->stream));
            memcpy(qtables_out[i], B.qt_host + (size_t)i * kJpegQuantSlots * 64, kJpegQuantSlots * 128);
        }
        b0 += n;
    }
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return LWP_OK;
}

extern "C" int lwp_time_jpeg_entropy_batch(lwp_handle h, int N, const unsigned char* const* data, const size_t* len, int subseq_bytes,
                                           int iters, float* ms_total, int* rounds) {
    if (iters < 1 || !ms_total || !rounds) return fail(h, LWP_ERR_ARG, "iters must be at least 1 and ms_total / rounds non-null");
    if (subseq_bytes != 0 && !jpeg_subseq_ok(subseq_bytes)) return fail(h, LWP_ERR_ARG, "subseq_bytes must be 0 (the default) or a multiple of 4 from 4 to 1024");
    if (!h) return fail(h, LWP_ERR_ARG, "handle is null");
    JpegDeviceBatch B;
    int rc = jpeg_device_prepare(h, N, data, len, nullptr, subseq_bytes ? subseq_bytes : h->jpeg_subseq, false, &B);
    if (rc) return rc;
    rc = time_on_stream(h, iters, [&]() { return jpeg_entropy_enqueue(h, B); }, ms_total);
    if (rc) return rc;
    HIP_TRY(h, hipMemcpyAsync(B.status_host, B.e.status, ((size_t)N + 2) * 4, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    for (int i = 0; i < N; ++i)
        if (B.status_host[i]) return jpeg_device_refusal(h, i, data[i], len[i], B.H.hd[i], JPEG_REFUSED, true);
    rounds[0] = B.status_host[N]; rounds[1] = B.status_host[N + 1];
    return LWP_OK;
}

extern "C" int lwp_jpeg_decode_batch(lwp_handle h, int N, const unsigned char* const* data, const size_t* len, unsigned char* const* out) {
    JpegLaunch j{};
    int rc = h && h->jpeg_entropy_mode == LWP_JPEG_ENTROPY_DEVICE ? jpeg_prepare_device(h, N, data, len, out, &j) : jpeg_prepare(h, N, data, len, out, &j);
    if (rc) return rc;
    LAUNCH(h, KC_OTHER, launch_jpeg_idct(j, h->stream));
    LAUNCH(h, KC_OTHER, launch_jpeg_color(j, h->stream));
    bool ordered = false;
    rc = order_out(h, h->stream, &ordered);
    if (rc) return rc;
    if (!ordered) HIP_TRY(h, hipStreamSynchronize(h->stream));
    return LWP_OK;
}

extern "C" int lwp_time_jpeg_decode_batch(lwp_handle h, int N, const unsigned char* const* data, const size_t* len,
                                          unsigned char* const* out, int iters, float* ms_total) {
    if (iters < 1 || !ms_total) return fail(h, LWP_ERR_ARG, "iters must be at least 1 and ms_total non-null");
    JpegLaunch j{};
    int rc = h && h->jpeg_entropy_mode == LWP_JPEG_ENTROPY_DEVICE ? jpeg_prepare_device(h, N, data, len, out, &j) : jpeg_prepare(h, N, data, len, out, &j);
    if (rc) return rc;
    rc = time_on_stream(h, iters, [&]() { LAUNCH(h, KC_OTHER, launch_jpeg_idct(j, h->stream)); return (int)LWP_OK; }, &ms_total[0]);
    if (rc) return rc;
    return time_on_stream(h, iters, [&]() { LAUNCH(h, KC_OTHER, launch_jpeg_color(j, h->stream)); return (int)LWP_OK; }, &ms_total[1]);
}

// ---------------------------------------------------------------------------------------------- JPEG encode
extern "C" int lwp_jpeg_encode_bound(int height, int width, int subsampling, int restart_interval, size_t* bound_out) {
    JpegEncGeom g;
    if (!bound_out) return fail(nullptr, LWP_ERR_ARG, "bound_out is null");
    if (!jpeg_enc_geometry(height, width, subsampling, restart_interval, &g))
        return fail(nullptr, LWP_ERR_ARG, "jpeg encode: height and width must be 1..65535, subsampling 0..2, restart_interval 0..65535");
    *bound_out = kJpegEncHeaderMax + jpeg_enc_scan_bound(g) + 2;
    return LWP_OK;
}

extern "C" int lwp_debug_jpeg_encode_header(int height, int width, int quality, int subsampling, int restart_interval, unsigned char* out,
                                            size_t cap, size_t* n_out) {
    JpegEncGeom g;
    if (!out || !n_out) return fail(nullptr, LWP_ERR_ARG, "out / n_out is null");
    if (quality < 1 || quality > 100) return fail(nullptr, LWP_ERR_ARG, "jpeg encode: quality must be 1..100");
    if (!jpeg_enc_geometry(height, width, subsampling, restart_interval, &g))
        return fail(nullptr, LWP_ERR_ARG, "jpeg encode: height and width must be 1..65535, subsampling 0..2, restart_interval 0..65535");
    unsigned char hd[kJpegEncHeaderMax];
    const size_t n = jpeg_enc_header(height, width, quality, subsampling, restart_interval, hd);
    if (n > cap) return fail(nullptr, LWP_ERR_CAPACITY, "jpeg encode: the header does not fit cap (640 bytes always suffice)");
    memcpy(out, hd, n);
    *n_out = n;
    return LWP_OK;
}

struct JpegEncBatch {
    JpegEncPlan P;
    JpegEncLaunch e{};
};

static JpegEncLaunch jpeg_enc_launch(unsigned char* dev, const JpegEncPlan& P) {
    JpegEncLaunch e{};
    e.images = reinterpret_cast<const JpegEncImage*>(dev + P.images);
    e.block_start = reinterpret_cast<const unsigned*>(dev + P.bstart); e.chunk_start = reinterpret_cast<const unsigned*>(dev + P.cstart);
    e.qtables = reinterpret_cast<const uint16_t*>(dev + P.qt); e.huff = reinterpret_cast<const unsigned*>(dev + P.huff);
    e.coef = reinterpret_cast<int16_t*>(dev + P.coef);
    e.bits = reinterpret_cast<unsigned*>(dev + P.bits); e.offs = reinterpret_cast<unsigned*>(dev + P.offs);
    e.istart = reinterpret_cast<unsigned*>(dev + P.istart);
    e.ulen = reinterpret_cast<unsigned*>(dev + P.ulen); e.slen = reinterpret_cast<unsigned*>(dev + P.slen);
    e.ffbase = reinterpret_cast<unsigned*>(dev + P.ffbase);
    e.workspace = dev;
    e.n_images = (int)P.geom.size(); e.total_blocks = (unsigned)P.blocks; e.total_chunks = (unsigned)P.chunks;
    return e;
}

// checks, then the batch's one upload.  Nothing is enqueued before every image has been checked.
static int jpeg_enc_prepare(lwp_handle h, int N, const unsigned char* const* frames, int mem, const int* heights, const int* widths,
                            int quality, int subsampling, int restart_interval, JpegEncBatch* B) {
    char msg[kJpegMsg];
    if (!h) return fail(h, LWP_ERR_ARG, "handle is null");
    if (!frames || !heights || !widths) return fail(h, LWP_ERR_ARG, "frames / heights / widths is null");
    if (N < 1 || N > 65535) return fail(h, LWP_ERR_ARG, "N must be 1..65535");
    if (mem != LWP_MEM_HOST && mem != LWP_MEM_DEVICE) return fail(h, LWP_ERR_ARG, "mem must be LWP_MEM_HOST or LWP_MEM_DEVICE");
    if (quality < 1 || quality > 100) return fail(h, LWP_ERR_ARG, "jpeg encode: quality must be 1..100");
    if (subsampling < 0 || subsampling > 2) return fail(h, LWP_ERR_ARG, "jpeg encode: subsampling must be LWP_JPEG_444, LWP_JPEG_422 or LWP_JPEG_420");
    if (restart_interval < 0 || restart_interval > 65535) return fail(h, LWP_ERR_ARG, "jpeg encode: restart_interval must be 0..65535 MCUs");
    const JpegEncPlan& P = B->P;
    int rc = jpeg_enc_plan(N, frames, mem == LWP_MEM_HOST, heights, widths, subsampling, restart_interval, &B->P, msg);
    if (rc) return jpeg_fail(h, rc, msg);
    unsigned char *host = nullptr, *dev = nullptr;
    rc = jpeg_stage_begin(h, h->jpeg_enc, P.upload, &host);
    if (rc) return rc;
    rc = jpeg_stage_send(h, h->jpeg_enc, P.upload, P.total, false, &dev,
                         [&](unsigned char* d) { jpeg_enc_fill(P, frames, mem == LWP_MEM_HOST, heights, widths, quality, d, host); });
    if (rc) return rc;
    B->e = jpeg_enc_launch(dev, P);
    return LWP_OK;
}

// stage A alone ...
static int jpeg_enc_enqueue_dct(lwp_handle h, const JpegEncBatch& B) {
    LAUNCH(h, KC_OTHER, launch_jpeg_enc_dct(B.e, h->stream));
    return LWP_OK;
}

// ... and behind it the entropy code of whatever B.e.coef holds: stages B and C, the memset of the un-stuffed scans, D, E, F
static int jpeg_enc_enqueue_entropy(lwp_handle h, const JpegEncBatch& B) {
    LAUNCH(h, KC_OTHER, launch_jpeg_enc_lengths(B.e, h->stream));
    LAUNCH(h, KC_OTHER, launch_jpeg_enc_offsets(B.e, h->stream));
    HIP_TRY(h, hipMemsetAsync(B.e.workspace + B.P.ubytes, 0, B.P.ubytes_total, h->stream));
    LAUNCH(h, KC_OTHER, launch_jpeg_enc_write(B.e, h->stream));
    LAUNCH(h, KC_OTHER, launch_jpeg_enc_stuff_scan(B.e, h->stream));
    LAUNCH(h, KC_OTHER, launch_jpeg_enc_stuff(B.e, h->stream));
    return LWP_OK;
}

// the six stages, in order, on the handle's stream
static int jpeg_enc_enqueue(lwp_handle h, const JpegEncBatch& B) {
    const int rc = jpeg_enc_enqueue_dct(h, B);
    return rc ? rc : jpeg_enc_enqueue_entropy(h, B);
}

// Behind the enqueue: the one wait of the call, for the N stuffed lengths, which are checked against the bound and, where
// out[i] is set, against cap[i] (what the caller writes of image i takes `around` bytes more than its scan); then the scans of
// those images come to the staging, scan[i] bytes at *host + at[i].  Nothing has been written to any out[i] when this fails.
static int jpeg_enc_fetch(lwp_handle h, const JpegEncBatch& B, unsigned char* const* out, const size_t* cap, size_t around,
                          std::vector<size_t>* scan_out, std::vector<size_t>* at_out, unsigned char** host_out) {
    const int N = (int)B.P.geom.size();
    // the staging's front part is free again: the upload ran in front of the kernels
    unsigned* lens = h->jpeg_enc.stage.as<unsigned>();
    HIP_TRY(h, hipMemcpyAsync(lens, B.e.slen, (size_t)N * 4, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    std::vector<size_t>& scan = *scan_out;
    std::vector<size_t>& at = *at_out;
    scan.assign((size_t)N, 0); at.assign((size_t)N, 0);
    size_t stage = 0;
    for (int i = 0; i < N; ++i) {
        scan[i] = lens[i];
        if (scan[i] > jpeg_enc_scan_bound(B.P.geom[i])) {
            char msg[160];
            snprintf(msg, sizeof msg, "image %d: jpeg encode: a scan of %zu bytes where %zu is the most possible", i, scan[i], jpeg_enc_scan_bound(B.P.geom[i]));
            return fail(h, LWP_ERR_INTERNAL, msg);
        }
        at[i] = stage;
        if (out[i]) stage += (scan[i] + 15) & ~(size_t)15;
    }
    for (int i = 0; i < N; ++i)
        if (out[i] && cap[i] < around + scan[i]) {
            char msg[160];
            snprintf(msg, sizeof msg, "image %d: jpeg encode: the %s takes %zu bytes, cap is %zu", i, around ? "file" : "scan", around + scan[i], cap[i]);
            return fail(h, LWP_ERR_CAPACITY, msg);
        }
    HIP_TRY(h, h->jpeg_enc.stage.ensure(stage));
    unsigned char* host = h->jpeg_enc.stage.as<unsigned char>();
    for (int i = 0; i < N; ++i)
        if (out[i] && scan[i]) HIP_TRY(h, hipMemcpyAsync(host + at[i], B.e.workspace + B.P.sbytes[i], scan[i], hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    *host_out = host;
    return LWP_OK;
}

extern "C" int lwp_jpeg_encode_batch(lwp_handle h, int N, const unsigned char* const* frames, int mem, const int* heights, const int* widths,
                                     int quality, int subsampling, int restart_interval, unsigned char* const* out, const size_t* cap,
                                     size_t* len_out) {
    if (!out || !cap || !len_out) return fail(h, LWP_ERR_ARG, "out / cap / len_out is null");
    JpegEncBatch B;
    int rc = jpeg_enc_prepare(h, N, frames, mem, heights, widths, quality, subsampling, restart_interval, &B);
    if (rc) return rc;
    rc = jpeg_enc_enqueue(h, B);
    if (rc) return rc;
    unsigned char hd[kJpegEncHeaderMax];
    const size_t hd_len = jpeg_enc_header(heights[0], widths[0], quality, subsampling, restart_interval, hd);      // the same for every size
    std::vector<size_t> scan, at;
    unsigned char* host = nullptr;
    rc = jpeg_enc_fetch(h, B, out, cap, hd_len + 2, &scan, &at, &host);
    if (rc) return rc;
    for (int i = 0; i < N; ++i) {
        len_out[i] = hd_len + scan[i] + 2;
        if (!out[i]) continue;
        jpeg_enc_header(heights[i], widths[i], quality, subsampling, restart_interval, out[i]);
        memcpy(out[i] + hd_len, host + at[i], scan[i]);
        out[i][hd_len + scan[i]] = 0xFF; out[i][hd_len + scan[i] + 1] = 0xD9;
    }
    return LWP_OK;
}

extern "C" int lwp_debug_jpeg_encode_blocks(lwp_handle h, int N, const unsigned char* const* frames, int mem, const int* heights,
                                            const int* widths, int quality, int subsampling, int16_t* const* coef_out, uint16_t* qtables_out) {
    if (!coef_out || !qtables_out) return fail(h, LWP_ERR_ARG, "coef_out / qtables_out is null");
    JpegEncBatch B;
    int rc = jpeg_enc_prepare(h, N, frames, mem, heights, widths, quality, subsampling, 0, &B);
    if (rc) return rc;
    for (int i = 0; i < N; ++i)
        if (!coef_out[i]) return fail(h, LWP_ERR_ARG, "coef_out holds a null pointer");
    rc = jpeg_enc_enqueue_dct(h, B);
    if (rc) return rc;
    size_t b0 = 0;
    for (int i = 0; i < N; ++i) {
        HIP_TRY(h, hipMemcpyAsync(coef_out[i], B.e.coef + b0 * 64, (size_t)B.P.geom[i].total_blocks * 128, hipMemcpyDeviceToHost, h->stream));
        b0 += (size_t)B.P.geom[i].total_blocks;
    }
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    memset(qtables_out, 0, (size_t)kJpegQuantSlots * 64 * sizeof(uint16_t));
    jpeg_enc_quant_tables(quality, reinterpret_cast<uint16_t(*)[64]>(qtables_out));
    return LWP_OK;
}

// the other stages alone: the caller's coefficients in stage A's place
extern "C" int lwp_debug_jpeg_encode_scan(lwp_handle h, int N, const int16_t* const* coef, const int* heights, const int* widths,
                                          int subsampling, int restart_interval, unsigned char* const* out, const size_t* cap,
                                          size_t* len_out) {
    if (!h) return fail(h, LWP_ERR_ARG, "handle is null");
    if (!coef || !heights || !widths || !out || !cap || !len_out) return fail(h, LWP_ERR_ARG, "coef / heights / widths / out / cap / len_out is null");
    if (N < 1 || N > 65535) return fail(h, LWP_ERR_ARG, "N must be 1..65535");
    // the kernels' contract, which stage A keeps by construction: a DC of -1024..1023, AC terms of -1023..1023
    for (int i = 0; i < N; ++i) {
        char msg[200];
        JpegEncGeom g;
        if (!coef[i]) { snprintf(msg, sizeof msg, "image %d: coef is null", i); return fail(h, LWP_ERR_ARG, msg); }
        if (!jpeg_enc_geometry(heights[i], widths[i], subsampling, restart_interval, &g)) {
            snprintf(msg, sizeof msg, "image %d: jpeg encode: %d x %d: height and width must be 1..65535, subsampling 0..2, restart_interval 0..65535",
                     i, heights[i], widths[i]);
            return fail(h, LWP_ERR_ARG, msg);
        }
        for (size_t k = 0; k < (size_t)g.total_blocks * 64; ++k) {
            const int v = coef[i][k];
            if (v > 1023 || v < (k & 63 ? -1023 : -1024)) {
                snprintf(msg, sizeof msg, "image %d: jpeg encode: coefficient %d of block %zu is %d: a DC must be -1024..1023, an AC term -1023..1023",
                         i, (int)(k & 63), k >> 6, v);
                return fail(h, LWP_ERR_ARG, msg);
            }
        }
    }
    JpegEncBatch B;
    // the records want frame addresses; stage A, the one reader of them, does not run: the coefficients' own stand in
    int rc = jpeg_enc_prepare(h, N, reinterpret_cast<const unsigned char* const*>(coef), LWP_MEM_DEVICE, heights, widths, 100, subsampling,
                              restart_interval, &B);
    if (rc) return rc;
    size_t b0 = 0;
    for (int i = 0; i < N; ++i) {
        HIP_TRY(h, hipMemcpyAsync(B.e.coef + b0 * 64, coef[i], (size_t)B.P.geom[i].total_blocks * 128, hipMemcpyHostToDevice, h->stream));
        b0 += (size_t)B.P.geom[i].total_blocks;
    }
    rc = jpeg_enc_enqueue_entropy(h, B);
    if (rc) return rc;
    std::vector<size_t> scan, at;
    unsigned char* host = nullptr;
    rc = jpeg_enc_fetch(h, B, out, cap, 0, &scan, &at, &host);
    if (rc) return rc;
    for (int i = 0; i < N; ++i) {
        len_out[i] = scan[i];
        if (out[i]) memcpy(out[i], host + at[i], scan[i]);
    }
    return LWP_OK;
}

extern "C" int lwp_time_jpeg_encode_batch(lwp_handle h, int N, const unsigned char* const* frames, int mem, const int* heights,
                                          const int* widths, int quality, int subsampling, int restart_interval, int iters, float* ms_total) {
    if (iters < 1 || !ms_total) return fail(h, LWP_ERR_ARG, "iters must be at least 1 and ms_total non-null");
    JpegEncBatch B;
    int rc = jpeg_enc_prepare(h, N, frames, mem, heights, widths, quality, subsampling, restart_interval, &B);
    if (rc) return rc;
    rc = jpeg_enc_enqueue(h, B);                       // every stage has its inputs, whatever order the windows below run in
    if (rc) return rc;
    rc = time_on_stream(h, iters, [&]() { LAUNCH(h, KC_OTHER, launch_jpeg_enc_dct(B.e, h->stream)); return (int)LWP_OK; }, &ms_total[0]);
    if (rc) return rc;
    rc = time_on_stream(h, iters, [&]() { LAUNCH(h, KC_OTHER, launch_jpeg_enc_lengths(B.e, h->stream)); return (int)LWP_OK; }, &ms_total[1]);
    if (rc) return rc;
    rc = time_on_stream(h, iters, [&]() { LAUNCH(h, KC_OTHER, launch_jpeg_enc_offsets(B.e, h->stream)); return (int)LWP_OK; }, &ms_total[2]);
    if (rc) return rc;
    rc = time_on_stream(h, iters, [&]() {
        HIP_TRY(h, hipMemsetAsync(B.e.workspace + B.P.ubytes, 0, B.P.ubytes_total, h->stream));
        LAUNCH(h, KC_OTHER, launch_jpeg_enc_write(B.e, h->stream));
        return (int)LWP_OK;
    }, &ms_total[3]);
    if (rc) return rc;
    rc = time_on_stream(h, iters, [&]() { LAUNCH(h, KC_OTHER, launch_jpeg_enc_stuff_scan(B.e, h->stream)); return (int)LWP_OK; }, &ms_total[4]);
    if (rc) return rc;
    return time_on_stream(h, iters, [&]() { LAUNCH(h, KC_OTHER, launch_jpeg_enc_stuff(B.e, h->stream)); return (int)LWP_OK; }, &ms_total[5]);
}

// ---------------------------------------------------------------------------------------------- training augmentation
// argument checks, then the batch's one upload: the plan records (their pointers rewritten to device addresses) followed by
// every host image and mask; shared by lwp_augment_batch and lwp_time_augment_batch.  With `crowd` (lwp_augment_batch_crowd)
// the run tables of the crowd masks ride in the same upload, the masks' workspace lies behind it in the same allocation, and
// the records of the samples that have segmentations point into it
static int augment_prepare(lwp_handle h, const lwp_augment_plan* plans, int N, int crop_h, int crop_w, int stride, float* image_out,
                           unsigned char* mask_out, float* mask_small_out, const lwp_augment_plan** plans_device,
                           const CrowdRuns* crowd = nullptr, CrowdLaunch* crowd_launch = nullptr) {
    char msg[200];
    if (!plans || !image_out || !mask_out || !mask_small_out) return fail(h, LWP_ERR_ARG, "plans / image_out / mask_out / mask_small_out is null");
    if (N < 1 || N > 65535) return fail(h, LWP_ERR_ARG, "N must be 1..65535");
    if (stride < 1 || stride > 1024) return fail(h, LWP_ERR_ARG, "stride must be 1..1024");
    if (crop_h < 1 || crop_w < 1 || crop_h >= 32768 || crop_w >= 32768) return fail(h, LWP_ERR_ARG, "the crop must be 1..32767 pixels a side");
    if (crop_h % stride || crop_w % stride) {
        snprintf(msg, sizeof msg, "a %d x %d crop is not a whole number of %d x %d blocks", crop_h, crop_w, stride, stride);
        return fail(h, LWP_ERR_ARG, msg);
    }
    auto bad = [&](int f, const char* what) {
        snprintf(msg, sizeof msg, "sample %d: %s", f, what);
        return fail(h, LWP_ERR_ARG, msg);
    };
    auto dim_ok = [](int v) { return v >= 1 && v < 32768; };
    size_t bytes = ((size_t)N * sizeof(lwp_augment_plan) + 15) & ~(size_t)15;
    for (int f = 0; f < N; ++f) {
        const lwp_augment_plan& p = plans[f];
        if (!p.image) return bad(f, "the image is null");
        if (p.mem != LWP_MEM_HOST && p.mem != LWP_MEM_DEVICE) return bad(f, "mem must be LWP_MEM_HOST or LWP_MEM_DEVICE");
        if (!dim_ok(p.src_h) || !dim_ok(p.src_w) || !dim_ok(p.rs_h) || !dim_ok(p.rs_w) || !dim_ok(p.bound_h) || !dim_ok(p.bound_w))
            return bad(f, "a source, resized or bound size is outside 1..32767 (OpenCV saturates coordinates to short at 32768)");
        if (!(p.rs_scale > 0) || !std::isfinite(p.rs_scale)) return bad(f, "rs_scale must be positive and finite");
        for (int i = 0; i < 6; ++i)
            if (!std::isfinite(p.m[i])) return bad(f, "a matrix value is not finite");
        if ((p.area != 0 && p.area != 1) || (p.flip != 0 && p.flip != 1) || (p.should_crop != 0 && p.should_crop != 1))
            return bad(f, "area, flip and should_crop must be 0 or 1");
        if (p.should_crop) {
            if (p.dst_y0 < 0 || p.dst_y1 < p.dst_y0 || p.dst_y1 > crop_h || p.dst_x0 < 0 || p.dst_x1 < p.dst_x0 || p.dst_x1 > crop_w)
                return bad(f, "the dst rectangle lies outside the crop");
            const int ny = p.dst_y1 - p.dst_y0, nx = p.dst_x1 - p.dst_x0;
            if (ny > 0 && nx > 0 &&
                (p.img_y0 < 0 || p.img_x0 < 0 || p.img_y0 + ny > p.bound_h || p.img_x0 + nx > p.bound_w))
                return bad(f, "the dst rectangle's source lies outside the bound");
        }
        if (p.mem == LWP_MEM_HOST) {
            bytes += ((size_t)p.src_h * p.src_w * 3 + 15) & ~(size_t)15;
            if (p.mask) bytes += ((size_t)p.src_h * p.src_w * sizeof(float) + 15) & ~(size_t)15;
        }
    }
    auto size_of = [&](int f, int* ih, int* iw) { *ih = plans[f].src_h; *iw = plans[f].src_w; };
    auto has_segs = [&](int f) { return crowd->image_seg_off[f + 1] > crowd->image_seg_off[f]; };
    CrowdTables tab;
    std::vector<int64_t> ws_off;                       // float offset of a sample's rendered mask in the workspace
    const size_t tab_at = bytes;
    size_t ws_at = bytes, total = bytes;
    if (crowd) {
        int rc = crowd_check(h, *crowd, N, size_of, has_segs, &tab);
        if (rc) return rc;
        ws_off.assign((size_t)N + 1, 0);
        for (int f = 0; f < N; ++f) {
            if (has_segs(f) && plans[f].mask) return bad(f, "a sample with segmentations must have a null mask");
            ws_off[f + 1] = ws_off[f] + (has_segs(f) ? (int64_t)plans[f].src_h * plans[f].src_w : 0);
        }
        bytes += tab.bytes;
        ws_at = (bytes + 255) & ~(size_t)255;
        total = ws_at + (size_t)ws_off[N] * sizeof(float);
    }
    if (!h) return fail(h, LWP_ERR_ARG, "handle is null");
    HIP_TRY(h, hipSetDevice(h->device));
    int rc = order_in(h);
    if (rc) return rc;
    if (h->d_augment.size() < total) {
        HIP_TRY(h, hipStreamSynchronize(h->stream));   // an earlier launch may still read the old buffer
        HIP_TRY(h, h->d_augment.ensure(total));
    }
    h->augment_stage.resize(bytes);
    unsigned char* host = h->augment_stage.data();
    unsigned char* dev = h->d_augment.as<unsigned char>();
    lwp_augment_plan* recs = reinterpret_cast<lwp_augment_plan*>(host);
    size_t at = ((size_t)N * sizeof(lwp_augment_plan) + 15) & ~(size_t)15;
    if (crowd)
        *crowd_launch = crowd_pack(tab, *crowd, N, size_of, has_segs, [&](int f) { return ws_off[f]; }, host + tab_at, dev + tab_at,
                                   reinterpret_cast<float*>(dev + ws_at));
    for (int f = 0; f < N; ++f) {
        recs[f] = plans[f];
        if (crowd && has_segs(f)) recs[f].mask = reinterpret_cast<const float*>(dev + ws_at) + ws_off[f];
        if (plans[f].mem != LWP_MEM_HOST) continue;
        const size_t ib = (size_t)plans[f].src_h * plans[f].src_w * 3, mb = (size_t)plans[f].src_h * plans[f].src_w * sizeof(float);
        memcpy(host + at, plans[f].image, ib);
        recs[f].image = dev + at;
        at += (ib + 15) & ~(size_t)15;
        if (plans[f].mask) {
            memcpy(host + at, plans[f].mask, mb);
            recs[f].mask = reinterpret_cast<const float*>(dev + at);
            at += (mb + 15) & ~(size_t)15;
        }
    }
    HIP_TRY(h, hipMemcpyAsync(dev, host, bytes, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));       // the staging vector and the caller's arrays are free from here on
    *plans_device = reinterpret_cast<const lwp_augment_plan*>(dev);
    return LWP_OK;
}

extern "C" int lwp_augment_batch(lwp_handle h, const lwp_augment_plan* plans, int N, int crop_h, int crop_w, int stride,
                                 float* image_out, unsigned char* mask_out, float* mask_small_out) {
    const lwp_augment_plan* d_plans = nullptr;
    int rc = augment_prepare(h, plans, N, crop_h, crop_w, stride, image_out, mask_out, mask_small_out, &d_plans);
    if (rc) return rc;
    LAUNCH(h, KC_OTHER, launch_augment(d_plans, N, crop_h, crop_w, stride, image_out, mask_out, mask_small_out, h->stream));
    bool ordered = false;
    rc = order_out(h, h->stream, &ordered);
    if (rc) return rc;
    if (!ordered) HIP_TRY(h, hipStreamSynchronize(h->stream));
    return LWP_OK;
}

extern "C" int lwp_augment_batch_crowd(lwp_handle h, const lwp_augment_plan* plans, int N, int crop_h, int crop_w, int stride,
                                       const int64_t* counts, const int64_t* seg_off, const int64_t* image_seg_off, float* image_out,
                                       unsigned char* mask_out, float* mask_small_out) {
    const lwp_augment_plan* d_plans = nullptr;
    const CrowdRuns runs{counts, seg_off, image_seg_off};
    CrowdLaunch c{};
    int rc = augment_prepare(h, plans, N, crop_h, crop_w, stride, image_out, mask_out, mask_small_out, &d_plans, &runs, &c);
    if (rc) return rc;
    LAUNCH(h, KC_OTHER, launch_crowd_masks(c, h->stream));           // the same stream: the augment kernel reads finished masks
    LAUNCH(h, KC_OTHER, launch_augment(d_plans, N, crop_h, crop_w, stride, image_out, mask_out, mask_small_out, h->stream));
    bool ordered = false;
    rc = order_out(h, h->stream, &ordered);
    if (rc) return rc;
    if (!ordered) HIP_TRY(h, hipStreamSynchronize(h->stream));
    return LWP_OK;
}

// ---------------------------------------------------------------------------------------------- COCO key-point evaluation
// the device memory of one evaluation: released when it goes out of scope, whatever way the call ends
struct CocoEvalRun {
    DevBuf in, scratch;
    CocoEvalParams p{};
    std::vector<int64_t> sel_off, oks_off;
    std::vector<unsigned char> stage;                  // host side of the upload: alive until the run has synchronised
    // the accumulation's order (not needed by the debug twin)
    unsigned long long *keys = nullptr, *keys_out = nullptr;
    unsigned int *vals = nullptr, *perm = nullptr;
    void* sort_tmp = nullptr; size_t sort_tmp_bytes = 0;
};

struct CocoEvalInput {
    int n_images;
    const int64_t* dt_off; const double* dt_kp; const double* dt_score;
    const int64_t* gt_off; const double* gt_kp; const double* gt_area; const double* gt_bbox; const int* gt_iscrowd; const int* gt_ignore;
};

// gt_only: the ground-truth half alone (lwp_coco_open), same rules and wording
static int coco_eval_check(lwp_handle h, const CocoEvalInput& in, bool gt_only = false) {
    char msg[200];
    if (gt_only ? !in.gt_off : (!in.dt_off || !in.gt_off)) return fail(h, LWP_ERR_ARG, gt_only ? "gt_off is null" : "dt_off / gt_off is null");
    if (in.n_images < 1) return fail(h, LWP_ERR_ARG, "n_images must be at least 1");
    const int64_t lim = (int64_t)1 << 31;
    for (int pass = gt_only ? 1 : 0; pass < 2; ++pass) {
        const int64_t* off = pass ? in.gt_off : in.dt_off;
        const char* what = pass ? "gt_off" : "dt_off";
        if (off[0] != 0) { snprintf(msg, sizeof msg, "%s[0] must be 0", what); return fail(h, LWP_ERR_ARG, msg); }
        for (int i = 0; i < in.n_images; ++i)
            if (off[i + 1] < off[i]) { snprintf(msg, sizeof msg, "%s descends at image %d", what, i); return fail(h, LWP_ERR_ARG, msg); }
        if (off[in.n_images] >= lim) { snprintf(msg, sizeof msg, "%s: 2^31 rows or more", what); return fail(h, LWP_ERR_ARG, msg); }
    }
    const int64_t ND = gt_only ? 0 : in.dt_off[in.n_images], NG = in.gt_off[in.n_images];
    if (ND > 0 && (!in.dt_kp || !in.dt_score)) return fail(h, LWP_ERR_ARG, "dt_kp / dt_score is null");
    if (NG > 0 && (!in.gt_kp || !in.gt_area || !in.gt_bbox || !in.gt_iscrowd || !in.gt_ignore))
        return fail(h, LWP_ERR_ARG, "gt_kp / gt_area / gt_bbox / gt_iscrowd / gt_ignore is null");
    auto finite = [](const double* v, int64_t n) {
        for (int64_t i = 0; i < n; ++i) if (!std::isfinite(v[i])) return false;
        return true;
    };
    if (!finite(in.dt_score, ND)) return fail(h, LWP_ERR_ARG, "a detection score is not finite");
    if (!finite(in.dt_kp, ND * kEvalK * 3)) return fail(h, LWP_ERR_ARG, "a detection coordinate is not finite");
    if (!finite(in.gt_kp, NG * kEvalK * 3)) return fail(h, LWP_ERR_ARG, "a ground-truth coordinate is not finite");
    if (!finite(in.gt_area, NG)) return fail(h, LWP_ERR_ARG, "a ground-truth area is not finite");
    if (!finite(in.gt_bbox, NG * 4)) return fail(h, LWP_ERR_ARG, "a ground-truth box is not finite");
    return LWP_OK;
}

// first selected detection and first OKS entry of every image, the defaults and the sizes: what both ways of staging share
static void coco_eval_offsets(int n, const int64_t* dt_off, const int64_t* gt_off, CocoEvalRun* run) {
    run->sel_off.assign((size_t)n + 1, 0);
    run->oks_off.assign((size_t)n + 1, 0);
    for (int i = 0; i < n; ++i) {
        const int64_t D = dt_off[i + 1] - dt_off[i], G = gt_off[i + 1] - gt_off[i];
        const int64_t Ds = std::min<int64_t>(D, kEvalMaxDets);
        run->sel_off[i + 1] = run->sel_off[i] + Ds;
        run->oks_off[i + 1] = run->oks_off[i] + Ds * G;
    }
    coco_eval_defaults(&run->p);
    run->p.n_images = n; run->p.NG = gt_off[n]; run->p.NS = run->sel_off[n];
}

static int coco_eval_launch(lwp_handle h, bool with_order, CocoEvalRun* run);
static int coco_eval_accumulate(lwp_handle h, const CocoEvalRun& run, double* precision, double* recall, double* scores, int64_t* npig);

// "stage the inputs" of lwp_coco_eval and its debug twin: checks and the one upload of host arrays; then "scratch + launch"
// (coco_eval_launch: scratch and the per-image kernel; with_order: the sort buffers of the accumulation too), which
// lwp_coco_finish shares
static int coco_eval_match(lwp_handle h, const CocoEvalInput& in, bool with_order, CocoEvalRun* run) {
    int rc = coco_eval_check(h, in);
    if (rc) return rc;
    if (!h) return fail(h, LWP_ERR_ARG, "handle is null");
    HIP_TRY(h, hipSetDevice(h->device));
    rc = order_in(h);
    if (rc) return rc;
    const int n = in.n_images;
    const int64_t ND = in.dt_off[n], NG = in.gt_off[n];
    coco_eval_offsets(n, in.dt_off, in.gt_off, run);
    CocoEvalParams& p = run->p;

    // sections of the allocation, each 16-byte aligned
    Layout lay;
    const size_t nb = ((size_t)n + 1) * sizeof(int64_t);
    const size_t i_dt_off = lay.take<char>(nb), i_gt_off = lay.take<char>(nb), i_sel_off = lay.take<char>(nb), i_oks_off = lay.take<char>(nb);
    const size_t i_dt_kp = lay.take<char>((size_t)ND * kEvalK * 3 * 8), i_dt_score = lay.take<char>((size_t)ND * 8);
    const size_t i_gt_kp = lay.take<char>((size_t)NG * kEvalK * 3 * 8), i_gt_area = lay.take<char>((size_t)NG * 8), i_gt_bbox = lay.take<char>((size_t)NG * 4 * 8);
    const size_t i_gt_crowd = lay.take<char>((size_t)NG * 4), i_gt_ignore = lay.take<char>((size_t)NG * 4);
    const size_t in_bytes = std::max<size_t>(lay.align(), 16);
    std::vector<unsigned char>& stage = run->stage;
    stage.assign(in_bytes, 0);
    auto put = [&](size_t off, const void* src, size_t bytes) { if (bytes) memcpy(stage.data() + off, src, bytes); };
    put(i_dt_off, in.dt_off, nb); put(i_gt_off, in.gt_off, nb); put(i_sel_off, run->sel_off.data(), nb); put(i_oks_off, run->oks_off.data(), nb);
    put(i_dt_kp, in.dt_kp, (size_t)ND * kEvalK * 3 * 8); put(i_dt_score, in.dt_score, (size_t)ND * 8);
    put(i_gt_kp, in.gt_kp, (size_t)NG * kEvalK * 3 * 8); put(i_gt_area, in.gt_area, (size_t)NG * 8); put(i_gt_bbox, in.gt_bbox, (size_t)NG * 4 * 8);
    put(i_gt_crowd, in.gt_iscrowd, (size_t)NG * 4); put(i_gt_ignore, in.gt_ignore, (size_t)NG * 4);
    HIP_TRY(h, run->in.ensure(in_bytes));
    unsigned char* di = run->in.as<unsigned char>();
    HIP_TRY(h, hipMemcpyAsync(di, stage.data(), in_bytes, hipMemcpyHostToDevice, h->stream));
    p.dt_off = (const int64_t*)(di + i_dt_off); p.gt_off = (const int64_t*)(di + i_gt_off);
    p.sel_off = (const int64_t*)(di + i_sel_off); p.oks_off = (const int64_t*)(di + i_oks_off);
    p.dt_kp = (const double*)(di + i_dt_kp); p.dt_score = (const double*)(di + i_dt_score);
    p.gt_kp = (const double*)(di + i_gt_kp); p.gt_area = (const double*)(di + i_gt_area); p.gt_bbox = (const double*)(di + i_gt_bbox);
    p.gt_iscrowd = (const int*)(di + i_gt_crowd); p.gt_ignore = (const int*)(di + i_gt_ignore);
    return coco_eval_launch(h, with_order, run);
}

// run->p holds the sizes and the input pointers (host arrays staged by coco_eval_match, or the store's by lwp_coco_finish)
static int coco_eval_launch(lwp_handle h, bool with_order, CocoEvalRun* run) {
    CocoEvalParams& p = run->p;
    const int n = p.n_images;
    const int64_t NG = p.NG, NS = p.NS, NO = run->oks_off[n];
    Layout lay;
    const size_t s_gt_m = lay.take<char>((size_t)kEvalAT * NG);                       // first: the part that is zeroed
    const size_t zero_bytes = lay.align();
    const size_t s_sel_idx = lay.take<char>((size_t)NS * 4), s_sel_score = lay.take<char>((size_t)NS * 8), s_oks = lay.take<char>((size_t)NO * 8);
    const size_t s_gt_flag = lay.take<char>((size_t)NG), s_dt_m = lay.take<char>((size_t)kEvalAT * NS), s_dt_ig = lay.take<char>((size_t)kEvalAT * NS);
    const size_t s_npig_img = lay.take<char>((size_t)n * kEvalA * 4);
    const size_t s_out = lay.take<char>(((size_t)2 * kEvalT * kEvalR * kEvalA + kEvalT * kEvalA) * 8 + kEvalA * 8);
    size_t s_keys = 0, s_keys_out = 0, s_vals = 0, s_perm = 0, s_tpfp = 0, s_pr = 0, s_tmp = 0;
    if (with_order) {
        HIP_TRY(h, coco_sort_temp_bytes(NS, &run->sort_tmp_bytes));
        s_keys = lay.take<char>((size_t)NS * 8); s_keys_out = lay.take<char>((size_t)NS * 8); s_vals = lay.take<char>((size_t)NS * 4); s_perm = lay.take<char>((size_t)NS * 4);
        s_tpfp = lay.take<char>((size_t)kEvalAT * NS * 8); s_pr = lay.take<char>((size_t)kEvalAT * NS * 8);
        s_tmp = lay.take<char>(run->sort_tmp_bytes);
    }
    const size_t scratch_bytes = std::max<size_t>(lay.align(), 16);
    HIP_TRY(h, run->scratch.ensure(scratch_bytes));
    unsigned char* ds = run->scratch.as<unsigned char>();
    if (zero_bytes) HIP_TRY(h, hipMemsetAsync(ds + s_gt_m, 0, zero_bytes, h->stream));
    p.gt_m = ds + s_gt_m; p.sel_idx = (int*)(ds + s_sel_idx); p.sel_score = (double*)(ds + s_sel_score); p.oks = (double*)(ds + s_oks);
    p.gt_flag = ds + s_gt_flag; p.dt_m = ds + s_dt_m; p.dt_ig = ds + s_dt_ig; p.npig_img = (int*)(ds + s_npig_img);
    p.precision = (double*)(ds + s_out); p.scores = p.precision + kEvalT * kEvalR * kEvalA;
    p.recall = p.scores + kEvalT * kEvalR * kEvalA; p.npig = (long long*)(p.recall + kEvalT * kEvalA);
    if (with_order) {
        run->keys = (unsigned long long*)(ds + s_keys); run->keys_out = (unsigned long long*)(ds + s_keys_out);
        run->vals = (unsigned int*)(ds + s_vals); run->perm = (unsigned int*)(ds + s_perm);
        run->sort_tmp = ds + s_tmp;
        p.perm = run->perm; p.tpfp = (unsigned long long*)(ds + s_tpfp); p.pr = (double*)(ds + s_pr);
    }
    LAUNCH(h, KC_OTHER, launch_coco_match(p, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));       // the staging vector is free from here on; a fault of the kernel is reported here
    return LWP_OK;
}

extern "C" int lwp_coco_eval(lwp_handle h, int n_images, const int64_t* dt_off, const double* dt_kp, const double* dt_score,
                             const int64_t* gt_off, const double* gt_kp, const double* gt_area, const double* gt_bbox,
                             const int* gt_iscrowd, const int* gt_ignore, double* precision, double* recall, double* scores,
                             int64_t* npig) {
    if (!precision || !recall || !scores || !npig) return fail(h, LWP_ERR_ARG, "precision / recall / scores / npig is null");
    const CocoEvalInput in{n_images, dt_off, dt_kp, dt_score, gt_off, gt_kp, gt_area, gt_bbox, gt_iscrowd, gt_ignore};
    CocoEvalRun run;
    int rc = coco_eval_match(h, in, true, &run);
    if (rc) return rc;
    return coco_eval_accumulate(h, run, precision, recall, scores, npig);
}

// the order of the selected detections, accumulate, and the one copy back: behind coco_eval_launch(with_order = true)
static int coco_eval_accumulate(lwp_handle h, const CocoEvalRun& run, double* precision, double* recall, double* scores, int64_t* npig) {
    const CocoEvalParams& p = run.p;
    LAUNCH(h, KC_OTHER, launch_coco_sort(p.sel_score, p.NS, run.keys, run.keys_out, run.vals, run.perm, run.sort_tmp, run.sort_tmp_bytes, h->stream));
    LAUNCH(h, KC_OTHER, launch_coco_accumulate(p, h->stream));
    // precision | scores | recall | npig lie back to back
    const size_t n_pr = (size_t)kEvalT * kEvalR * kEvalA, n_rc = (size_t)kEvalT * kEvalA;
    std::vector<double> out(2 * n_pr + n_rc + kEvalA);
    HIP_TRY(h, hipMemcpyAsync(out.data(), p.precision, out.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    memcpy(precision, out.data(), n_pr * sizeof(double));
    memcpy(scores, out.data() + n_pr, n_pr * sizeof(double));
    memcpy(recall, out.data() + 2 * n_pr, n_rc * sizeof(double));
    long long np3[kEvalA];
    memcpy(np3, out.data() + 2 * n_pr + n_rc, sizeof np3);
    for (int a = 0; a < kEvalA; ++a) npig[a] = (int64_t)np3[a];
    return LWP_OK;
}

extern "C" int lwp_debug_coco_oks(lwp_handle h, int n_images, const int64_t* dt_off, const double* dt_kp, const double* dt_score,
                                  const int64_t* gt_off, const double* gt_kp, const double* gt_area, const double* gt_bbox,
                                  const int* gt_iscrowd, const int* gt_ignore, int image, int* n_sel, int* order, double* oks,
                                  int64_t oks_cap, unsigned char* matched, unsigned char* ignored, int* npig3) {
    if (!n_sel || !order || !matched || !ignored || !npig3) return fail(h, LWP_ERR_ARG, "n_sel / order / matched / ignored / npig3 is null");
    const CocoEvalInput in{n_images, dt_off, dt_kp, dt_score, gt_off, gt_kp, gt_area, gt_bbox, gt_iscrowd, gt_ignore};
    int rc = coco_eval_check(h, in);
    if (rc) return rc;
    if (image < 0 || image >= n_images) return fail(h, LWP_ERR_ARG, "image out of range");
    const int64_t D = dt_off[image + 1] - dt_off[image], G = gt_off[image + 1] - gt_off[image];
    const int Ds = (int)std::min<int64_t>(D, kEvalMaxDets);
    if (oks_cap < 0 || (int64_t)Ds * G > oks_cap) return fail(h, LWP_ERR_CAPACITY, "oks_cap is below n_sel * G");
    if (Ds * G > 0 && !oks) return fail(h, LWP_ERR_ARG, "oks is null");
    CocoEvalRun run;
    rc = coco_eval_match(h, in, false, &run);
    if (rc) return rc;
    const CocoEvalParams& p = run.p;
    const int64_t s0 = run.sel_off[image], o0 = run.oks_off[image];
    *n_sel = Ds;
    memset(matched, 0, (size_t)kEvalAT * kEvalMaxDets);
    memset(ignored, 0, (size_t)kEvalAT * kEvalMaxDets);
    for (int r = 0; r < kEvalMaxDets; ++r) order[r] = -1;
    HIP_TRY(h, hipMemcpyAsync(npig3, p.npig_img + (size_t)image * kEvalA, kEvalA * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    if (Ds > 0) {
        HIP_TRY(h, hipMemcpyAsync(order, p.sel_idx + s0, (size_t)Ds * sizeof(int), hipMemcpyDeviceToHost, h->stream));
        if (G > 0) HIP_TRY(h, hipMemcpyAsync(oks, p.oks + o0, (size_t)Ds * G * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        for (int at = 0; at < kEvalAT; ++at) {
            HIP_TRY(h, hipMemcpyAsync(matched + at * kEvalMaxDets, p.dt_m + (size_t)at * p.NS + s0, (size_t)Ds, hipMemcpyDeviceToHost, h->stream));
            HIP_TRY(h, hipMemcpyAsync(ignored + at * kEvalMaxDets, p.dt_ig + (size_t)at * p.NS + s0, (size_t)Ds, hipMemcpyDeviceToHost, h->stream));
        }
    }
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return LWP_OK;
}

// ---------------------------------------------------------------------------------------------- detection store
static void coco_store_free(lwp_context* h) {
    auto& c = h->coco;
    (void)c.gt.reset(); (void)c.rows.reset(); (void)c.meta.reset(); (void)c.ring.reset();
    c.open = false; c.ring_used = 0; c.st = CocoStore(); c.NG = 0;
    c.gt_off.clear(); c.added.clear();
}

extern "C" int lwp_coco_open(lwp_handle h, int n_images, const int64_t* gt_off, const double* gt_kp, const double* gt_area,
                             const double* gt_bbox, const int* gt_iscrowd, const int* gt_ignore, int row_cap) {
    const CocoEvalInput in{n_images, nullptr, nullptr, nullptr, gt_off, gt_kp, gt_area, gt_bbox, gt_iscrowd, gt_ignore};
    int rc = coco_eval_check(h, in, true);
    if (rc) return rc;
    if (row_cap < 0) return fail(h, LWP_ERR_ARG, "row_cap must not be negative");
    if (!h) return fail(h, LWP_ERR_ARG, "handle is null");
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));       // a second open replaces the first: nothing reads the old store any more
    coco_store_free(h);
    auto& c = h->coco;
    const int n = n_images;
    const int64_t NG = gt_off[n];
    Layout lay;
    const size_t nb = ((size_t)n + 1) * sizeof(int64_t);
    const size_t o_off = lay.take<char>(nb);
    c.o_kp = lay.take<char>((size_t)NG * kEvalK * 3 * 8); c.o_area = lay.take<char>((size_t)NG * 8); c.o_bbox = lay.take<char>((size_t)NG * 4 * 8);
    c.o_crowd = lay.take<char>((size_t)NG * 4); c.o_ignore = lay.take<char>((size_t)NG * 4);
    std::vector<unsigned char> stage(std::max<size_t>(lay.align(), 16));
    auto put = [&](size_t off, const void* src, size_t bytes) { if (bytes) memcpy(stage.data() + off, src, bytes); };
    put(o_off, gt_off, nb); put(c.o_kp, gt_kp, (size_t)NG * kEvalK * 3 * 8); put(c.o_area, gt_area, (size_t)NG * 8);
    put(c.o_bbox, gt_bbox, (size_t)NG * 4 * 8); put(c.o_crowd, gt_iscrowd, (size_t)NG * 4); put(c.o_ignore, gt_ignore, (size_t)NG * 4);
    // rows: kp | score | image; tables: control words | count | start
    const size_t R = (size_t)row_cap;
    const size_t r_score = (R * kEvalK * 3 * 8 + 15) & ~(size_t)15, r_image = r_score + ((R * 8 + 15) & ~(size_t)15);
    const size_t rows_bytes = std::max<size_t>(r_image + R * 4, 16);
    const size_t m_count = 4 * sizeof(long long), m_start = m_count + (size_t)n * 4, meta_bytes = m_start + (size_t)n * 4;
    hipError_t e = c.gt.ensure(stage.size());
    if (e == hipSuccess) e = c.rows.ensure(rows_bytes);
    if (e == hipSuccess) e = c.meta.ensure(meta_bytes);
    if (e == hipSuccess) e = hipMemcpyAsync(c.gt.as<void>(), stage.data(), stage.size(), hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipMemsetAsync(c.meta.as<void>(), 0, meta_bytes, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);      // the staging vector goes out of scope
    if (e != hipSuccess) { coco_store_free(h); return fail(h, LWP_ERR_HIP, std::string("lwp_coco_open: ") + hipGetErrorString(e)); }
    char* r = c.rows.as<char>();
    char* m = c.meta.as<char>();
    c.st.kp = (double*)r; c.st.score = (double*)(r + r_score); c.st.image = (int*)(r + r_image);
    c.st.ctl = (long long*)m; c.st.count = (int*)(m + m_count); c.st.start = (int*)(m + m_start);
    c.st.row_cap = row_cap; c.st.n_images = n;
    c.NG = NG;
    c.gt_off.assign(gt_off, gt_off + n + 1);
    c.added.assign((size_t)n, 0);
    c.open = true;
    return LWP_OK;
}

extern "C" int lwp_coco_release(lwp_handle h) {
    if (!h) return fail(h, LWP_ERR_ARG, "handle is null");
    if (!h->coco.open) return LWP_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    coco_store_free(h);
    return LWP_OK;
}

static int coco_need_store(lwp_context* h) {
    if (!h) return fail(h, LWP_ERR_ARG, "handle is null");
    if (!h->coco.open) return fail(h, LWP_ERR_STATE, "no detection store is open (lwp_coco_open)");
    return LWP_OK;
}

extern "C" int lwp_coco_reset(lwp_handle h) {
    int rc = coco_need_store(h);
    if (rc) return rc;
    auto& c = h->coco;
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipMemsetAsync(c.meta.as<void>(), 0, 4 * sizeof(long long) + (size_t)c.st.n_images * 8, h->stream));   // cursor, status, count, start
    c.added.assign(c.added.size(), 0);
    return LWP_OK;
}

// host bytes -> pinned ring -> *dev, the address the kernels of this stream read them at.  The ring is reused from its start
// once it is full, after one synchronise: everything queued so far has read its part by then.
static int coco_ring_put(lwp_context* h, const void* src, size_t bytes, const void** dev) {
    auto& c = h->coco;
    *dev = nullptr;
    if (bytes == 0) return LWP_OK;                     // nothing to carry (an image without a detection): the kernel reads nothing
    const size_t need = (bytes + 15) & ~(size_t)15;
    if (c.ring.size() < need || c.ring_used + need > c.ring.size()) {
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        HIP_TRY(h, c.ring.ensure(std::max<size_t>(need, (size_t)1 << 20)));
        c.ring_used = 0;
    }
    memcpy(c.ring.as<char>() + c.ring_used, src, bytes);
    void* mapped = nullptr;
    HIP_TRY(h, hipHostGetDevicePointer(&mapped, c.ring.as<void>(), 0));
    *dev = (const char*)mapped + c.ring_used;
    c.ring_used += need;
    return LWP_OK;
}

// the image indices of one call: in range, not added before, no index twice
static int coco_add_check(lwp_context* h, int N, const int* image_index) {
    auto& c = h->coco;
    char msg[200];
    for (int f = 0; f < N; ++f) {
        const int i = image_index[f];
        if (i < 0 || i >= c.st.n_images) {
            snprintf(msg, sizeof msg, "image_index[%d] = %d is outside the ground truth's 0..%d", f, i, c.st.n_images - 1);
            return fail(h, LWP_ERR_ARG, msg);
        }
    }
    for (int f = 0; f < N; ++f) {
        const int i = image_index[f];
        bool twice = c.added[i] != 0;
        for (int g = 0; g < f && !twice; ++g) twice = image_index[g] == i;
        if (twice) {
            snprintf(msg, sizeof msg, "image %d was already added (lwp_coco_reset forgets the detections)", i);
            return fail(h, LWP_ERR_STATE, msg);
        }
    }
    return LWP_OK;
}

// the serial workspace holds frames nobody may fetch: as after lwp_track_poses
static void coco_claim_serial_ws(lwp_context* h) {
    h->stage_tail_N = 0; h->run_has_tail = false;
    h->last_N = 0; h->async_pending = false;
}

// the append kernel on the N frames the grouping (or lwp_debug_coco_rows) left in the serial workspace
static int coco_enqueue_append(lwp_context* h, int N, const int* image_index) {
    auto& c = h->coco;
    const void* d_index = nullptr;
    int rc = coco_ring_put(h, image_index, (size_t)N * sizeof(int), &d_index);
    if (rc) return rc;
    const PostWorkspace& w = h->ws;
    CocoAppendParams p{};
    p.flags = w.flags; p.kpts_out = w.kpts_out; p.entries = w.entries; p.n_entries = w.n_entries;
    p.image_index = (const int*)d_index;
    p.N = N; p.max_entries = w.caps.max_entries; p.max_rows = w.K * w.caps.max_kpts;
    LAUNCH(h, KC_POST, launch_coco_append(c.st, p, h->stream));
    for (int f = 0; f < N; ++f) c.added[image_index[f]] = 1;
    return LWP_OK;
}

static int coco_default_skeleton(lwp_context* h) {
    if (!h->skel.is_default || h->skel.K != kCocoTypes || h->skel.E != kCocoEntry)
        return fail(h, LWP_ERR_STATE, "the detection store maps the default skeleton (18 key-point types, rows of 20) to COCO's 17 key-points: a custom skeleton has no mapping");
    return LWP_OK;
}

extern "C" int lwp_coco_add_maps(lwp_handle h, const float* heat, const float* paf, int layout, int N, int hs, int ws, int ratio,
                                 int demo, const int* image_index) {
    if (!heat || !paf || !image_index || N <= 0 || hs <= 0 || ws <= 0) return fail(h, LWP_ERR_ARG, "bad argument");
    if (layout != LWP_LAYOUT_NCHW && layout != LWP_LAYOUT_NHWC) return fail(h, LWP_ERR_ARG, "layout must be LWP_LAYOUT_NCHW or LWP_LAYOUT_NHWC");
    int rc = coco_need_store(h);
    if (rc) return rc;
    rc = check_pose_args(h, ratio, true, (int64_t)hs * ratio, (int64_t)ws * ratio);
    if (rc) return rc;
    rc = coco_add_check(h, N, image_index);
    if (rc) return rc;
    rc = coco_default_skeleton(h);
    if (rc) return rc;
    // the store takes detections, not tracks: the lanes of modes 2 / 3 must not advance on validation frames
    if (h->tail.mode >= 2) return fail(h, LWP_ERR_STATE, "tracking is on (lwp_set_tracking mode 2 or 3): the detection store takes untracked frames only");
    HIP_TRY(h, hipSetDevice(h->device));
    rc = ensure_ws(h, N);
    if (rc) return rc;
    rc = order_in(h);
    if (rc) return rc;
    MapView hv = nchw_view(heat, h->g.NH, hs, ws), pv = nchw_view(paf, h->g.NP, hs, ws);
    if (layout == LWP_LAYOUT_NHWC) {
        hv.ys = (int64_t)ws * h->g.NH; hv.xs = h->g.NH; hv.cs = 1;
        pv.ys = (int64_t)ws * h->g.NP; pv.xs = h->g.NP; pv.cs = 1;
    }
    coco_claim_serial_ws(h);
    rc = enqueue_grouping(h, hv, pv, N, ratio, demo, h->ws, h->stream);
    if (rc == LWP_OK) rc = coco_enqueue_append(h, N, image_index);
    if (rc) return rc;
    bool ordered = false;
    return order_out(h, h->stream, &ordered);          // enqueue only: no synchronise, no fetch
}

extern "C" int lwp_coco_add_rows(lwp_handle h, int image_index, int n, const double* dt_kp, const double* dt_score) {
    if (n < 0) return fail(h, LWP_ERR_ARG, "negative row count");
    if (n > 0 && (!dt_kp || !dt_score)) return fail(h, LWP_ERR_ARG, "dt_kp / dt_score is null");
    for (int64_t i = 0; i < n; ++i) if (!std::isfinite(dt_score[i])) return fail(h, LWP_ERR_ARG, "a detection score is not finite");
    for (int64_t i = 0; i < (int64_t)n * kEvalK * 3; ++i) if (!std::isfinite(dt_kp[i])) return fail(h, LWP_ERR_ARG, "a detection coordinate is not finite");
    int rc = coco_need_store(h);
    if (rc) return rc;
    rc = coco_add_check(h, 1, &image_index);
    if (rc) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    rc = order_in(h);
    if (rc) return rc;
    // key-points and scores travel as one section of the ring
    const size_t kb = (size_t)n * kEvalK * 3 * 8;
    std::vector<double> both((size_t)n * (kEvalK * 3 + 1));
    if (n > 0) { memcpy(both.data(), dt_kp, kb); memcpy(both.data() + (size_t)n * kEvalK * 3, dt_score, (size_t)n * 8); }
    const void* d = nullptr;
    rc = coco_ring_put(h, both.data(), both.size() * 8, &d);
    if (rc) return rc;
    const double* dk = (const double*)d;
    LAUNCH(h, KC_OTHER, launch_coco_append_rows(h->coco.st, image_index, n, dk, dk + (size_t)n * kEvalK * 3, h->stream));
    h->coco.added[image_index] = 1;
    return LWP_OK;
}

// the tables after everything queued so far: ONE copy (control words | counts) and one synchronise; a sticky status is the error
static int coco_tables_parse(lwp_context* h, const std::vector<long long>& buf, std::vector<int>* counts, long long* cursor);
static int coco_tables_copy(lwp_context* h, std::vector<long long>* buf) {
    auto& c = h->coco;
    const int n = c.st.n_images;
    buf->assign(4 + ((size_t)n + 1) / 2, 0);
    HIP_TRY(h, hipMemcpyAsync(buf->data(), c.meta.as<void>(), 4 * sizeof(long long) + (size_t)n * 4, hipMemcpyDeviceToHost, h->stream));
    return LWP_OK;
}
static int coco_fetch_tables(lwp_context* h, std::vector<int>* counts, long long* cursor) {
    std::vector<long long> buf;
    int rc = coco_tables_copy(h, &buf);
    if (rc) return rc;
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return coco_tables_parse(h, buf, counts, cursor);
}
static int coco_tables_parse(lwp_context* h, const std::vector<long long>& buf, std::vector<int>* counts, long long* cursor) {
    auto& c = h->coco;
    const int n = c.st.n_images;
    const long long* ctl = buf.data();
    if (cursor) *cursor = ctl[0];
    char msg[240];
    switch ((int)ctl[1]) {
    case COCO_ST_OK: break;
    case COCO_ST_FLAGS:
        snprintf(msg, sizeof msg, "image %d: post-processing capacity exceeded (bits 0x%llx: 1 peaks, 2 key-points, 4 connections/entries)", (int)ctl[2], (unsigned long long)ctl[3]);
        return fail(h, LWP_ERR_CAPACITY, msg);
    case COCO_ST_UNBOUND:
        return fail(h, LWP_ERR_UNBOUND, "local variable 'ratio' referenced before assignment");
    case COCO_ST_ROWS:
        snprintf(msg, sizeof msg, "the detection store holds %d rows and %lld were added (image %d was the first without room): open it with row_cap >= %lld",
                 c.st.row_cap, ctl[0], (int)ctl[2], ctl[0]);
        return fail(h, LWP_ERR_CAPACITY, msg);
    case COCO_ST_NONFINITE:
        snprintf(msg, sizeof msg, "image %d: a detection coordinate or score is not finite", (int)ctl[2]);
        return fail(h, LWP_ERR_ARG, msg);
    default:
        return fail(h, LWP_ERR_STATE, "the detection store's status word is damaged");
    }
    const int* cnt = (const int*)(buf.data() + 4);
    counts->resize((size_t)n);
    for (int i = 0; i < n; ++i) (*counts)[i] = std::min(std::max(cnt[i], 0), c.st.row_cap);
    return LWP_OK;
}

extern "C" int lwp_coco_counts(lwp_handle h, int64_t* n_rows, int* per_image_counts) {
    if (!n_rows) return fail(h, LWP_ERR_ARG, "n_rows is null");
    int rc = coco_need_store(h);
    if (rc) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    rc = order_in(h);
    if (rc) return rc;
    std::vector<int> counts;
    rc = coco_fetch_tables(h, &counts, nullptr);
    if (rc) return rc;
    int64_t total = 0;
    for (size_t i = 0; i < counts.size(); ++i) { total += counts[i]; if (per_image_counts) per_image_counts[i] = counts[i]; }
    *n_rows = total;
    return LWP_OK;
}

// "stage the inputs" of lwp_coco_finish: the tables, the offsets formed on the host, and the store gathered into CSR order in
// run->in: [dt_off | sel_off | oks_off | dt_kp | dt_score]; the ground truth is the resident one
static int coco_gather_rows(lwp_context* h, CocoEvalRun* run) {
    auto& c = h->coco;
    const int n = c.st.n_images;
    std::vector<int> counts;
    int rc = coco_fetch_tables(h, &counts, nullptr);
    if (rc) return rc;
    std::vector<int64_t> dt_off((size_t)n + 1, 0);
    for (int i = 0; i < n; ++i) dt_off[i + 1] = dt_off[i] + counts[i];
    const int64_t ND = dt_off[n];
    if (ND > c.st.row_cap) return fail(h, LWP_ERR_STATE, "the detection store's counts exceed its rows");
    coco_eval_offsets(n, dt_off.data(), c.gt_off.data(), run);
    Layout lay;
    const size_t nb = ((size_t)n + 1) * sizeof(int64_t);
    const size_t i_dt_off = lay.take<char>(nb), i_sel_off = lay.take<char>(nb), i_oks_off = lay.take<char>(nb);
    const size_t up_bytes = lay.align();
    const size_t i_dt_kp = lay.take<char>((size_t)ND * kEvalK * 3 * 8), i_dt_score = lay.take<char>((size_t)ND * 8);
    run->stage.assign(up_bytes, 0);
    memcpy(run->stage.data() + i_dt_off, dt_off.data(), nb);
    memcpy(run->stage.data() + i_sel_off, run->sel_off.data(), nb);
    memcpy(run->stage.data() + i_oks_off, run->oks_off.data(), nb);
    HIP_TRY(h, run->in.ensure(std::max<size_t>(lay.align(), 16)));
    unsigned char* di = run->in.as<unsigned char>();
    HIP_TRY(h, hipMemcpyAsync(di, run->stage.data(), up_bytes, hipMemcpyHostToDevice, h->stream));
    CocoEvalParams& p = run->p;
    const char* g = c.gt.as<char>();
    p.dt_off = (const int64_t*)(di + i_dt_off); p.sel_off = (const int64_t*)(di + i_sel_off); p.oks_off = (const int64_t*)(di + i_oks_off);
    p.dt_kp = (const double*)(di + i_dt_kp); p.dt_score = (const double*)(di + i_dt_score);
    p.gt_off = (const int64_t*)g; p.gt_kp = (const double*)(g + c.o_kp); p.gt_area = (const double*)(g + c.o_area);
    p.gt_bbox = (const double*)(g + c.o_bbox); p.gt_iscrowd = (const int*)(g + c.o_crowd); p.gt_ignore = (const int*)(g + c.o_ignore);
    LAUNCH(h, KC_OTHER, launch_coco_gather(c.st, p.dt_off, ND, (double*)(di + i_dt_kp), (double*)(di + i_dt_score), nullptr, h->stream));
    return LWP_OK;
}

extern "C" int lwp_coco_rows(lwp_handle h, int* dt_image, double* dt_kp, double* dt_score, int64_t row_cap) {
    if (row_cap < 0) return fail(h, LWP_ERR_ARG, "row_cap must not be negative");
    if (row_cap > 0 && (!dt_image || !dt_kp || !dt_score)) return fail(h, LWP_ERR_ARG, "dt_image / dt_kp / dt_score is null");
    int rc = coco_need_store(h);
    if (rc) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    rc = order_in(h);
    if (rc) return rc;
    // the offsets are formed on the device here, so that the tables and the rows come back behind ONE synchronise: the first
    // `cap` rows of the evaluation's order are gathered and copied, and the counts say afterwards how many of them there are
    auto& c = h->coco;
    const int n = c.st.n_images;
    const size_t cap = (size_t)std::min<int64_t>(row_cap, c.st.row_cap);
    Layout lay;
    const size_t s_off = lay.take<char>(((size_t)n + 1) * 8), s_kp = lay.take<char>(cap * kEvalK * 3 * 8), s_score = lay.take<char>(cap * 8), s_image = lay.take<char>(cap * 4);
    DevBuf scratch;
    HIP_TRY(h, scratch.ensure(std::max<size_t>(lay.align(), 16)));
    char* ds = scratch.as<char>();
    LAUNCH(h, KC_OTHER, launch_coco_offsets(c.st, (int64_t*)(ds + s_off), h->stream));
    LAUNCH(h, KC_OTHER, launch_coco_gather(c.st, (const int64_t*)(ds + s_off), (int64_t)cap, (double*)(ds + s_kp), (double*)(ds + s_score),
                                           (int*)(ds + s_image), h->stream));
    std::vector<long long> tables;
    rc = coco_tables_copy(h, &tables);
    if (rc) return rc;
    std::vector<double> h_kp(cap * kEvalK * 3), h_score(cap);
    std::vector<int> h_image(cap);
    if (cap > 0) {
        HIP_TRY(h, hipMemcpyAsync(h_kp.data(), ds + s_kp, cap * kEvalK * 3 * 8, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipMemcpyAsync(h_score.data(), ds + s_score, cap * 8, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipMemcpyAsync(h_image.data(), ds + s_image, cap * 4, hipMemcpyDeviceToHost, h->stream));
    }
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    std::vector<int> counts;
    rc = coco_tables_parse(h, tables, &counts, nullptr);
    if (rc) return rc;
    int64_t ND = 0;
    for (int v : counts) ND += v;
    if (ND > row_cap) {
        char msg[120];
        snprintf(msg, sizeof msg, "the detection store holds %lld rows, the arrays %lld", (long long)ND, (long long)row_cap);
        return fail(h, LWP_ERR_CAPACITY, msg);
    }
    if (ND > 0) {
        memcpy(dt_kp, h_kp.data(), (size_t)ND * kEvalK * 3 * 8);
        memcpy(dt_score, h_score.data(), (size_t)ND * 8);
        memcpy(dt_image, h_image.data(), (size_t)ND * 4);
    }
    return LWP_OK;
}

extern "C" int lwp_coco_finish(lwp_handle h, double* precision, double* recall, double* scores, int64_t* npig) {
    if (!precision || !recall || !scores || !npig) return fail(h, LWP_ERR_ARG, "precision / recall / scores / npig is null");
    int rc = coco_need_store(h);
    if (rc) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    rc = order_in(h);
    if (rc) return rc;
    CocoEvalRun run;
    rc = coco_gather_rows(h, &run);
    if (rc) return rc;
    rc = coco_eval_launch(h, true, &run);
    if (rc) return rc;
    return coco_eval_accumulate(h, run, precision, recall, scores, npig);
}

extern "C" int lwp_debug_coco_rows(lwp_handle h, int N, const double* entries, const int* n_entries, const double* kpts,
                                   const int* kpt_counts, const int* image_index) {
    if (N <= 0 || !n_entries || !kpt_counts || !image_index) return fail(h, LWP_ERR_ARG, "bad argument");
    int rc = coco_need_store(h);
    if (rc) return rc;
    rc = coco_default_skeleton(h);
    if (rc) return rc;
    const int max_rows = h->skel.K * h->caps.max_kpts;
    int64_t te = 0, tk = 0;
    for (int f = 0; f < N; ++f) {
        if (n_entries[f] < 0 || kpt_counts[f] < 0) return fail(h, LWP_ERR_ARG, "negative count");
        if (n_entries[f] > h->caps.max_entries || kpt_counts[f] > max_rows) return fail(h, LWP_ERR_CAPACITY, "more rows than the workspace's capacity (lwp_set_capacity)");
        te += n_entries[f]; tk += kpt_counts[f];
    }
    if ((te > 0 && !entries) || (tk > 0 && !kpts)) return fail(h, LWP_ERR_ARG, "entries / kpts is null");
    rc = coco_add_check(h, N, image_index);
    if (rc) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    rc = ensure_ws(h, N);
    if (rc) return rc;
    rc = order_in(h);
    if (rc) return rc;
    coco_claim_serial_ws(h);
    const PostWorkspace& w = h->ws;
    std::vector<unsigned long long> fl((size_t)N * 4);
    // the copies below read `fl` and the caller's pageable arrays: whatever way the call ends, it ends synchronised (the guard
    // is declared behind the vector, so it runs before the vector is released)
    struct SyncAtExit { hipStream_t s; ~SyncAtExit() { (void)hipStreamSynchronize(s); } } sync_at_exit{h->stream};
    for (int f = 0; f < N; ++f) { fl[f * 4] = 0; fl[f * 4 + 1] = ~0ull; fl[f * 4 + 2] = ~0ull; fl[f * 4 + 3] = 0; }   // as find_peaks leaves them
    HIP_TRY(h, hipMemcpyAsync(w.flags, fl.data(), fl.size() * 8, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipMemcpyAsync(w.n_entries, n_entries, (size_t)N * sizeof(int), hipMemcpyHostToDevice, h->stream));
    const double *e = entries, *k = kpts;
    for (int f = 0; f < N; ++f) {                      // frame f's rows lie back to back in the caller's arrays
        if (n_entries[f]) HIP_TRY(h, hipMemcpyAsync(w.entries + (size_t)f * w.caps.max_entries * w.E, e, (size_t)n_entries[f] * w.E * 8, hipMemcpyHostToDevice, h->stream));
        if (kpt_counts[f]) HIP_TRY(h, hipMemcpyAsync(w.kpts_out + (size_t)f * max_rows * 4, k, (size_t)kpt_counts[f] * 4 * 8, hipMemcpyHostToDevice, h->stream));
        e += (size_t)n_entries[f] * w.E; k += (size_t)kpt_counts[f] * 4;
    }
    rc = coco_enqueue_append(h, N, image_index);
    if (rc) return rc;
    HIP_TRY(h, hipStreamSynchronize(h->stream));       // the caller's arrays and the vector above are free
    return LWP_OK;
}

// argument checks and the partials buffer: everything of lwp_stage_losses before its launches, shared with lwp_time_stage_losses
static int stage_losses_prepare(lwp_handle h, const float* const* outs, int n_outs, const float* keypoint_maps, const float* paf_maps,
                                const float* mask, int N, int hs, int ws, int batch_size) {
    char msg[200];
    if (!outs || !mask) return fail(h, LWP_ERR_ARG, "outs / mask is null");
    if (N < 1 || N > 65535) return fail(h, LWP_ERR_ARG, "N must be 1..65535");
    if (hs < 1 || ws < 1 || (int64_t)hs * ws > (1 << 28)) return fail(h, LWP_ERR_ARG, "empty or oversized map");
    if (batch_size < 1) return fail(h, LWP_ERR_ARG, "batch_size must be at least 1");
    if (!h) return fail(h, LWP_ERR_ARG, "handle is null");
    const int S = 2 * (h->g.nref + 1);
    if (n_outs != S) {
        snprintf(msg, sizeof msg, "n_outs is %d but the network returns %d stage tensors (2 x (num_refinement_stages + 1))", n_outs, S);
        return fail(h, LWP_ERR_ARG, msg);
    }
    if (h->skel.K + 1 != h->g.NH || 2 * h->skel.L != h->g.NP) {
        snprintf(msg, sizeof msg, "the skeleton's targets have %d + 1 heat-map and 2 x %d PAF channels, the network's tensors %d and %d",
                 h->skel.K, h->skel.L, h->g.NH, h->g.NP);
        return fail(h, LWP_ERR_ARG, msg);
    }
    bool any[2] = {false, false};
    for (int s = 0; s < S; ++s) if (outs[s]) any[s & 1] = true;
    if ((any[0] && !keypoint_maps) || (any[1] && !paf_maps)) return fail(h, LWP_ERR_ARG, "keypoint_maps / paf_maps is null but a tensor of its kind is given");
    HIP_TRY(h, hipSetDevice(h->device));
    int rc = order_in(h);
    if (rc) return rc;
    const int blocks = stage_loss_blocks(N, hs * ws);
    const size_t need = ((size_t)kLossMaxOuts * blocks + S) * sizeof(double);
    if (h->d_loss.size() < need) {
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        HIP_TRY(h, h->d_loss.ensure(need));
    }
    return LWP_OK;
}

// the launches of one lwp_stage_losses call; the S sums land behind the partials in d_loss.  With `log` each launch also adds
// its own range of sums / divisor to log[s0 ...], and the first one counts the call in `adds`.
static int enqueue_stage_losses(lwp_handle h, const float* const* outs, const float* keypoint_maps, const float* paf_maps,
                                const float* mask, int N, int hs, int ws, int batch_size, double* log = nullptr, double divisor = 1.0,
                                int64_t* adds = nullptr) {
    const int S = 2 * (h->g.nref + 1);
    const int blocks = stage_loss_blocks(N, hs * ws);
    double* d_partials = h->d_loss.as<double>();
    double* d_losses = d_partials + (size_t)kLossMaxOuts * blocks;
    for (int s0 = 0; s0 < S; s0 += kLossMaxOuts) {       // one launch up to 16 tensors (7 refinement stages); each launch reads the targets once
        StageLossParams p{};
        p.S = std::min(kLossMaxOuts, S - s0);
        for (int s = 0; s < p.S; ++s) p.outs[s] = outs[s0 + s];
        p.keypoint_maps = keypoint_maps; p.paf_maps = paf_maps; p.mask = mask;
        p.N = N; p.CH = h->g.NH; p.CP = h->g.NP; p.hw = hs * ws; p.batch = batch_size;
        p.partials = d_partials;
        LAUNCH(h, KC_OTHER, launch_stage_losses(p, d_losses + s0, h->stream, log ? log + s0 : nullptr, divisor, s0 == 0 ? adds : nullptr));
    }
    return LWP_OK;
}

// the log buffer, zeroed on the handle's stream when it is made: a handle's log is zero until its first add
static int ensure_loss_log(lwp_handle h) {
    if (h->d_loss_log) return LWP_OK;
    const size_t bytes = (size_t)(2 * (h->g.nref + 1)) * sizeof(double) + sizeof(int64_t);
    HIP_TRY(h, h->d_loss_log.ensure(bytes));
    HIP_TRY(h, hipMemsetAsync(h->d_loss_log.as<char>(), 0, bytes, h->stream));
    return LWP_OK;
}

extern "C" int lwp_stage_losses(lwp_handle h, const float* const* outs, int n_outs, const float* keypoint_maps, const float* paf_maps,
                                const float* mask, int N, int hs, int ws, int batch_size, double* losses_host) {
    if (!losses_host) return fail(h, LWP_ERR_ARG, "losses_host is null");
    int rc = stage_losses_prepare(h, outs, n_outs, keypoint_maps, paf_maps, mask, N, hs, ws, batch_size);
    if (rc) return rc;
    rc = enqueue_stage_losses(h, outs, keypoint_maps, paf_maps, mask, N, hs, ws, batch_size);
    if (rc) return rc;
    const int S = 2 * (h->g.nref + 1);
    const double* d_losses = h->d_loss.as<double>() + (size_t)kLossMaxOuts * stage_loss_blocks(N, hs * ws);
    HIP_TRY(h, hipMemcpyAsync(losses_host, d_losses, (size_t)S * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return LWP_OK;
}

extern "C" int lwp_stage_losses_log(lwp_handle h, const float* const* outs, int n_outs, const float* keypoint_maps, const float* paf_maps,
                                    const float* mask, int N, int hs, int ws, int batch_size, double divisor) {
    if (!(divisor > 0.0) || !std::isfinite(divisor)) return fail(h, LWP_ERR_ARG, "divisor must be finite and greater than 0");
    int rc = stage_losses_prepare(h, outs, n_outs, keypoint_maps, paf_maps, mask, N, hs, ws, batch_size);
    if (rc) return rc;
    rc = ensure_loss_log(h);
    if (rc) return rc;
    const int S = 2 * (h->g.nref + 1);
    double* log = h->d_loss_log.as<double>();
    rc = enqueue_stage_losses(h, outs, keypoint_maps, paf_maps, mask, N, hs, ws, batch_size, log, divisor, (int64_t*)(log + S));
    if (rc) return rc;
    bool ordered = false;                              // the caller's next work on the tensors waits for the launches; the host does not
    return order_out(h, h->stream, &ordered);
}

extern "C" int lwp_loss_log_read(lwp_handle h, double* sums_host, int64_t* adds, int reset) {
    if (!h) return fail(h, LWP_ERR_ARG, "handle is null");
    if (!sums_host || !adds) return fail(h, LWP_ERR_ARG, "sums_host / adds is null");
    HIP_TRY(h, hipSetDevice(h->device));
    int rc = ensure_loss_log(h);
    if (rc) return rc;
    const int S = 2 * (h->g.nref + 1);
    const size_t bytes = (size_t)S * sizeof(double) + sizeof(int64_t);
    std::vector<char> host(bytes);
    HIP_TRY(h, hipMemcpyAsync(host.data(), h->d_loss_log.as<char>(), bytes, hipMemcpyDeviceToHost, h->stream));
    if (reset) HIP_TRY(h, hipMemsetAsync(h->d_loss_log.as<char>(), 0, bytes, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    memcpy(sums_host, host.data(), (size_t)S * sizeof(double));
    memcpy(adds, host.data() + (size_t)S * sizeof(double), sizeof(int64_t));
    return LWP_OK;
}

// ---------------------------------------------------------------------------------------------- stage backward
// classes of the backward launches for lwp_profile_stage_backward (they share the forward's event table)
enum BwdClass { BK_ELEMENTWISE = 0, BK_DGRAD = 1, BK_WGRAD = 2, BK_REDUCE = 3, BK_COUNT = 4 };

static int ensure_train_buffers(lwp_context* h, int N, int H, int W) {
    bool synced = false;
    for (size_t i = 0; i < h->tp.bufs.size(); ++i) {
        int fh, fw;
        level_dims(H, W, h->tp.bufs[i].level, &fh, &fw);
        const size_t bytes = (size_t)N * fh * fw * h->tp.bufs[i].channels * sizeof(float);
        const bool with_grad = h->tp.grad_mode[i] == TrainPlan::GRAD_ALWAYS;     // (GRAD_ON_DEMAND: stage_backward_prepare)
        const bool grow = bytes > h->tbufs[i].size() || (with_grad && bytes > h->gbufs[i].size());
        if (grow) {
            if (!synced) { HIP_TRY(h, hipStreamSynchronize(h->stream)); synced = true; }
            HIP_TRY(h, h->tbufs[i].ensure(bytes));
            if (with_grad) HIP_TRY(h, h->gbufs[i].ensure(bytes));
        }
        // pad channels of a concat buffer are read with zero weights: finite at every geometry (as in ensure_activations)
        if (h->tp.bufs[i].has_pad && (grow || N != h->train_N || H != h->train_H || W != h->train_W))
            HIP_TRY(h, hipMemsetAsync(h->tbufs[i].as<void>(), 0, bytes, h->stream));
    }
    if (h->tp.cut < 0) {                               // LWP_TRAIN_ALL: the stem's weight gradient reads the image
        const size_t bytes = (size_t)N * 3 * H * W * sizeof(float);
        if (bytes > h->d_train_in.size()) {
            if (!synced) HIP_TRY(h, hipStreamSynchronize(h->stream));
            HIP_TRY(h, h->d_train_in.ensure(bytes));
        }
    }
    return LWP_OK;
}

static int train_handle_check(lwp_context* h) {
    if (!h) return fail(h, LWP_ERR_ARG, "handle is null");
    if (h->dtype != LWP_F32) return fail(h, LWP_ERR_ARG, "the stage backward runs on fp32 handles only (this one is bf16 / fp16)");
    if (!h->weights_loaded) return fail(h, LWP_ERR_ARG, "weights not loaded (call lwp_load_weights first)");
    if (!h->raw_loaded) return fail(h, LWP_ERR_ARG, "the stage backward needs the raw parameters: load them with lwp_load_weights (a weight blob holds folded weights only)");
    return LWP_OK;
}

extern "C" int lwp_train_forward(lwp_handle h, const float* in_device, int N, int H, int W, float* const* outs_device) {
    int rc = train_handle_check(h);
    if (rc) return rc;
    if (!in_device || !outs_device) return fail(h, LWP_ERR_ARG, "null argument");
    rc = check_frame_shape(h, N, H, W);
    if (rc) return rc;
    const int nout = 2 * (1 + h->g.nref);
    for (int i = 0; i < nout; ++i) if (!outs_device[i]) return fail(h, LWP_ERR_ARG, "null output pointer");
    HIP_TRY(h, hipSetDevice(h->device));
    if (frames_per_pass(h, N, H, W) != N) return fail(h, LWP_ERR_ARG, "batch too large for one retaining pass (a tensor would reach 2 GiB)");
    rc = ensure_activations(h, N, H, W);
    if (rc) return rc;
    rc = ensure_train_buffers(h, N, H, W);
    if (rc) return rc;
    h->train_N = 0;
    rc = order_in(h);
    if (rc) return rc;
    // the layers in front of the plan's cut (cpm.conv, or the backbone's last layer in scope LWP_TRAIN_CPM; none in scope
    // LWP_TRAIN_ALL): the graph's own plan, nothing retained; then the retaining plan, with the outputs of the kernels Engine.forward uses
    const TrainPlan& tp = h->tp;
    if (tp.cut < 0) HIP_TRY(h, hipMemcpyAsync(h->d_train_in.as<void>(), in_device, (size_t)N * 3 * H * W * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
    rc = enqueue_forward(h, h->g.layers, 0, tp.cut, in_device, N, H, W, nullptr);
    if (!rc) rc = enqueue_forward(h, tp.layers, std::max(tp.cut, 0), tp.cpm_conv + 1, in_device, N, H, W, outs_device, true);
    if (rc) return rc;
    int fh, fw;
    level_dims(H, W, 3, &fh, &fw);
    const int C = h->g.C, catc = h->g.cat_channels, nb = (int)h->g.bufs.size();
    for (int k = 1; k < h->g.nref; ++k)        // every refinement stage reads [features | heat | paf] of a buffer of its own
        LAUNCH(h, KC_OTHER, launch_grad_add(h->tbufs[tp.cats[k] - nb].as<float>(), catc, h->tbufs[tp.cats[0] - nb].as<float>(), catc, (int64_t)N * fh * fw, C, 0, h->stream));
    rc = enqueue_forward(h, tp.layers, tp.cpm_conv + 1, (int)tp.layers.size(), in_device, N, H, W, outs_device, true);
    if (rc) return rc;
    h->train_N = N; h->train_H = H; h->train_W = W;
    bool ordered = false;
    return order_out(h, h->stream, &ordered);
}

static float* grad_at(lwp_context* h, const BufRef& r) { return h->gbufs[r.buf - (int)h->g.bufs.size()].as<float>() + r.coff; }

struct BackwardArgs {
    const float* keypoint_maps; const float* paf_maps; const float* mask;
    int N, hs, ws, batch_size, accumulate;
    double loss_scale;
    float* grads; float* d_features;
    float* d_backbone = nullptr;       // LWP_TRAIN_CPM: the gradient at the cpm's input, N x 512 x hs x ws, or null
};

// What the backward of one layer of the retaining plan launches with, on its output map of M = N x h x w pixels: the pixel ranges
// of every weight-gradient launch and the floats of the workspace d_bwd they need.  stage_backward_prepare sizes d_bwd from the
// maxima over the layers and the walk launches from the same values, so the sizes and the launches cannot drift apart.
struct PixelRanges { int splits = 0, chunk = 0; };
struct LayerBackwardPlan {
    std::vector<PixelRanges> w;        // dense weight gradients: the layer's own (the pointwise half's of an L_DWPW block), or one per
                                       // source conv of a merged head layer; L_STEM: the stem kernel's
    PixelRanges dw;                    // L_DW, L_DWPW: the depthwise weight gradient
    size_t part = 0;                   // partials of the largest of these launches
    size_t fold = 0;                   // folded G | g in front of the largest BatchNorm chain rule
    size_t pwf = 0;                    // the folded pointwise matrix of a fused block with BatchNorm
};
static LayerBackwardPlan backward_plan(const Layer& l, int64_t M) {
    LayerBackwardPlan bp;
    if (l.kind == L_STEM) {                                       // (LWP_TRAIN_ALL) [28][32] partials per range, G (32, 27) | g (32)
        PixelRanges r;
        stem_wgrad_plan(M, &r.splits, &r.chunk);
        bp.w.push_back(r);
        bp.part = (size_t)r.splits * 28 * 32;
        bp.fold = (size_t)32 * 27 + 32;
        return bp;
    }
    if (l.kind == L_DW || l.kind == L_DWPW) {
        const bool bn = !l.bn_key.empty();                        // with BatchNorm: the sum of dZ as a tenth row
        dw_wgrad_plan(M, l.cin, &bp.dw.splits, &bp.dw.chunk);
        bp.part = (size_t)bp.dw.splits * (bn ? 10 : 9) * l.cin;
        if (bn) bp.fold = (size_t)10 * l.cin;
        if (l.kind == L_DW) return bp;
        if (!l.bn2_key.empty()) {
            bp.fold = std::max(bp.fold, (size_t)l.cout * l.cin + l.cout);
            bp.pwf = (size_t)l.cout * l.cin;
        }
    }
    const int ks = l.kind == L_DWPW ? 1 : l.ks;                   // the pointwise half of a fused block
    auto one = [&](int cout, int cin) {
        WgradParams w{};
        w.cout = cout; w.cin = cin; w.ks = ks;
        wgrad_plan(M, cout, cin, ks, &w.splits, &w.chunk);
        bp.w.push_back({w.splits, w.chunk});
        bp.part = std::max(bp.part, wgrad_partial_floats(w));
    };
    if (l.blocks.empty()) one(l.cout, l.cin);
    else for (const WBlock& b : l.blocks) one(b.cout, b.cin);
    if (l.kind == L_GEMM && !l.bn_key.empty()) bp.fold = std::max(bp.fold, (size_t)l.cout * l.cin * l.ks * l.ks + l.cout);
    return bp;
}

static int stage_backward_prepare(lwp_handle h, const BackwardArgs& a) {
    char msg[200];
    int rc = train_handle_check(h);
    if (rc) return rc;
    if (!a.keypoint_maps || !a.paf_maps || !a.mask || !a.grads) return fail(h, LWP_ERR_ARG, "keypoint_maps / paf_maps / mask / grads_device is null");
    if (a.batch_size < 1) return fail(h, LWP_ERR_ARG, "batch_size must be at least 1");
    if (a.d_backbone && h->scope == LWP_TRAIN_STAGES)
        return fail(h, LWP_ERR_ARG, "d_backbone_device needs the train scope LWP_TRAIN_CPM or LWP_TRAIN_ALL (lwp_set_train_scope): in scope LWP_TRAIN_STAGES the cpm has no backward");
    if (!std::isfinite(a.loss_scale)) return fail(h, LWP_ERR_ARG, "loss_scale must be finite");
    if (h->skel.K + 1 != h->g.NH || 2 * h->skel.L != h->g.NP) {
        snprintf(msg, sizeof msg, "the skeleton's targets have %d + 1 heat-map and 2 x %d PAF channels, the network's tensors %d and %d",
                 h->skel.K, h->skel.L, h->g.NH, h->g.NP);
        return fail(h, LWP_ERR_ARG, msg);
    }
    int fh = 0, fw = 0;
    if (h->train_N > 0) level_dims(h->train_H, h->train_W, 3, &fh, &fw);
    if (h->train_N < 1 || h->train_N != a.N || fh != a.hs || fw != a.ws) {
        snprintf(msg, sizeof msg, "no retaining forward of %d x %d x %d maps precedes this call (lwp_train_forward; the last one kept %d x %d x %d)",
                 a.N, a.hs, a.ws, h->train_N, fh, fw);
        return fail(h, LWP_ERR_ARG, msg);
    }
    HIP_TRY(h, hipSetDevice(h->device));
    // workspace: the largest partials of a layer + the folded gradients of the largest BatchNorm layer + the largest folded pointwise matrix
    size_t part = 0, fold = 0, pwf = 0;
    for (size_t i = (size_t)(h->tp.cut + 1); i < h->tp.layers.size(); ++i) {
        const Layer& l = h->tp.layers[i];
        int lh, lw;                                               // the layer's output map (a backbone layer's may be above level 3)
        level_dims(h->train_H, h->train_W, buf_level(h, l.dst.buf), &lh, &lw);
        const LayerBackwardPlan bp = backward_plan(l, (int64_t)a.N * lh * lw);
        part = std::max(part, bp.part);
        fold = std::max(fold, bp.fold);
        pwf = std::max(pwf, bp.pwf);
    }
    part = (part + 63) / 64 * 64;
    fold = (fold + 63) / 64 * 64;
    h->bwd_fold_off = part;
    h->bwd_pw_off = part + fold;
    const size_t need = (part + fold + pwf) * sizeof(float);
    if (h->d_bwd.size() < need) {
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        HIP_TRY(h, h->d_bwd.ensure(need));
    }
    if (a.d_backbone && h->tp.cut == h->tp.cpm_in) {   // LWP_TRAIN_CPM: the 512-channel gradient at the cpm's input exists only once it is asked for
        const int xb = h->tp.layers[h->tp.cut].dst.buf - (int)h->g.bufs.size();
        if (h->gbufs[xb].size() < h->tbufs[xb].size()) {
            HIP_TRY(h, hipStreamSynchronize(h->stream));
            HIP_TRY(h, h->gbufs[xb].ensure(h->tbufs[xb].size()));
        }
    }
    return order_in(h);
}

// the gradient buffers of one backward walk: a buffer's first writer overwrites, later ones add (the launch order is the summation order)
struct GradBuffers {
    std::vector<char> written;
    int nb;
    int adds(const BufRef& r) {                        // for the launch that writes r next: 1 = add to what is there
        char& w = written[r.buf - nb];
        const int had = w;
        w = 1;
        return had;
    }
};

// g = g * act'(z) from the retained output y: ELU from y itself, ReLU as the mask y > res (res null: y > 0)
static int enqueue_act_grad(lwp_context* h, int act, float* g, int g_ld, const float* y, int y_ld, const float* res, int res_ld, int64_t M, int C) {
    if (act == ACT_ELU) LAUNCH(h, BK_ELEMENTWISE, launch_elu_grad(g, g_ld, y, y_ld, M, C, h->stream));
    if (act == ACT_RELU) LAUNCH(h, BK_ELEMENTWISE, launch_relu_mask(g, g_ld, y, y_ld, res, res_ld, M, C, h->stream));
    return LWP_OK;
}

// BatchNorm chain rule behind a conv: folded G, g in the workspace -> dW, db (with a conv bias), dgamma, dbeta in the gradient array
static int enqueue_bn_chain(lwp_context* h, const std::string& conv_key, const std::string& bn_key, bool has_bias, const float* G, const float* g,
                            int cout, int K, const BackwardArgs& a) {
    BnChainParams b{};
    b.G = G; b.g = g;
    b.W = h->raw(conv_key + ".weight"); b.b = has_bias ? h->raw(conv_key + ".bias") : h->d_zeros.as<float>();   // (1024 zeros: the backbone's cout is at most 512)
    b.gamma = h->raw(bn_key + ".weight");
    b.mean = h->raw(bn_key + ".running_mean"); b.var = h->raw(bn_key + ".running_var");
    b.dW = a.grads + h->grad_off.at(conv_key + ".weight"); b.db = has_bias ? a.grads + h->grad_off.at(conv_key + ".bias") : nullptr;
    b.dgamma = a.grads + h->grad_off.at(bn_key + ".weight"); b.dbeta = a.grads + h->grad_off.at(bn_key + ".bias");
    b.cout = cout; b.K = K; b.accumulate = a.accumulate;
    LAUNCH(h, BK_REDUCE, launch_bn_chain(b, h->stream));
    return LWP_OK;
}

static DgradParams dgrad_params(const float* dz, int dz_ld, const float* w, int cout_pad, int cin_pad, float* dx, int dx_ld, int acc_from,
                                int N, int H, int W, int cout, int cin, int ks, int dil) {
    DgradParams d{};
    d.dz = dz; d.dz_ld = dz_ld; d.w = w; d.dx = dx; d.dx_ld = dx_ld;
    d.N = N; d.H = H; d.W = W; d.cout = cout; d.cout_pad = cout_pad; d.cin = cin; d.cin_pad = cin_pad; d.ks = ks; d.dil = dil; d.acc_from = acc_from;
    return d;
}

// wgrad of one conv (a whole layer, or one source conv of a merged head layer) over the plan's pixel ranges: partials, fixed-order
// reduction, and the BatchNorm chain rule where the layer has one
// (pointwise: the 1x1 half of an L_DWPW block, conv_key its conv2_key; a conv without bias has no bias row and no db)
static int enqueue_wgrad(lwp_context* h, const Layer& l, const float* dz, int dz_ld, const float* x, int x_ld, int cout, int cin,
                         const std::string& conv_key, const BackwardArgs& a, PixelRanges r, bool pointwise = false) {
    const bool has_bias = !pointwise && l.has_bias;
    const std::string& bn_key = pointwise ? l.bn2_key : l.bn_key;
    WgradParams w{};
    w.dz = dz; w.dz_ld = dz_ld; w.x = x; w.x_ld = x_ld; w.partial = h->d_bwd.as<float>();
    w.N = a.N; w.H = a.hs; w.W = a.ws; w.cout = cout; w.cin = cin; w.ks = pointwise ? 1 : l.ks; w.dil = pointwise ? 1 : l.dil;
    w.no_bias = (has_bias || !bn_key.empty()) ? 0 : 1;     // the BatchNorm chain rule needs the column sums of dZ, conv bias or not
    w.splits = r.splits; w.chunk = r.chunk;
    LAUNCH(h, BK_WGRAD, launch_wgrad(w, h->stream, h->bwd_prec));
    if (bn_key.empty()) {
        float* db = has_bias ? a.grads + h->grad_off.at(conv_key + ".bias") : nullptr;
        LAUNCH(h, BK_REDUCE, launch_wgrad_reduce(w, a.grads + h->grad_off.at(conv_key + ".weight"), db, a.accumulate, h->stream));
        return LWP_OK;
    }
    float* G = h->d_bwd.as<float>() + h->bwd_fold_off;
    float* g = G + (size_t)cout * cin * w.ks * w.ks;
    LAUNCH(h, BK_REDUCE, launch_wgrad_reduce(w, G, g, 0, h->stream));
    return enqueue_bn_chain(h, conv_key, bn_key, has_bias, G, g, cout, cin * w.ks * w.ks, a);
}

// the stem (LWP_TRAIN_ALL): its weight gradient only, there is no gradient at the image.  dz: the gradient at its pre-activation output
static int enqueue_stem_wgrad(lwp_context* h, const Layer& l, const float* dz, const BackwardArgs& a, PixelRanges r) {
    StemWgradParams p{};
    p.dz = dz; p.dz_ld = l.dst.ld; p.x = h->d_train_in.as<float>(); p.partial = h->d_bwd.as<float>();
    p.N = a.N; p.H = h->train_H; p.W = h->train_W; p.Ho = a.hs; p.Wo = a.ws;
    p.splits = r.splits; p.chunk = r.chunk;
    float* G = h->d_bwd.as<float>() + h->bwd_fold_off;
    float* g = G + 32 * 27;
    LAUNCH(h, BK_WGRAD, launch_stem_wgrad(p, h->stream));
    LAUNCH(h, BK_REDUCE, launch_stem_wgrad_reduce(p, G, g, h->stream));
    return enqueue_bn_chain(h, l.conv_key, l.bn_key, false, G, g, 32, 27, a);
}

// depthwise 3x3 (an L_DW layer, or the first half of an L_DWPW block): dz is the gradient at its activation output y, on the
// layer's a.hs x a.ws output map.  The cpm's has an ELU behind it and no BatchNorm: its weight gradient goes straight to the
// gradient array.  The backbone's (stride 1 | 2, dilation 1 | 2) has BatchNorm + ReLU: folded G | g, then the chain rule.
static int enqueue_dw_backward(lwp_context* h, const Layer& l, float* dz, int dz_ld, const float* y, int y_ld, const BackwardArgs& a,
                               PixelRanges r, GradBuffers& gb) {
    int rc = enqueue_act_grad(h, l.act, dz, dz_ld, y, y_ld, nullptr, 0, (int64_t)a.N * a.hs * a.ws, l.cin);
    if (rc) return rc;
    DwGradParams p{};
    p.dz = dz; p.dz_ld = dz_ld; p.x = buf_at(h, l.src); p.x_ld = l.src.ld; p.w = h->blob(l.w_off);
    p.dx = grad_at(h, l.src); p.dx_ld = l.src.ld; p.partial = h->d_bwd.as<float>();
    level_dims(h->train_H, h->train_W, buf_level(h, l.src.buf), &p.H, &p.W);
    p.N = a.N; p.Ho = a.hs; p.Wo = a.ws; p.C = l.cin; p.stride = l.stride; p.dil = l.dil; p.beta = gb.adds(l.src);
    p.splits = r.splits; p.chunk = r.chunk;
    const bool bn = !l.bn_key.empty();
    LAUNCH(h, BK_WGRAD, launch_dw_wgrad(p, bn, h->stream));
    if (bn) {
        float* G = h->d_bwd.as<float>() + h->bwd_fold_off;
        float* g = G + (size_t)9 * l.cin;
        LAUNCH(h, BK_REDUCE, launch_dw_wgrad_reduce(p, G, g, 0, h->stream));
        rc = enqueue_bn_chain(h, l.conv_key, l.bn_key, false, G, g, l.cin, 9, a);
        if (rc) return rc;
    } else
        LAUNCH(h, BK_REDUCE, launch_dw_wgrad_reduce(p, a.grads + h->grad_off.at(l.conv_key + ".weight"), nullptr, a.accumulate, h->stream));
    LAUNCH(h, BK_DGRAD, launch_dw_dgrad(p, h->stream));
    return LWP_OK;
}

// a fused block, dy the gradient at its pre-activation output: the pointwise half on the retained copy of the depthwise half's
// output, then the depthwise half.  The blob holds the pointwise weights in fragment order only, so the 1x1 dgrad reads the raw
// (cout, cin) matrix: without BatchNorm (the cpm) the raw values are the folded ones, with it (the backbone) the folded matrix
// is made from the raw parameters for this launch.
static int enqueue_dwpw_backward(lwp_context* h, const Layer& l, int i, const float* dy, const BackwardArgs& a, const LayerBackwardPlan& bp,
                                 GradBuffers& gb) {
    const float* dcopy = h->tbufs[h->tp.dw_copy[i] - gb.nb].as<float>();
    float* gd = h->gbufs[h->tp.dw_copy[i] - gb.nb].as<float>();
    const int rc = enqueue_wgrad(h, l, dy, l.dst.ld, dcopy, l.cin, l.cout, l.cin, l.conv2_key, a, bp.w[0], true);
    if (rc) return rc;
    const float* w = h->raw(l.conv2_key + ".weight");
    if (!l.bn2_key.empty()) {
        float* wf = h->d_bwd.as<float>() + h->bwd_pw_off;
        LAUNCH(h, BK_ELEMENTWISE, launch_pw_fold(w, h->raw(l.bn2_key + ".weight"), h->raw(l.bn2_key + ".running_var"), wf, l.cout, l.cin, h->stream));
        w = wf;
    }
    const DgradParams d = dgrad_params(dy, l.dst.ld, w, l.cout, l.cin, gd, l.cin, l.cin, a.N, a.hs, a.ws, l.cout, l.cin, 1, 1);
    LAUNCH(h, BK_DGRAD, launch_dgrad(d, h->stream, h->bwd_prec));
    return enqueue_dw_backward(h, l, gd, l.cin, dcopy, l.cin, a, bp.dw, gb);
}

// one layer of the walk.  a: the call's arguments, its hs x ws the level-3 map of the stages and the cpm
static int enqueue_layer_backward(lwp_context* h, int i, const BackwardArgs& a, GradBuffers& gb) {
    const TrainPlan& tp = h->tp;
    const Graph& g = h->g;
    const Layer& l = tp.layers[i];
    const int nb = gb.nb, C = g.C, catc = g.cat_channels;
    BackwardArgs al = a;                               // the layer's own output map (a backbone layer's may be above level 3)
    level_dims(h->train_H, h->train_W, buf_level(h, l.dst.buf), &al.hs, &al.ws);
    const int64_t M = (int64_t)al.N * al.hs * al.ws;
    const LayerBackwardPlan bp = backward_plan(l, M);
    h->bwd_splits[i] = bp.w.empty() ? bp.dw.splits : bp.w.back().splits;
    h->bwd_dw_splits[i] = bp.dw.splits;
    float* dy = grad_at(h, l.dst);
    const float* y = buf_at(h, l.dst);
    if (i == tp.cpm_in && a.d_backbone)                // LWP_TRAIN_ALL: the backbone's last layer (in LWP_TRAIN_CPM the walk ends above it: step 3)
        LAUNCH(h, BK_ELEMENTWISE, launch_nchw_from_nhwc(dy, l.dst.ld, a.d_backbone, a.N, a.hs * a.ws, l.cout, h->stream));
    if (i == tp.cpm_conv && tp.cut != tp.cpm_conv) {
        // LWP_TRAIN_CPM: cpm.conv's output feeds the initial stage and every refinement stage; its gradient is their sum in
        // stage order (step 3 below does the same for d_features, on the same values in the same order)
        for (int k = 1; k < g.nref; ++k)
            LAUNCH(h, BK_ELEMENTWISE, launch_grad_add(dy, catc, h->gbufs[tp.cats[k] - nb].as<float>(), catc, M, C, 1, h->stream));
        if (a.d_features) LAUNCH(h, BK_ELEMENTWISE, launch_nchw_from_nhwc(dy, catc, a.d_features, a.N, a.hs * a.ws, C, h->stream));
    }
    if (l.res.buf >= 0)                                // out = act(z) + res: the residual branch takes the gradient as it is
        LAUNCH(h, BK_ELEMENTWISE, launch_grad_add(grad_at(h, l.res), l.res.ld, dy, l.dst.ld, M, l.cout, gb.adds(l.res), h->stream));
    if (l.kind == L_DW) return enqueue_dw_backward(h, l, dy, l.dst.ld, y, l.dst.ld, al, bp.dw, gb);
    // the activation behind the layer's last conv; the ELU output in front of a residual add is the retained copy of the launch without it
    const int act = l.kind == L_DWPW ? l.act2 : l.act;
    const float* y_act = act == ACT_ELU && tp.nores_copy[i] >= 0 ? h->tbufs[tp.nores_copy[i] - nb].as<float>() : y;
    int rc = enqueue_act_grad(h, act, dy, l.dst.ld, y_act, l.dst.ld, l.res.buf >= 0 ? buf_at(h, l.res) : nullptr, l.res.ld, M, l.cout);
    if (rc) return rc;
    if (l.kind == L_STEM) return enqueue_stem_wgrad(h, l, dy, al, bp.w[0]);
    if (l.kind == L_DWPW) return enqueue_dwpw_backward(h, l, i, dy, al, bp, gb);
    const float* x = buf_at(h, l.src);
    if (l.blocks.empty()) rc = enqueue_wgrad(h, l, dy, l.dst.ld, x, l.src.ld, l.cout, l.cin, l.conv_key, al, bp.w[0]);
    else
        for (size_t k = 0; k < l.blocks.size() && !rc; ++k) {
            const WBlock& b = l.blocks[k];
            rc = enqueue_wgrad(h, l, dy + b.out_off, l.dst.ld, x + b.in_off, l.src.ld, b.cout, b.cin, b.conv_key, al, bp.w[k]);
        }
    if (rc) return rc;
    if (i == tp.cut + 1 && h->scope == LWP_TRAIN_CPM && !a.d_backbone) return LWP_OK;      // cpm.align's dgrad is 512 wide: only when asked for
    // a concat buffer's heat / PAF channels already hold the stage's loss gradient; its feature channels are summed over the stages
    const bool is_cat = std::find(tp.cats.begin(), tp.cats.end(), l.src.buf) != tp.cats.end();
    const int acc_from = gb.adds(l.src) ? 0 : (is_cat ? C : l.cin);
    const DgradParams d = dgrad_params(dy, l.dst.ld, h->blob(l.w_off), l.cout_pad, l.cin_pad, grad_at(h, l.src), l.src.ld, acc_from, al.N, al.hs, al.ws,
                                       l.cout, l.cin, l.ks, l.dil);
    LAUNCH(h, BK_DGRAD, launch_dgrad(d, h->stream, h->bwd_prec));
    return LWP_OK;
}

static int enqueue_stage_backward(lwp_context* h, const BackwardArgs& a) {
    const TrainPlan& tp = h->tp;
    const Graph& g = h->g;
    const int nb = (int)g.bufs.size();
    const int C = g.C, NH = g.NH, NP = g.NP, catc = g.cat_channels;
    const int64_t M = (int64_t)a.N * a.hs * a.ws;
    const int S = 2 * (g.nref + 1);
    // 1. dL/d out of every stage, one launch per 16 tensors: from the [heat | paf] window of the stage's concat buffer (the very
    //    values of the NCHW stage tensors) into the same window of its gradient buffer
    for (int s0 = 0; s0 < S; s0 += kLossMaxOuts) {
        LossGradParams p{};
        p.S = std::min(kLossMaxOuts, S - s0);
        for (int s = 0; s < p.S; ++s) {
            const int st = (s0 + s) / 2;
            const int coff = C + (((s0 + s) & 1) ? NH : 0);
            p.outs[s] = h->tbufs[tp.cats[st] - nb].as<float>() + coff;
            p.dst[s] = h->gbufs[tp.cats[st] - nb].as<float>() + coff;
        }
        p.ld = catc;
        p.keypoint_maps = a.keypoint_maps; p.paf_maps = a.paf_maps; p.mask = a.mask;
        p.N = a.N; p.CH = NH; p.CP = NP; p.hw = a.hs * a.ws;
        p.scale = (float)(a.loss_scale / (double)a.batch_size);
        LAUNCH(h, BK_ELEMENTWISE, launch_loss_grad(p, h->stream));
    }
    // 2. the layers in reverse
    GradBuffers gb{std::vector<char>(tp.bufs.size(), 0), nb};
    for (int i = (int)tp.layers.size() - 1; i > tp.cut; --i) {
        h->cur_layer = i;
        const int rc = enqueue_layer_backward(h, i, a, gb);
        h->cur_layer = -1;
        if (rc) return rc;
    }
    // 3. backbone_features feeds the initial stage and every refinement stage: stage order, then NCHW
    if (a.d_backbone && tp.cut == tp.cpm_in) {
        const BufRef& xin = tp.layers[tp.cut].dst;
        LAUNCH(h, BK_ELEMENTWISE, launch_nchw_from_nhwc(grad_at(h, xin), xin.ld, a.d_backbone, a.N, a.hs * a.ws, tp.layers[tp.cut].cout, h->stream));
    }
    if (a.d_features && tp.cut == tp.cpm_conv) {
        float* g0 = h->gbufs[tp.cats[0] - nb].as<float>();
        for (int k = 1; k < g.nref; ++k)
            LAUNCH(h, BK_ELEMENTWISE, launch_grad_add(g0, catc, h->gbufs[tp.cats[k] - nb].as<float>(), catc, M, C, 1, h->stream));
        LAUNCH(h, BK_ELEMENTWISE, launch_nchw_from_nhwc(g0, catc, a.d_features, a.N, a.hs * a.ws, C, h->stream));
    }
    return LWP_OK;
}

extern "C" int lwp_stage_backward(lwp_handle h, const float* keypoint_maps, const float* paf_maps, const float* mask, int N, int hs, int ws,
                                  int batch_size, double loss_scale, int accumulate, float* grads_device, float* d_features_device) {
    return lwp_train_backward(h, keypoint_maps, paf_maps, mask, N, hs, ws, batch_size, loss_scale, accumulate, grads_device, d_features_device, nullptr);
}

extern "C" int lwp_train_backward(lwp_handle h, const float* keypoint_maps, const float* paf_maps, const float* mask, int N, int hs, int ws,
                                  int batch_size, double loss_scale, int accumulate, float* grads_device, float* d_features_device,
                                  float* d_backbone_device) {
    const BackwardArgs a{keypoint_maps, paf_maps, mask, N, hs, ws, batch_size, accumulate, loss_scale, grads_device, d_features_device, d_backbone_device};
    int rc = stage_backward_prepare(h, a);
    if (rc) return rc;
    rc = enqueue_stage_backward(h, a);
    if (rc) return rc;
    bool ordered = false;
    return order_out(h, h->stream, &ordered);
}

extern "C" int lwp_set_train_scope(lwp_handle h, int scope) {
    if (!h) return fail(h, LWP_ERR_ARG, "handle is null");
    if (h->dtype != LWP_F32) return fail(h, LWP_ERR_ARG, "the train scope belongs to fp32 handles only (this one is bf16 / fp16)");
    if (scope != LWP_TRAIN_STAGES && scope != LWP_TRAIN_CPM && scope != LWP_TRAIN_ALL)
        return fail(h, LWP_ERR_ARG, "unknown train scope (LWP_TRAIN_STAGES, LWP_TRAIN_CPM or LWP_TRAIN_ALL)");
    for (auto& sl : h->slots) if (sl.pending) return fail(h, LWP_ERR_STATE, "pipeline slot pending: fetch it before changing the train scope");
    if (h->async_pending) return fail(h, LWP_ERR_STATE, "an lwp_infer_poses_async is pending: fetch it before changing the train scope");
    if (h->adam_t > 0)
        return fail(h, LWP_ERR_STATE, "the optimiser has taken steps: the moments are laid out for the current scope (lwp_stage_adam_reset first, or set the scope before the first step)");
    if (scope == h->scope) { h->train_N = 0; return LWP_OK; }
    HIP_TRY(h, hipSetDevice(h->device));
    int rc = order_in(h);
    if (rc) return rc;
    HIP_TRY(h, hipStreamSynchronize(h->stream));       // the plan's buffers and the optimiser tables are released below
    apply_train_scope(h, scope);
    return LWP_OK;
}

extern "C" int lwp_set_backward_precision(lwp_handle h, int dtype, double grad_scale) {
    if (!h) return fail(h, LWP_ERR_ARG, "handle is null");
    if (h->dtype != LWP_F32) return fail(h, LWP_ERR_ARG, "the backward precision belongs to fp32 handles only (this one is bf16 / fp16)");
    if (dtype != LWP_F32 && dtype != LWP_BF16 && dtype != LWP_F16) return fail(h, LWP_ERR_ARG, "unknown backward precision (LWP_F32, LWP_BF16 or LWP_F16)");
    int e = 0;
    if (!(grad_scale >= 1.0 && grad_scale <= 16777216.0) || std::frexp(grad_scale, &e) != 0.5)
        return fail(h, LWP_ERR_ARG, "grad_scale must be a power of two in [1, 2^24]");
    if (dtype == LWP_F32 && grad_scale != 1.0) return fail(h, LWP_ERR_ARG, "grad_scale must be 1 with LWP_F32 (the fp32 kernels do not scale)");
    h->bwd_prec.dtype = dtype;
    h->bwd_prec.scale = (float)grad_scale;
    return LWP_OK;
}

extern "C" int lwp_get_backward_precision(lwp_handle h, int* dtype, double* grad_scale) {
    if (!h || !dtype || !grad_scale) return fail(h, LWP_ERR_ARG, "null argument");
    *dtype = h->bwd_prec.dtype;
    *grad_scale = (double)h->bwd_prec.scale;
    return LWP_OK;
}

extern "C" int lwp_profile_stage_backward(lwp_handle h, const float* keypoint_maps, const float* paf_maps, const float* mask, int N, int hs,
                                          int ws, int batch_size, double loss_scale, float* grads_device, float* d_features_device,
                                          int reps, float* ms, int* launches) {
    if (!ms || !launches || reps <= 0) return fail(h, LWP_ERR_ARG, "bad argument");
    const BackwardArgs a{keypoint_maps, paf_maps, mask, N, hs, ws, batch_size, 0, loss_scale, grads_device, d_features_device};
    int rc = stage_backward_prepare(h, a);
    if (rc) return rc;
    return profile_by_class(h, BK_COUNT, reps, ms, launches, [&]() { return enqueue_stage_backward(h, a); });
}

extern "C" int lwp_stage_grad_count(int nref, int C, int NH, int NP, int64_t* total_floats) {
    if (nref < 0 || C <= 0 || NH <= 0 || NP <= 0) return LWP_ERR_ARG;
    size_t total = 0;
    const int n = (int)stage_grad_spec(nref, C, NH, NP, &total).size();
    if (total_floats) *total_floats = (int64_t)total;
    return n;
}

extern "C" int lwp_stage_grad_spec(int nref, int C, int NH, int NP, int index, char* name, int name_cap, int64_t shape[4], int* ndim,
                                   int64_t* offset) {
    if (nref < 0 || C <= 0 || NH <= 0 || NP <= 0 || !name || !shape || !ndim || !offset) return fail(nullptr, LWP_ERR_ARG, "bad argument");
    const auto t = stage_grad_spec(nref, C, NH, NP, nullptr);
    if (index < 0 || index >= (int)t.size()) return fail(nullptr, LWP_ERR_ARG, "index out of range");
    if ((int)t[index].key.size() + 1 > name_cap) return fail(nullptr, LWP_ERR_ARG, "name buffer too small");
    std::strcpy(name, t[index].key.c_str());
    for (int d = 0; d < 4; ++d) shape[d] = t[index].shape[d];
    *ndim = t[index].ndim;
    *offset = (int64_t)t[index].off;
    return LWP_OK;
}

static bool train_shape_ok(int scope, int nref, int C, int NH, int NP) {
    return (scope == LWP_TRAIN_STAGES || scope == LWP_TRAIN_CPM || scope == LWP_TRAIN_ALL) && nref >= 0 && C > 0 && NH > 0 && NP > 0;
}
extern "C" int lwp_train_grad_count(int scope, int nref, int C, int NH, int NP, int64_t* total_floats) {
    if (!train_shape_ok(scope, nref, C, NH, NP)) return LWP_ERR_ARG;
    size_t total = 0;
    const int n = (int)train_grad_spec(scope, nref, C, NH, NP, &total).size();
    if (total_floats) *total_floats = (int64_t)total;
    return n;
}

extern "C" int lwp_train_grad_spec(int scope, int nref, int C, int NH, int NP, int index, char* name, int name_cap, int64_t shape[4], int* ndim,
                                   int64_t* offset) {
    if (!train_shape_ok(scope, nref, C, NH, NP) || !name || !shape || !ndim || !offset) return fail(nullptr, LWP_ERR_ARG, "bad argument");
    const auto t = train_grad_spec(scope, nref, C, NH, NP, nullptr);
    if (index < 0 || index >= (int)t.size()) return fail(nullptr, LWP_ERR_ARG, "index out of range");
    if ((int)t[index].key.size() + 1 > name_cap) return fail(nullptr, LWP_ERR_ARG, "name buffer too small");
    std::strcpy(name, t[index].key.c_str());
    for (int d = 0; d < 4; ++d) shape[d] = t[index].shape[d];
    *ndim = t[index].ndim;
    *offset = (int64_t)t[index].off;
    return LWP_OK;
}

extern "C" int lwp_debug_train_activation(lwp_handle h, int idx, float* dst, size_t dst_floats, int out_dims[4]) {
    return lwp_debug_train_copy(h, idx, LWP_KEPT_OUTPUT, dst, dst_floats, out_dims);
}

extern "C" int lwp_debug_train_copy(lwp_handle h, int idx, int which, float* dst, size_t dst_floats, int out_dims[4]) {
    int rc = train_handle_check(h);
    if (rc) return rc;
    if (!dst || !out_dims) return fail(h, LWP_ERR_ARG, "bad argument");
    if (idx < 0 || idx < h->tp.cut || idx >= (int)h->tp.layers.size()) return fail(h, LWP_ERR_ARG, "layer_index is not a layer of the retaining plan");
    if (which != LWP_KEPT_OUTPUT && which != LWP_KEPT_DEPTHWISE && which != LWP_KEPT_NO_RESIDUAL) return fail(h, LWP_ERR_ARG, "unknown kind of retained tensor");
    if ((which == LWP_KEPT_DEPTHWISE && h->tp.dw_copy[idx] < 0) || (which == LWP_KEPT_NO_RESIDUAL && h->tp.nores_copy[idx] < 0))
        return fail(h, LWP_ERR_ARG, "the layer has no such retained copy");
    if (h->train_N < 1) return fail(h, LWP_ERR_ARG, "no retaining forward precedes this call (lwp_train_forward)");
    HIP_TRY(h, hipSetDevice(h->device));
    Layer l = h->tp.layers[idx];
    if (which == LWP_KEPT_DEPTHWISE) { l.dst = BufRef(); l.dst.buf = h->tp.dw_copy[idx]; l.dst.ld = l.cin; l.cout = l.cin; }
    if (which == LWP_KEPT_NO_RESIDUAL) { l.dst.buf = h->tp.nores_copy[idx]; l.dst.coff = 0; }
    int dh, dw;
    level_dims(h->train_H, h->train_W, buf_level(h, l.dst.buf), &dh, &dw);
    const size_t n = (size_t)h->train_N * l.cout * dh * dw;
    if (dst_floats < n) return fail(h, LWP_ERR_ARG, "dst too small");
    HIP_TRY(h, h->d_tmp.ensure(n * sizeof(float)));
    HIP_TRY(h, launch_nchw_from_nhwc(buf_at(h, l.dst), l.dst.ld, h->d_tmp.as<float>(), h->train_N, dh * dw, l.cout, h->stream));
    HIP_TRY(h, hipMemcpyAsync(dst, h->d_tmp.as<float>(), n * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    out_dims[0] = h->train_N; out_dims[1] = l.cout; out_dims[2] = dh; out_dims[3] = dw;
    return LWP_OK;
}

extern "C" int lwp_debug_backward_splits(lwp_handle h, int idx) {
    if (!h || idx < 0 || idx >= (int)h->bwd_splits.size()) return LWP_ERR_ARG;
    return h->bwd_splits[idx];
}

extern "C" int lwp_debug_backward_dw_splits(lwp_handle h, int idx) {
    if (!h || idx < 0 || idx >= (int)h->bwd_dw_splits.size()) return LWP_ERR_ARG;
    return h->bwd_dw_splits[idx];
}

// the gradient kernels alone (tests): crafted tensors in, results out, the partials in a scratch allocation.
// Ranges of at most max_chunk pixels (0: the plan's own), so that a small tensor runs several of them
static void clamp_chunk(int64_t M, int max_chunk, int* splits, int* chunk) {
    if (max_chunk > 0 && *chunk > max_chunk) { *chunk = max_chunk; *splits = (int)((M + max_chunk - 1) / max_chunk); }
}

// the depthwise family (lwp_debug_dw_grad: the cpm's form, windows, beta, accumulate; lwp_debug_dw_grad_sd: the backbone's, with
// stride, dilation and the sum of dZ): the entry points check their arguments, fill the parameters here and run them below
static DwGradParams debug_dw_params(const float* dz, int dz_ld, const float* x, int x_ld, const float* w, float* dx, int dx_ld, int N, int H, int W,
                                    int C, int stride, int dil, int beta, int max_chunk) {
    DwGradParams p{};
    p.dz = dz; p.dz_ld = dz_ld; p.x = x; p.x_ld = x_ld; p.w = w; p.dx = dx; p.dx_ld = dx_ld;
    p.N = N; p.H = H; p.W = W; p.Ho = (H - 1) / stride + 1; p.Wo = (W - 1) / stride + 1; p.C = C; p.stride = stride; p.dil = dil; p.beta = beta;
    const int64_t M = (int64_t)N * p.Ho * p.Wo;
    dw_wgrad_plan(M, C, &p.splits, &p.chunk);
    clamp_chunk(M, max_chunk, &p.splits, &p.chunk);
    return p;
}
// g null: nine rows of partials, dw written with `accumulate`; else ten, the tenth summed into g
static int debug_dw_grad(lwp_context* h, DwGradParams p, float* dw, float* g, int accumulate, int* splits) {
    HIP_TRY(h, hipSetDevice(h->device));
    DevBuf part;
    HIP_TRY(h, part.ensure((size_t)p.splits * (g ? 10 : 9) * p.C * sizeof(float)));
    p.partial = part.as<float>();
    HIP_TRY(h, launch_dw_wgrad(p, g != nullptr, h->stream));
    HIP_TRY(h, launch_dw_wgrad_reduce(p, dw, g, accumulate, h->stream));
    HIP_TRY(h, launch_dw_dgrad(p, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    *splits = p.splits;
    return LWP_OK;
}

extern "C" int lwp_debug_dw_grad_sd(lwp_handle h, const float* dz, const float* x, const float* w, int N, int H, int W, int C, int stride, int dil,
                                    int max_chunk, float* dx, float* G, float* g, int* splits) {
    if (!h || !dz || !x || !w || !dx || !G || !g || !splits) return fail(h, LWP_ERR_ARG, "null argument");
    if (N < 1 || H < 1 || W < 1 || C < 4 || (C & 3) || (stride != 1 && stride != 2) || (dil != 1 && dil != 2) || max_chunk < 0 || (max_chunk & 15))
        return fail(h, LWP_ERR_ARG, "bad shape (C a multiple of 4, stride and dilation 1 or 2, max_chunk a multiple of 16)");
    const DwGradParams p = debug_dw_params(dz, C, x, C, w, dx, C, N, H, W, C, stride, dil, 0, max_chunk);
    return debug_dw_grad(h, p, G, g, 0, splits);
}

extern "C" int lwp_debug_stem_wgrad(lwp_handle h, const float* dz, const float* x, int N, int H, int W, int max_chunk, float* G, float* g, int* splits) {
    if (!h || !dz || !x || !G || !g || !splits) return fail(h, LWP_ERR_ARG, "null argument");
    if (N < 1 || H < 1 || W < 1 || max_chunk < 0) return fail(h, LWP_ERR_ARG, "bad shape");
    HIP_TRY(h, hipSetDevice(h->device));
    StemWgradParams p{};
    p.dz = dz; p.dz_ld = 32; p.x = x;
    p.N = N; p.H = H; p.W = W; p.Ho = (H - 1) / 2 + 1; p.Wo = (W - 1) / 2 + 1;
    const int64_t M = (int64_t)N * p.Ho * p.Wo;
    stem_wgrad_plan(M, &p.splits, &p.chunk);
    clamp_chunk(M, max_chunk, &p.splits, &p.chunk);
    DevBuf part;
    HIP_TRY(h, part.ensure((size_t)p.splits * 28 * 32 * sizeof(float)));
    p.partial = part.as<float>();
    HIP_TRY(h, launch_stem_wgrad(p, h->stream));
    HIP_TRY(h, launch_stem_wgrad_reduce(p, G, g, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    *splits = p.splits;
    return LWP_OK;
}

// the stage and cpm gradient kernels alone (tests).  The argument rules of the launchers are checked here first, so that a
// refused call is LWP_ERR_ARG and nothing is launched.
static bool window_ok(const void* p, int ld, int off, int C) { return p && off >= 0 && C >= 1 && (int64_t)off + C <= ld; }

extern "C" int lwp_debug_conv_grad(lwp_handle h, const float* dz, int dz_ld, int dz_off, const float* x, int x_ld, int x_off, const float* w,
                                   int N, int H, int W, int cout, int cin, int ks, int dil, int pad_mode, int max_chunk, int acc_from,
                                   int no_bias, int accumulate, float* dx, int dx_ld, int dx_off, float* dw, float* db, int* splits) {
    if (!h || !w || !dw || !db || !splits) return fail(h, LWP_ERR_ARG, "null argument");
    if (N < 1 || H < 1 || W < 1 || cout < 1 || cin < 1 || cout > 4096 || cin > 4096 || (int64_t)N * H * W >= (1ll << 24))
        return fail(h, LWP_ERR_ARG, "bad shape");
    if ((ks != 1 && ks != 3) || (dil != 1 && dil != 2)) return fail(h, LWP_ERR_ARG, "ks is 1 or 3, dil 1 or 2");
    if (max_chunk < 0 || (max_chunk & 15)) return fail(h, LWP_ERR_ARG, "max_chunk is a multiple of 16");
    if (pad_mode != LWP_PAD_GRAPH && pad_mode != LWP_PAD_RAW) return fail(h, LWP_ERR_ARG, "unknown pad mode");
    if (pad_mode == LWP_PAD_RAW && ((cout & 15) || (cin & 3))) return fail(h, LWP_ERR_ARG, "raw weights need cout a multiple of 16 and cin a multiple of 4");
    if (acc_from < 0 || acc_from > cin) return fail(h, LWP_ERR_ARG, "acc_from is in 0..cin");
    if (!window_ok(dz, dz_ld, dz_off, cout) || !window_ok(x, x_ld, x_off, cin) || !window_ok(dx, dx_ld, dx_off, cin))
        return fail(h, LWP_ERR_ARG, "a window does not fit its row stride");
    HIP_TRY(h, hipSetDevice(h->device));
    const int taps = ks * ks;
    const int cout_pad = pad_mode == LWP_PAD_RAW ? cout : (cout + 63) / 64 * 64;
    const int cin_pad = pad_mode == LWP_PAD_RAW ? cin : (cin + 31) / 32 * 32;
    // OIHW -> [taps][cout_pad][cin_pad], zero-filled
    std::vector<float> raw((size_t)cout * cin * taps), packed((size_t)taps * cout_pad * cin_pad, 0.0f);
    HIP_TRY(h, hipMemcpy(raw.data(), w, raw.size() * sizeof(float), hipMemcpyDeviceToHost));
    for (int o = 0; o < cout; ++o)
        for (int ci = 0; ci < cin; ++ci)
            for (int t = 0; t < taps; ++t) packed[((size_t)t * cout_pad + o) * cin_pad + ci] = raw[((size_t)o * cin + ci) * taps + t];
    DevBuf wbuf, part;
    HIP_TRY(h, wbuf.ensure(packed.size() * sizeof(float)));
    HIP_TRY(h, hipMemcpy(wbuf.as<float>(), packed.data(), packed.size() * sizeof(float), hipMemcpyHostToDevice));
    WgradParams p{};
    p.dz = dz + dz_off; p.dz_ld = dz_ld; p.x = x + x_off; p.x_ld = x_ld;
    p.N = N; p.H = H; p.W = W; p.cout = cout; p.cin = cin; p.ks = ks; p.dil = dil; p.no_bias = no_bias ? 1 : 0;
    const int64_t M = (int64_t)N * H * W;
    wgrad_plan(M, cout, cin, ks, &p.splits, &p.chunk);
    clamp_chunk(M, max_chunk, &p.splits, &p.chunk);
    if (p.splits > 65535) return fail(h, LWP_ERR_ARG, "too many pixel ranges");
    HIP_TRY(h, part.ensure(wgrad_partial_floats(p) * sizeof(float)));
    p.partial = part.as<float>();
    const DgradParams d = dgrad_params(p.dz, dz_ld, wbuf.as<float>(), cout_pad, cin_pad, dx + dx_off, dx_ld, acc_from, N, H, W, cout, cin, ks, dil);
    HIP_TRY(h, launch_wgrad(p, h->stream, h->bwd_prec));
    HIP_TRY(h, launch_wgrad_reduce(p, dw, db, accumulate ? 1 : 0, h->stream));
    HIP_TRY(h, launch_dgrad(d, h->stream, h->bwd_prec));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    *splits = p.splits;
    return LWP_OK;
}

static bool quad_window_ok(const void* p, int ld, int C) { return p && ((uintptr_t)p & 15) == 0 && ld >= C && (ld & 3) == 0; }

extern "C" int lwp_debug_dw_grad(lwp_handle h, const float* dz, int dz_ld, const float* x, int x_ld, const float* w, int N, int H, int W, int C,
                                 int beta, int accumulate, int max_chunk, float* dx, int dx_ld, float* dw, int* splits) {
    if (!h || !w || !dw || !splits) return fail(h, LWP_ERR_ARG, "null argument");
    if (N < 1 || H < 1 || W < 1 || C < 4 || (C & 3) || (int64_t)N * H * W >= (1ll << 24) || max_chunk < 0 || (max_chunk & 15))
        return fail(h, LWP_ERR_ARG, "bad shape (C a multiple of 4, max_chunk a multiple of 16)");
    if (!quad_window_ok(dz, dz_ld, C) || !quad_window_ok(x, x_ld, C) || !quad_window_ok(dx, dx_ld, C) || ((uintptr_t)w & 15))
        return fail(h, LWP_ERR_ARG, "row strides are multiples of 4 and at least C, pointers 16-byte aligned");
    const DwGradParams p = debug_dw_params(dz, dz_ld, x, x_ld, w, dx, dx_ld, N, H, W, C, 1, 1, beta ? 1 : 0, max_chunk);
    if (p.splits > 65535) return fail(h, LWP_ERR_ARG, "too many pixel ranges");
    return debug_dw_grad(h, p, dw, nullptr, accumulate ? 1 : 0, splits);
}

extern "C" int lwp_debug_loss_grad(lwp_handle h, const float* const* outs, float* const* dst, int S, int ld, const float* keypoint_maps,
                                   const float* paf_maps, const float* mask, int N, int CH, int CP, int hw, float scale) {
    if (!h || !outs || !dst || !keypoint_maps || !paf_maps || !mask) return fail(h, LWP_ERR_ARG, "null argument");
    if (S < 1 || S > kLossMaxOuts || N < 1 || CH < 1 || CP < 1 || hw < 1 || ld < std::max(CH, CP) || (int64_t)N * hw * ld >= (1ll << 31))
        return fail(h, LWP_ERR_ARG, "bad shape");
    LossGradParams p{};
    for (int s = 0; s < S; ++s) {
        if (!outs[s] || !dst[s]) return fail(h, LWP_ERR_ARG, "null argument");
        p.outs[s] = outs[s]; p.dst[s] = dst[s];
    }
    p.S = S; p.ld = ld; p.keypoint_maps = keypoint_maps; p.paf_maps = paf_maps; p.mask = mask;
    p.N = N; p.CH = CH; p.CP = CP; p.hw = hw; p.scale = scale;
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, launch_loss_grad(p, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return LWP_OK;
}

static bool rows_ok(int64_t M, int C, int ld) { return M >= 1 && C >= 1 && ld >= C && M * ld < (1ll << 32); }

extern "C" int lwp_debug_relu_mask(lwp_handle h, float* g, int g_ld, const float* y, int y_ld, const float* res, int res_ld, int64_t M, int C) {
    if (!h || !g || !y) return fail(h, LWP_ERR_ARG, "null argument");
    if (!rows_ok(M, C, g_ld) || !rows_ok(M, C, y_ld) || (res && !rows_ok(M, C, res_ld))) return fail(h, LWP_ERR_ARG, "bad shape");
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, launch_relu_mask(g, g_ld, y, y_ld, res, res_ld, M, C, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return LWP_OK;
}

extern "C" int lwp_debug_grad_add(lwp_handle h, float* dst, int dst_ld, const float* src, int src_ld, int64_t M, int C, int beta) {
    if (!h || !dst || !src) return fail(h, LWP_ERR_ARG, "null argument");
    if (!rows_ok(M, C, dst_ld) || !rows_ok(M, C, src_ld)) return fail(h, LWP_ERR_ARG, "bad shape");
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, launch_grad_add(dst, dst_ld, src, src_ld, M, C, beta ? 1 : 0, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return LWP_OK;
}

extern "C" int lwp_debug_elu_grad(lwp_handle h, float* g, int g_ld, const float* y, int y_ld, int64_t M, int C) {
    if (!h) return fail(h, LWP_ERR_ARG, "null argument");
    if (C < 4 || (C & 3) || !rows_ok(M, C, g_ld) || !rows_ok(M, C, y_ld) || !quad_window_ok(g, g_ld, C) || !quad_window_ok(y, y_ld, C))
        return fail(h, LWP_ERR_ARG, "bad shape (C and the row strides multiples of 4, pointers 16-byte aligned)");
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, launch_elu_grad(g, g_ld, y, y_ld, M, C, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return LWP_OK;
}

extern "C" int lwp_debug_pw_fold(lwp_handle h, const float* w, const float* gamma, const float* var, float* out, int cout, int cin) {
    if (!h || !w || !gamma || !var || !out || cout < 1 || cin < 1) return fail(h, LWP_ERR_ARG, "bad argument");
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, launch_pw_fold(w, gamma, var, out, cout, cin, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return LWP_OK;
}

extern "C" int lwp_debug_bn_chain(lwp_handle h, const float* G, const float* g, const float* W, const float* b, const float* gamma,
                                  const float* mean, const float* var, float* dW, float* db, float* dgamma, float* dbeta, int cout, int K,
                                  int accumulate) {
    if (!h || !G || !g || !W || !b || !gamma || !mean || !var || !dW || !dgamma || !dbeta || cout < 1 || K < 1) return fail(h, LWP_ERR_ARG, "bad argument");
    BnChainParams p{};
    p.G = G; p.g = g; p.W = W; p.b = b; p.gamma = gamma; p.mean = mean; p.var = var;
    p.dW = dW; p.db = db; p.dgamma = dgamma; p.dbeta = dbeta; p.cout = cout; p.K = K; p.accumulate = accumulate ? 1 : 0;
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, launch_bn_chain(p, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return LWP_OK;
}

// ---------------------------------------------------------------------------------------------- stage fine-tuning step
// train.py:41-55's parameter groups for the stage parameters: log2 of the learning-rate multiplier in bits 0-1, weight decay in bit 2
static uint32_t stage_adam_group(const std::string& key, int role) {
    const bool refine = key.rfind("refinement_stages.", 0) == 0;
    switch (role) {
    case LWP_ROLE_CONV_W: return (refine ? 2u : 0u) | 4u;
    case LWP_ROLE_CONV_B: return refine ? 3u : 1u;
    case LWP_ROLE_BN_W: return 0u;
    default: return 1u;                            // LWP_ROLE_BN_B
    }
}
// train.py:46-48 with get_parameters.py for the cpm: conv weights with groups == 1 x1 with weight decay, conv biases x2
// without, depthwise weights (cpm.trunk.j.0) x1 without
static uint32_t cpm_adam_group(const std::string& key, int role) {
    if (role == LWP_ROLE_CONV_B) return 1u;
    const bool depthwise = key.rfind("cpm.trunk.", 0) == 0 && key.size() > 8 && key.compare(key.size() - 9, 9, ".0.weight") == 0;
    return depthwise ? 0u : 4u;
}
// train.py:42-45 with get_parameters.py for the backbone: conv weights with groups == 1 (the stem model.0.0 and the pointwise
// model.i.3) x1 with weight decay, depthwise weights (model.i.0, i >= 1) x1 without, BatchNorm weights x1 without, biases x2 without
static uint32_t backbone_adam_group(const std::string& key, int role) {
    if (role == LWP_ROLE_BN_W) return 0u;
    if (role == LWP_ROLE_BN_B) return 1u;
    const bool depthwise = key.rfind("model.0.", 0) != 0 && key.size() > 8 && key.compare(key.size() - 9, 9, ".0.weight") == 0;
    return depthwise ? 0u : 4u;
}
static std::vector<uint32_t> train_adam_groups(int scope, int nref, int C, int NH, int NP) {
    std::vector<uint32_t> v;
    const std::vector<ParamSpec> table = param_table(nref, C, NH, NP);
    for (int part = first_part(scope); part < 3; ++part)
        for (const ParamSpec& p : table)
            if (in_part(part, p.key) && p.role != LWP_ROLE_BN_MEAN && p.role != LWP_ROLE_BN_VAR && p.role != LWP_ROLE_BN_NBT)
                v.push_back(part == 0 ? backbone_adam_group(p.key, p.role) : part == 1 ? cpm_adam_group(p.key, p.role) : stage_adam_group(p.key, p.role));
    return v;
}
static std::vector<uint32_t> stage_adam_groups(int nref, int C, int NH, int NP) { return train_adam_groups(LWP_TRAIN_STAGES, nref, C, NH, NP); }

extern "C" int lwp_train_adam_group(int scope, int nref, int C, int NH, int NP, int index, int* lr_mult, int* weight_decay_on) {
    if (!train_shape_ok(scope, nref, C, NH, NP) || !lr_mult || !weight_decay_on) return fail(nullptr, LWP_ERR_ARG, "bad argument");
    const auto g = train_adam_groups(scope, nref, C, NH, NP);
    if (index < 0 || index >= (int)g.size()) return fail(nullptr, LWP_ERR_ARG, "index out of range");
    *lr_mult = 1 << (g[index] & 3u);
    *weight_decay_on = (g[index] & 4u) ? 1 : 0;
    return LWP_OK;
}

extern "C" int lwp_stage_adam_group(int nref, int C, int NH, int NP, int index, int* lr_mult, int* weight_decay_on) {
    if (nref < 0 || C <= 0 || NH <= 0 || NP <= 0 || !lr_mult || !weight_decay_on) return fail(nullptr, LWP_ERR_ARG, "bad argument");
    const auto g = stage_adam_groups(nref, C, NH, NP);
    if (index < 0 || index >= (int)g.size()) return fail(nullptr, LWP_ERR_ARG, "index out of range");
    *lr_mult = 1 << (g[index] & 3u);
    *weight_decay_on = (g[index] & 4u) ? 1 : 0;
    return LWP_OK;
}

static int adam_handle_check(lwp_context* h) {
    if (!h) return fail(h, LWP_ERR_ARG, "handle is null");
    if (h->dtype != LWP_F32) return fail(h, LWP_ERR_ARG, "the stage optimiser runs on fp32 handles only (this one is bf16 / fp16)");
    if (!h->weights_loaded) return fail(h, LWP_ERR_ARG, "weights not loaded (call lwp_load_weights first)");
    if (!h->raw_loaded) return fail(h, LWP_ERR_ARG, "the stage optimiser needs the raw parameters: load them with lwp_load_weights (a weight blob holds folded weights only)");
    return LWP_OK;
}

// the two device tables, built once per handle: chunks of at most kAdamChunk elements that never cross a parameter (a parameter
// that starts off the 16-byte grid gets a head chunk up to the grid), and one descriptor per stage layer
static int ensure_adam_tables(lwp_context* h) {
    if (h->d_adam_chunks) return LWP_OK;
    const std::vector<uint32_t> groups = train_adam_groups(h->scope, h->g.nref, h->g.C, h->g.NH, h->g.NP);
    std::vector<AdamChunk> chunks;
    for (size_t i = 0; i < h->gspec.size(); ++i) {
        const auto& s = h->gspec[i];
        size_t n = 1;
        for (int d = 0; d < s.ndim; ++d) n *= (size_t)s.shape[d];
        const size_t roff = h->raw_off.at(s.key);
        size_t done = 0;
        while (done < n) {
            size_t take = std::min<size_t>(kAdamChunk, n - done);
            const size_t mis = (s.off + done) & 3;
            if (mis && ((roff + done) & 3) == mis) take = std::min<size_t>(take, 4 - mis);
            chunks.push_back(AdamChunk{(uint32_t)(s.off + done), (uint32_t)(roff + done), (uint32_t)take, groups[i]});
            done += take;
        }
    }
    auto raw_at = [&](const std::string& k) { auto it = h->raw_off.find(k); return it == h->raw_off.end() ? -1 : (int)it->second; };
    std::vector<RepackLayer> tab;
    uint32_t blocks = 0;
    std::vector<DwRepack> dws;
    StemRepack stem{};
    bool has_stem = false;
    for (size_t i = (size_t)(h->tp.cut + 1); i < h->g.layers.size(); ++i) {
        const Layer& l = h->g.layers[i];
        if (l.kind == L_STEM) {                            // model.0 (LWP_TRAIN_ALL)
            stem.w_raw = raw_at(l.conv_key + ".weight");
            stem.gamma = raw_at(l.bn_key + ".weight"); stem.beta = raw_at(l.bn_key + ".bias");
            stem.mean = raw_at(l.bn_key + ".running_mean"); stem.var = raw_at(l.bn_key + ".running_var");
            stem.w_off = (uint32_t)l.w_off; stem.b_off = (uint32_t)l.b_off;
            if (stem.w_raw < 0 || stem.gamma < 0 || stem.beta < 0 || stem.mean < 0 || stem.var < 0) return fail(h, LWP_ERR_STATE, "raw parameters of '" + l.name + "' missing");
            has_stem = true;
            continue;
        }
        if (l.kind == L_DW || l.kind == L_DWPW) {          // the cpm trunk (no BatchNorm), the backbone's blocks (LWP_TRAIN_ALL: BatchNorm behind both halves)
            DwRepack d{};
            d.C = l.cin; d.cout = l.kind == L_DWPW ? l.cout : 0;
            d.dw_raw = raw_at(l.conv_key + ".weight"); d.pw_raw = l.kind == L_DWPW ? raw_at(l.conv2_key + ".weight") : -1;
            d.w_off = (uint32_t)l.w_off; d.b_off = (uint32_t)l.b_off; d.w2_off = (uint32_t)l.w2_off; d.b2_off = (uint32_t)l.b2_off;
            if (d.dw_raw < 0 || (d.cout > 0 && d.pw_raw < 0)) return fail(h, LWP_ERR_STATE, "raw weights of '" + l.name + "' missing");
            d.dw_gamma = d.dw_beta = d.dw_mean = d.dw_var = d.pw_gamma = d.pw_beta = d.pw_mean = d.pw_var = -1;
            if (!l.bn_key.empty()) {
                d.dw_gamma = raw_at(l.bn_key + ".weight"); d.dw_beta = raw_at(l.bn_key + ".bias");
                d.dw_mean = raw_at(l.bn_key + ".running_mean"); d.dw_var = raw_at(l.bn_key + ".running_var");
                if (d.dw_gamma < 0 || d.dw_beta < 0 || d.dw_mean < 0 || d.dw_var < 0) return fail(h, LWP_ERR_STATE, "raw BatchNorm parameters of '" + l.name + "' missing");
            }
            if (l.kind == L_DWPW && !l.bn2_key.empty()) {
                d.pw_gamma = raw_at(l.bn2_key + ".weight"); d.pw_beta = raw_at(l.bn2_key + ".bias");
                d.pw_mean = raw_at(l.bn2_key + ".running_mean"); d.pw_var = raw_at(l.bn2_key + ".running_var");
                if (d.pw_gamma < 0 || d.pw_beta < 0 || d.pw_mean < 0 || d.pw_var < 0) return fail(h, LWP_ERR_STATE, "raw BatchNorm parameters of '" + l.name + "' missing");
            }
            dws.push_back(d);
            continue;
        }
        if (l.kind != L_GEMM || l.blocks.size() > 2 || (!l.blocks.empty() && l.ks != 1) || l.cin_pad % 32 || l.cout_pad % 32)
            return fail(h, LWP_ERR_STATE, "stage layer '" + l.name + "' has no device repack");
        RepackLayer r{};
        r.block_begin = blocks;
        r.w_off = (uint32_t)l.w_off; r.w2_off = (uint32_t)l.w2_off; r.b_off = (uint32_t)l.b_off;
        r.cin = l.cin; r.cout = l.cout; r.cin_pad = l.cin_pad; r.cout_pad = l.cout_pad; r.taps = l.ks * l.ks;
        r.w_raw = raw_at(l.conv_key + ".weight");
        r.b_raw = l.has_bias ? raw_at(l.conv_key + ".bias") : -1;
        r.gamma_raw = r.beta_raw = r.mean_raw = r.var_raw = -1;
        if (!l.bn_key.empty()) {
            r.gamma_raw = raw_at(l.bn_key + ".weight"); r.beta_raw = raw_at(l.bn_key + ".bias");
            r.mean_raw = raw_at(l.bn_key + ".running_mean"); r.var_raw = raw_at(l.bn_key + ".running_var");
            if (r.gamma_raw < 0 || r.beta_raw < 0 || r.mean_raw < 0 || r.var_raw < 0) return fail(h, LWP_ERR_STATE, "raw BatchNorm parameters of '" + l.name + "' missing");
        }
        r.n_blocks = (int)l.blocks.size();
        for (int b = 0; b < r.n_blocks; ++b) {
            const WBlock& wb = l.blocks[b];
            r.blk[b] = RepackBlock{raw_at(wb.conv_key + ".weight"), raw_at(wb.conv_key + ".bias"), wb.out_off, wb.in_off, wb.cout, wb.cin};
            if (r.blk[b].w_raw < 0 || r.blk[b].b_raw < 0 || wb.out_off + wb.cout > l.cout_pad || wb.in_off + wb.cin > l.cin_pad)
                return fail(h, LWP_ERR_STATE, "source conv of '" + l.name + "' missing or out of range");
        }
        if (r.n_blocks == 0 && r.w_raw < 0) return fail(h, LWP_ERR_STATE, "raw weight of '" + l.name + "' missing");
        blocks += (uint32_t)(r.taps * (l.cin_pad / 32) * (l.cout_pad / 32));
        tab.push_back(r);
    }
    DevBuf d_tab, d_chunks;                            // the handle takes them once both are uploaded
    HIP_TRY(h, d_tab.ensure(std::max<size_t>(tab.size(), 1) * sizeof(RepackLayer)));
    HIP_TRY(h, hipMemcpy(d_tab.as<void>(), tab.data(), tab.size() * sizeof(RepackLayer), hipMemcpyHostToDevice));
    HIP_TRY(h, d_chunks.ensure(std::max<size_t>(chunks.size(), 1) * sizeof(AdamChunk)));
    HIP_TRY(h, hipMemcpy(d_chunks.as<void>(), chunks.data(), chunks.size() * sizeof(AdamChunk), hipMemcpyHostToDevice));
    h->d_repack = std::move(d_tab); h->repack_layers = (int)tab.size(); h->repack_blocks = (int)blocks;
    h->d_adam_chunks = std::move(d_chunks); h->adam_chunks = (int)chunks.size();
    h->dw_repack = dws;
    h->stem_repack = stem; h->has_stem_repack = has_stem;
    return LWP_OK;
}

// exp_avg and exp_avg_sq, zeroed on the handle's stream when first needed
static int ensure_adam_state(lwp_context* h) {
    if (h->d_adam) return LWP_OK;
    h->adam_sq_off = (h->grad_floats + 3) / 4 * 4;
    const size_t bytes = std::max<size_t>(2 * h->adam_sq_off, 4) * sizeof(float);
    HIP_TRY(h, h->d_adam.ensure(bytes));
    HIP_TRY(h, hipMemsetAsync(h->d_adam.as<float>(), 0, bytes, h->stream));
    h->adam_t = 0;
    return LWP_OK;
}

struct AdamArgs { const float* grads; double base_lr, beta1, beta2, eps, weight_decay; };

static int adam_args_check(lwp_context* h, const AdamArgs& a) {
    if (!a.grads) return fail(h, LWP_ERR_ARG, "grads_device is null");
    if (!std::isfinite(a.base_lr) || !(a.base_lr > 0.0)) return fail(h, LWP_ERR_ARG, "base_lr must be finite and positive");
    if (!(a.beta1 >= 0.0 && a.beta1 < 1.0) || !(a.beta2 >= 0.0 && a.beta2 < 1.0)) return fail(h, LWP_ERR_ARG, "betas must lie in [0, 1)");
    if (!std::isfinite(a.eps) || a.eps < 0.0) return fail(h, LWP_ERR_ARG, "eps must be finite and not negative");
    if (!std::isfinite(a.weight_decay) || a.weight_decay < 0.0) return fail(h, LWP_ERR_ARG, "weight_decay must be finite and not negative");
    return LWP_OK;
}

// launch parameters of step `t` on the given arrays; the bias corrections and the learning rates are host doubles
static AdamParams adam_params(lwp_context* h, const AdamArgs& a, int64_t t, float* raw, float* state) {
    AdamParams p{};
    p.grads = a.grads; p.raw = raw; p.exp_avg = state; p.exp_avg_sq = state + h->adam_sq_off;
    p.chunks = h->d_adam_chunks.as<AdamChunk>(); p.n_chunks = h->adam_chunks;
    p.vec_ok = (((uintptr_t)p.grads | (uintptr_t)p.raw | (uintptr_t)p.exp_avg | (uintptr_t)p.exp_avg_sq) & 15) == 0;
    const double bc1 = 1.0 - std::pow(a.beta1, (double)t), bc2 = 1.0 - std::pow(a.beta2, (double)t);
    for (int k = 0; k < 4; ++k) p.step_size[k] = a.base_lr * (double)(1 << k) / bc1;
    p.one_minus_b1 = 1.0 - a.beta1; p.b2 = a.beta2; p.one_minus_b2 = 1.0 - a.beta2;
    p.sqrt_bc2 = std::sqrt(bc2); p.eps = a.eps; p.weight_decay = a.weight_decay;
    return p;
}

extern "C" int lwp_stage_adam_step(lwp_handle h, const float* grads_device, double base_lr, double beta1, double beta2, double eps,
                                   double weight_decay) {
    int rc = adam_handle_check(h);
    if (rc) return rc;
    const AdamArgs a{grads_device, base_lr, beta1, beta2, eps, weight_decay};
    rc = adam_args_check(h, a);
    if (rc) return rc;
    // the blob is read by the network kernels, which all run on the main stream (a slot's post stream reads maps, never
    // weights), and by the host-synchronous copies of lwp_load_weights / lwp_weights_blob_export / _import, which wait for the
    // main stream first: a write on the main stream is ordered against every reader.  Work in flight whose results the caller has not
    // taken yet would still see consistent weights, but a step between a submit and its fetch is a caller's mistake.
    for (auto& sl : h->slots) if (sl.pending) return fail(h, LWP_ERR_STATE, "pipeline slot pending: fetch it before the optimiser step");
    if (h->async_pending) return fail(h, LWP_ERR_STATE, "an lwp_infer_poses_async is pending: fetch it before the optimiser step");
    HIP_TRY(h, hipSetDevice(h->device));
    rc = ensure_adam_tables(h);
    if (!rc) rc = ensure_adam_state(h);
    if (!rc) rc = order_in(h);
    if (rc) return rc;
    const AdamParams p = adam_params(h, a, h->adam_t + 1, h->d_raw.as<float>(), h->d_adam.as<float>());
    LAUNCH(h, KC_OTHER, launch_stage_adam(p, h->stream));
    h->adam_t += 1;                                    // from here on the raw parameters and the state are those of step t
    h->train_N = 0;                                    // the retained activations belong to the old weights
    hipError_t e = launch_stage_repack(h->d_repack.as<RepackLayer>(), h->repack_layers, h->repack_blocks, h->d_raw.as<float>(), h->d_blob.as<float>(), h->stream);
    for (size_t k = 0; k < h->dw_repack.size() && e == hipSuccess; ++k) e = launch_dw_repack(h->dw_repack[k], h->d_raw.as<float>(), h->d_blob.as<float>(), h->stream);
    if (h->has_stem_repack && e == hipSuccess) e = launch_stem_repack(h->stem_repack, h->d_raw.as<float>(), h->d_blob.as<float>(), h->stream);
    if (e != hipSuccess) {                             // the blob no longer matches the raw parameters: no forward until lwp_load_weights
        h->weights_loaded = false;
        return fail(h, LWP_ERR_HIP, std::string("launch_stage_repack: ") + hipGetErrorString(e) + " (the weight blob is stale: load the weights again)");
    }
    bool ordered = false;
    return order_out(h, h->stream, &ordered);
}

extern "C" int lwp_stage_params_get(lwp_handle h, float* flat_device) {
    int rc = adam_handle_check(h);
    if (rc) return rc;
    if (!flat_device) return fail(h, LWP_ERR_ARG, "flat_device is null");
    HIP_TRY(h, hipSetDevice(h->device));
    rc = order_in(h);
    if (rc) return rc;
    for (const auto& s : h->gspec) {                   // gradient-spec offset <- raw offset, entry by entry
        size_t n = 1;
        for (int d = 0; d < s.ndim; ++d) n *= (size_t)s.shape[d];
        HIP_TRY(h, hipMemcpyAsync(flat_device + s.off, h->raw(s.key), n * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
    }
    bool ordered = false;
    rc = order_out(h, h->stream, &ordered);
    if (rc) return rc;
    if (!ordered) HIP_TRY(h, hipStreamSynchronize(h->stream));
    return LWP_OK;
}

extern "C" int lwp_stage_adam_state_get(lwp_handle h, float* exp_avg_device, float* exp_avg_sq_device, int64_t* step) {
    int rc = adam_handle_check(h);
    if (rc) return rc;
    if (!exp_avg_device || !exp_avg_sq_device || !step) return fail(h, LWP_ERR_ARG, "null argument");
    HIP_TRY(h, hipSetDevice(h->device));
    rc = order_in(h);
    if (rc) return rc;
    const size_t bytes = h->grad_floats * sizeof(float);
    if (h->d_adam) {
        HIP_TRY(h, hipMemcpyAsync(exp_avg_device, h->d_adam.as<float>(), bytes, hipMemcpyDeviceToDevice, h->stream));
        HIP_TRY(h, hipMemcpyAsync(exp_avg_sq_device, h->d_adam.as<float>() + h->adam_sq_off, bytes, hipMemcpyDeviceToDevice, h->stream));
    } else {
        HIP_TRY(h, hipMemsetAsync(exp_avg_device, 0, bytes, h->stream));
        HIP_TRY(h, hipMemsetAsync(exp_avg_sq_device, 0, bytes, h->stream));
    }
    *step = h->d_adam ? h->adam_t : 0;
    bool ordered = false;
    rc = order_out(h, h->stream, &ordered);
    if (rc) return rc;
    if (!ordered) HIP_TRY(h, hipStreamSynchronize(h->stream));
    return LWP_OK;
}

extern "C" int lwp_stage_adam_state_set(lwp_handle h, const float* exp_avg_device, const float* exp_avg_sq_device, int64_t step) {
    int rc = adam_handle_check(h);
    if (rc) return rc;
    if (!exp_avg_device || !exp_avg_sq_device) return fail(h, LWP_ERR_ARG, "null argument");
    if (step < 0) return fail(h, LWP_ERR_ARG, "step must not be negative");
    HIP_TRY(h, hipSetDevice(h->device));
    rc = ensure_adam_state(h);
    if (!rc) rc = order_in(h);
    if (rc) return rc;
    const size_t bytes = h->grad_floats * sizeof(float);
    HIP_TRY(h, hipMemcpyAsync(h->d_adam.as<float>(), exp_avg_device, bytes, hipMemcpyDeviceToDevice, h->stream));
    HIP_TRY(h, hipMemcpyAsync(h->d_adam.as<float>() + h->adam_sq_off, exp_avg_sq_device, bytes, hipMemcpyDeviceToDevice, h->stream));
    h->adam_t = step;
    bool ordered = false;
    rc = order_out(h, h->stream, &ordered);            // the caller may free or overwrite its arrays once its stream gets here
    if (rc) return rc;
    if (!ordered) HIP_TRY(h, hipStreamSynchronize(h->stream));
    return LWP_OK;
}

extern "C" int lwp_stage_adam_reset(lwp_handle h) {
    int rc = adam_handle_check(h);
    if (rc) return rc;
    h->adam_t = 0;
    if (!h->d_adam) return LWP_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    rc = order_in(h);                                  // the caller may still read an array lwp_stage_adam_state_get handed over
    if (rc) return rc;
    HIP_TRY(h, hipMemsetAsync(h->d_adam.as<float>(), 0, std::max<size_t>(2 * h->adam_sq_off, 4) * sizeof(float), h->stream));
    return LWP_OK;
}

// the two kernels alone, `iters` back-to-back launches each between two events (ms[0]: Adam, ms[1]: repack), on scratch copies
// of the raw parameters, the state and the blob: the handle's weights and optimiser state do not move
extern "C" int lwp_time_stage_adam_step(lwp_handle h, const float* grads_device, double base_lr, double beta1, double beta2, double eps,
                                        double weight_decay, int iters, float* ms) {
    int rc = adam_handle_check(h);
    if (rc) return rc;
    if (!ms || iters <= 0) return fail(h, LWP_ERR_ARG, "bad argument");
    const AdamArgs a{grads_device, base_lr, beta1, beta2, eps, weight_decay};
    rc = adam_args_check(h, a);
    if (rc) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    rc = ensure_adam_tables(h);
    if (rc) return rc;
    if (!h->adam_sq_off) h->adam_sq_off = (h->grad_floats + 3) / 4 * 4;
    DevBuf raw, state, blob;
    const size_t state_bytes = std::max<size_t>(2 * h->adam_sq_off, 4) * sizeof(float);
    HIP_TRY(h, raw.ensure(std::max<size_t>(h->raw_floats, 1) * sizeof(float)));
    HIP_TRY(h, state.ensure(state_bytes));
    HIP_TRY(h, blob.ensure(h->g.blob_floats * sizeof(float)));
    rc = order_in(h);
    if (rc) return rc;
    HIP_TRY(h, hipMemcpyAsync(raw.as<void>(), h->d_raw.as<float>(), h->raw_floats * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
    HIP_TRY(h, hipMemsetAsync(state.as<void>(), 0, state_bytes, h->stream));
    HIP_TRY(h, hipMemcpyAsync(blob.as<void>(), h->d_blob.as<float>(), h->g.blob_floats * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
    const AdamParams p = adam_params(h, a, 1, raw.as<float>(), state.as<float>());
    rc = time_on_stream(h, iters, [&]() { LAUNCH(h, KC_OTHER, launch_stage_adam(p, h->stream)); return (int)LWP_OK; }, &ms[0]);
    if (!rc)
        rc = time_on_stream(h, iters, [&]() {
            LAUNCH(h, KC_OTHER, launch_stage_repack(h->d_repack.as<RepackLayer>(), h->repack_layers, h->repack_blocks, raw.as<float>(), blob.as<float>(), h->stream));
            for (const DwRepack& d : h->dw_repack) LAUNCH(h, KC_OTHER, launch_dw_repack(d, raw.as<float>(), blob.as<float>(), h->stream));
            if (h->has_stem_repack) LAUNCH(h, KC_OTHER, launch_stem_repack(h->stem_repack, raw.as<float>(), blob.as<float>(), h->stream));
            return (int)LWP_OK; }, &ms[1]);
    (void)hipStreamSynchronize(h->stream);             // the scratch arrays are freed on return
    return rc;
}

// ---------------------------------------------------------------------------------------------- introspection
extern "C" int lwp_layer_count(lwp_handle h) { return h ? (int)h->g.layers.size() : LWP_ERR_ARG; }

extern "C" int lwp_layer_info(lwp_handle h, int idx, char* name, int name_cap, int* kind, int* cin, int* cout, int* ks,
                              int* stride, int* dil, int64_t* macs_per_pixel) {
    if (!h || idx < 0 || idx >= (int)h->g.layers.size() || !name) return fail(h, LWP_ERR_ARG, "bad argument");
    const Layer& l = h->g.layers[idx];
    if ((int)l.name.size() + 1 > name_cap) return fail(h, LWP_ERR_ARG, "name buffer too small");
    std::strcpy(name, l.name.c_str());
    if (kind) *kind = l.kind;
    if (cin) *cin = l.cin;
    if (cout) *cout = l.cout;
    if (ks) *ks = l.ks;
    if (stride) *stride = l.stride;
    if (dil) *dil = l.dil;
    if (macs_per_pixel) *macs_per_pixel = l.macs_per_pixel;
    return LWP_OK;
}

extern "C" int lwp_debug_layer_output(lwp_handle h, const float* in, int N, int H, int W, int idx, float* dst, size_t dst_floats,
                                      int out_dims[4]) {
    if (!h || !in || !dst || !out_dims || idx < 0 || idx >= (int)h->g.layers.size()) return fail(h, LWP_ERR_ARG, "bad argument");
    int rc = check_frame_shape(h, N, H, W);
    if (rc) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    rc = ensure_activations(h, N, H, W);
    if (rc) return rc;
    const float* d_in = nullptr;
    rc = stage_input(h, in, LWP_MEM_HOST, (size_t)N * 3 * H * W * sizeof(float), &d_in);
    if (rc) return rc;
    h->record_variants = true;
    rc = enqueue_forward(h, h->g.layers, 0, idx + 1, d_in, N, H, W, nullptr);
    h->record_variants = false;
    if (rc) return rc;
    const Layer& l = h->g.layers[idx];
    int dh, dw;
    level_dims(H, W, h->g.bufs[l.dst.buf].level, &dh, &dw);
    const size_t n = (size_t)N * l.cout * dh * dw;
    if (dst_floats < n) return fail(h, LWP_ERR_ARG, "dst too small");
    HIP_TRY(h, h->d_tmp.ensure(n * sizeof(float)));
    // NHWC window (ld, coff) -> compact NCHW
    if (h->dtype != LWP_F32) HIP_TRY(h, launch_nchw_from_nhwc_bf16(buf_at(h, l.dst), l.dst.ld, h->d_tmp.as<float>(), N, dh * dw, l.cout, h->stream, h->dtype == LWP_F16));
    else HIP_TRY(h, launch_nchw_from_nhwc(buf_at(h, l.dst), l.dst.ld, h->d_tmp.as<float>(), N, dh * dw, l.cout, h->stream));
    HIP_TRY(h, hipMemcpyAsync(dst, h->d_tmp.as<float>(), n * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    out_dims[0] = N; out_dims[1] = l.cout; out_dims[2] = dh; out_dims[3] = dw;
    return LWP_OK;
}

extern "C" int lwp_debug_frames_per_pass(lwp_handle h, int N, int H, int W) {
    if (!h || N <= 0 || H <= 0 || W <= 0) return LWP_ERR_ARG;
    return frames_per_pass(h, N, H, W);
}

extern "C" int lwp_debug_post_counts_ex(lwp_handle h, int frame, int* peaks, int* kpts, int* candidates, int* picked, int K, int L) {
    if (!h || !peaks || !kpts || !candidates || !picked) return fail(h, LWP_ERR_ARG, "null argument");
    if (K != h->ws.K || L != h->ws.L) return fail(h, LWP_ERR_ARG, "K / L do not match the skeleton of the last run");
    if (frame < 0 || frame >= h->last_N) return fail(h, LWP_ERR_ARG, "frame outside the last batch");   // (last_N <= ws.N: whatever frees the workspace zeroes it)
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (h->post_stream && h->post_stream != h->stream) HIP_TRY(h, hipStreamSynchronize(h->post_stream));
    HIP_TRY(h, hipMemcpy(peaks, h->ws.seen + (size_t)frame * (K + L), K * sizeof(int), hipMemcpyDeviceToHost));
    HIP_TRY(h, hipMemcpy(kpts, h->ws.kpt_count + (size_t)frame * K, K * sizeof(int), hipMemcpyDeviceToHost));
    HIP_TRY(h, hipMemcpy(candidates, h->ws.seen + (size_t)frame * (K + L) + K, L * sizeof(int), hipMemcpyDeviceToHost));
    HIP_TRY(h, hipMemcpy(picked, h->ws.sel_count + (size_t)frame * L, L * sizeof(int), hipMemcpyDeviceToHost));
    return LWP_OK;
}

extern "C" int lwp_debug_post_counts(lwp_handle h, int frame, int* peaks18, int* kpts18, int* candidates19, int* picked19) {
    if (!h || !peaks18 || !kpts18 || !candidates19 || !picked19) return fail(h, LWP_ERR_ARG, "null argument");
    if (!h->skel.is_default) return fail(h, LWP_ERR_STATE, "custom skeleton: use lwp_debug_post_counts_ex");
    return lwp_debug_post_counts_ex(h, frame, peaks18, kpts18, candidates19, picked19, 18, 19);
}

extern "C" int lwp_debug_post_generic(lwp_handle h) {
    if (!h) return LWP_ERR_ARG;
    if (h->ws.N > 0) return h->ws.generic;             // the form the handle's current workspace launches
    return (!h->skel.is_default || h->tune.post_generic == 1) ? 1 : 0;
}

extern "C" int lwp_debug_live_resources(int64_t out[4]) {
    if (!out) return fail(nullptr, LWP_ERR_ARG, "out is null");
    const LiveResources& r = live_resources();
    out[0] = r.dev_bytes; out[1] = r.pin_bytes; out[2] = r.events; out[3] = r.streams;
    return LWP_OK;
}

extern "C" int lwp_debug_f32_to_f16(const float* src, uint16_t* dst, int64_t n) {
    if ((!src || !dst) && n > 0) return fail(nullptr, LWP_ERR_ARG, "null argument");
    for (int64_t i = 0; i < n; ++i) dst[i] = f32_to_f16_rne(src[i]);
    return LWP_OK;
}

extern "C" int lwp_debug_layer_variant(lwp_handle h, int idx, char* name, int name_cap) {
    if (!h || idx < 0 || idx >= (int)h->g.layers.size() || !name || name_cap <= 0) return fail(h, LWP_ERR_ARG, "bad argument");
    const std::string& v = h->variants[idx];
    if ((int)v.size() + 1 > name_cap) return fail(h, LWP_ERR_ARG, "name buffer too small");
    std::strcpy(name, v.c_str());
    return LWP_OK;
}

extern "C" int lwp_debug_time_layer(lwp_handle h, int idx, int N, int H, int W, int iters, float* ms_avg) {
    if (!h || !ms_avg || idx < 0 || idx >= (int)h->g.layers.size() || iters <= 0) return fail(h, LWP_ERR_ARG, "bad argument");
    int rc = check_frame_shape(h, N, H, W);
    if (rc) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    rc = ensure_activations(h, N, H, W);
    if (rc) return rc;
    HIP_TRY(h, h->d_in.ensure((size_t)N * 3 * H * W * sizeof(float)));
    const Layer& l = h->g.layers[idx];
    // a fused head pair is timed at its first layer; its second layer has no launch of its own.  A fold mark is not acted
    // on: a dense 3x3 is timed alone
    const std::vector<Layer>& ls = h->g.layers;
    int fh, fw;
    level_dims(H, W, 3, &fh, &fw);
    const int64_t M3 = (int64_t)N * fh * fw;
    const bool pair = idx + 1 < (int)ls.size() && heads_pair_runs(h, l, ls[idx + 1], M3);
    if (idx > 0 && heads_pair_runs(h, ls[idx - 1], l, M3)) { *ms_avg = 0.f; return LWP_OK; }
    auto one = [&]() { return pair ? enqueue_heads_pair(h, l, ls[idx + 1], N, H, W, nullptr) : enqueue_layer(h, l, h->d_in.as<float>(), N, H, W, nullptr); };
    for (int i = 0; i < 3; ++i) { rc = one(); if (rc) return rc; }
    float ms = 0.f;
    rc = time_on_stream(h, iters, one, &ms);
    *ms_avg = ms / (float)iters;
    return rc;
}

extern "C" int lwp_synchronize(lwp_handle h) {
    if (!h) return LWP_ERR_ARG;
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (h->post_stream) HIP_TRY(h, hipStreamSynchronize(h->post_stream));
    return LWP_OK;
}

// ---------------------------------------------------------------------------------------------- measurement
extern "C" int lwp_time_pipeline(lwp_handle h, const float* in_device, int N, int H, int W, int ratio, int demo, int what,
                                 int iters, float* ms_total) {
    if (!h || !in_device || !ms_total || iters <= 0) return fail(h, LWP_ERR_ARG, "bad argument");
    int rc = prepare_poses(h, N, H, W, ratio);
    if (rc) return rc;
    h->last_N = N; h->async_pending = false;
    return time_on_stream(h, iters, [&]() { return enqueue_poses(h, in_device, N, H, W, ratio, demo, what != 0); }, ms_total);
}

// the training kernels alone: ``iters`` back-to-back launches between two events, after one prepare (checks, uploads) and
// without the per-call synchronise or the copy-back of the sums
extern "C" int lwp_time_train_targets(lwp_handle h, const double* kpts, int kpts_mem, const int* n_persons, int N, int Pmax, int H,
                                      int W, int stride, double sigma, double paf_thickness, float* keypoint_maps_device,
                                      float* paf_maps_device, int iters, float* ms_total) {
    if (!ms_total || iters <= 0) return fail(h, LWP_ERR_ARG, "bad argument");
    TrainTargetsParams p{};
    int rc = train_targets_prepare(h, kpts, kpts_mem, n_persons, N, Pmax, H, W, stride, sigma, paf_thickness, keypoint_maps_device,
                                   paf_maps_device, &p);
    if (rc) return rc;
    return time_on_stream(h, iters, [&]() { LAUNCH(h, KC_OTHER, launch_train_targets(p, N, h->stream)); return (int)LWP_OK; }, ms_total);
}

extern "C" int lwp_time_augment_batch(lwp_handle h, const lwp_augment_plan* plans, int N, int crop_h, int crop_w, int stride,
                                      float* image_out, unsigned char* mask_out, float* mask_small_out, int iters, float* ms_total) {
    if (!ms_total || iters <= 0) return fail(h, LWP_ERR_ARG, "bad argument");
    const lwp_augment_plan* d_plans = nullptr;
    int rc = augment_prepare(h, plans, N, crop_h, crop_w, stride, image_out, mask_out, mask_small_out, &d_plans);
    if (rc) return rc;
    return time_on_stream(h, iters, [&]() {
        LAUNCH(h, KC_OTHER, launch_augment(d_plans, N, crop_h, crop_w, stride, image_out, mask_out, mask_small_out, h->stream));
        return (int)LWP_OK; }, ms_total);
}

extern "C" int lwp_time_crowd_masks(lwp_handle h, const int64_t* counts, const int64_t* seg_off, const int64_t* image_seg_off,
                                    const int* heights, const int* widths, int N, const int64_t* out_off, float* masks_device,
                                    int iters, float* ms_total) {
    if (!ms_total || iters <= 0) return fail(h, LWP_ERR_ARG, "bad argument");
    CrowdLaunch c{};
    int rc = crowd_masks_prepare(h, CrowdRuns{counts, seg_off, image_seg_off}, heights, widths, N, out_off, masks_device, &c);
    if (rc) return rc;
    return time_on_stream(h, iters, [&]() { LAUNCH(h, KC_OTHER, launch_crowd_masks(c, h->stream)); return (int)LWP_OK; }, ms_total);
}

extern "C" int lwp_time_stage_losses(lwp_handle h, const float* const* outs, int n_outs, const float* keypoint_maps,
                                     const float* paf_maps, const float* mask, int N, int hs, int ws, int batch_size, int iters,
                                     float* ms_total) {
    if (!ms_total || iters <= 0) return fail(h, LWP_ERR_ARG, "bad argument");
    int rc = stage_losses_prepare(h, outs, n_outs, keypoint_maps, paf_maps, mask, N, hs, ws, batch_size);
    if (rc) return rc;
    return time_on_stream(h, iters, [&]() { return enqueue_stage_losses(h, outs, keypoint_maps, paf_maps, mask, N, hs, ws, batch_size); }, ms_total);
}

extern "C" int lwp_profile_launches(lwp_handle h, const float* in_device, int N, int H, int W, int ratio, int demo, int reps,
                                    float* ms, int* kclass, int cap, int* n_launches) {
    if (!h || !in_device || !ms || !kclass || !n_launches || reps <= 0 || cap <= 0) return fail(h, LWP_ERR_ARG, "bad argument");
    int rc = prepare_poses(h, N, H, W, ratio);
    if (rc) return rc;
    h->last_N = N; h->async_pending = false;
    for (int i = 0; i < cap; ++i) { ms[i] = 0.f; kclass[i] = -1; }
    size_t nl = 0;
    for (int r = 0; r < reps; ++r) {
        h->profiling = true;
        h->record_variants = true;
        h->ev_used = 0;
        rc = enqueue_poses(h, in_device, N, H, W, ratio, demo, true);
        h->profiling = false;
        h->record_variants = false;
        if (rc) return rc;
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        nl = h->ev_used / 2;
        if ((int)nl > cap) return fail(h, LWP_ERR_ARG, "launch arrays too small");
        for (size_t i = 0; i < nl; ++i) {
            float t = 0.f;
            HIP_TRY(h, hipEventElapsedTime(&t, h->ev[2 * i], h->ev[2 * i + 1]));
            ms[i] += t / (float)reps;
            kclass[i] = h->ev_class[i] | ((h->ev_layer[i] + 1) << 8);
        }
    }
    *n_launches = (int)nl;
    return LWP_OK;
}

extern "C" int lwp_profile_classes(lwp_handle h, const float* in_device, int N, int H, int W, int ratio, int demo, int reps,
                                   float* ms, int* launches) {
    if (!h || !in_device || !ms || !launches || reps <= 0) return fail(h, LWP_ERR_ARG, "bad argument");
    int rc = prepare_poses(h, N, H, W, ratio);
    if (rc) return rc;
    h->last_N = N; h->async_pending = false;
    return profile_by_class(h, KC_COUNT, reps, ms, launches, [&]() { return enqueue_poses(h, in_device, N, H, W, ratio, demo, true); });
}
