/*
 * lwpose.h — C ABI of the MI355X-native Lightweight-OpenPose inference path.
 *
 * The reference (vivek87799/lightweight-human-pose-estimation.pytorch) is pure Python and has no
 * FFI/plugin registry; its drop-in boundary is duck typing at a few Python call sites.  This header
 * is what a binding for those call sites talks to (the ctypes stub is in INTEGRATION.md and in
 * lwpose_amd/_lib.py).  Each entry point cites the reference interface it replaces.
 *
 * Conventions
 *   - every function returns int: 0 = LWP_OK, negative = error class; nothing throws across the ABI;
 *     lwp_last_error(h) returns a human-readable message for the last failing call on that handle
 *     (h == NULL: last failure of a call that had no handle).
 *   - plain pointers and sizes only; the caller owns every buffer it passes, the handle owns all
 *     device memory it allocates.  Pointer arguments tagged "mem" accept host or device memory
 *     according to the LWP_MEM_* flag passed with them (device pointers = zero-copy from
 *     torch-ROCm tensors via data_ptr()).
 *   - one handle per (device, stream); a handle is not thread-safe; distinct handles are independent (handles on
 *     different devices may live in one process; the usual deployment is one process per GPU).
 *   - all maps are float32.  Network tensors crossing the ABI are NCHW (as the reference's
 *     nn.Module sees them); post-processing maps are HWC (as numpy sees them after demo.py:71-76).
 */
#ifndef LWPOSE_H
#define LWPOSE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct lwp_context* lwp_handle;

enum {
    LWP_OK = 0,
    LWP_ERR_ARG = -1,       /* bad argument / shape                               */
    LWP_ERR_HIP = -2,       /* HIP runtime error (message has the hipError string) */
    LWP_ERR_STATE = -3,     /* call order (e.g. forward before load_weights)       */
    LWP_ERR_CAPACITY = -4,  /* a peak / key-point / connection list overflowed its configured capacity */
    LWP_ERR_NOGPU = -5,     /* no usable HIP device                                */
    LWP_ERR_UNBOUND = -6,   /* the reference would raise UnboundLocalError here (keypoints.py:116,137) */
    LWP_ERR_INTERNAL = -7   /* two parts of the library that must agree do not (the message names both verdicts) */
};

enum { LWP_MEM_HOST = 0, LWP_MEM_DEVICE = 1 };
enum { LWP_LAYOUT_NCHW = 0, LWP_LAYOUT_NHWC = 1 };
enum { LWP_F32 = 0, LWP_BF16 = 1, LWP_F16 = 2 };   /* storage/MFMA dtype of the conv stack; accumulation, bias, depthwise
                                                       weights, activations and all post-processing are always f32/f64.
                                                       LWP_F16 (IEEE half) is the bf16 graph with 3 more significand bits;
                                                       a folded weight beyond +-65504 fails lwp_load_weights */

/* role codes returned by lwp_param_spec */
enum { LWP_ROLE_CONV_W = 0, LWP_ROLE_CONV_B = 1, LWP_ROLE_BN_W = 2, LWP_ROLE_BN_B = 3,
       LWP_ROLE_BN_MEAN = 4, LWP_ROLE_BN_VAR = 5, LWP_ROLE_BN_NBT = 6 };

int lwp_version(void);

/* ---- parameter table: replaces nn.Module.state_dict() key/shape enumeration
 *      (models/with_mobilenet.py:89-112 + modules/conv.py:4-32; consumed by modules/load_state.py:4-15).
 *      No GPU needed. */
int lwp_param_count(int num_refinement_stages, int num_channels, int num_heatmaps, int num_pafs);
int lwp_param_spec(int num_refinement_stages, int num_channels, int num_heatmaps, int num_pafs,
                   int index, char* name, int name_cap, int64_t shape[4], int* ndim, int* role);

/* ---- lifetime: replaces PoseEstimationWithMobileNet(...) + net.cuda() (demo.py:156, demo.py:82-84) */
int lwp_create(int device_id, int num_refinement_stages, int num_channels, int num_heatmaps,
               int num_pafs, int dtype, lwp_handle* out);
int lwp_destroy(lwp_handle h);
const char* lwp_last_error(lwp_handle h);

/* ---- stream ordering: the reference's net(tensor_img) runs on torch's CURRENT stream (demo.py:64-68), so a caller never
 *      synchronises by hand.  The handle computes on its own non-blocking stream; with lwp_set_stream(h, s, 1) every later
 *      entry point that takes or returns DEVICE memory (a) makes its stream wait — by event, without blocking the host — for
 *      the work queued on `s` so far (the producers of its inputs and the last users of the buffers it overwrites), and (b) makes
 *      `s` wait for the results it leaves on the device.  `caller_stream` is a hipStream_t (NULL = the legacy default stream,
 *      which is torch's default current stream).  enable = 0 restores the initial state: no ordering, the caller synchronises
 *      (lwp_synchronize) around device-memory hand-overs.  enable = 2: (a) only — device results stay on the handle's stream for
 *      its own next call (the frame tensor between lwp_preprocess_u8 and lwp_infer_poses inside infer_fast, demo.py:59-68, never
 *      meets the caller's stream), which saves the cross-queue wait.  An idle caller stream costs nothing in any mode (it is
 *      queried first).  Host-memory results are complete on return in all modes. */
int lwp_set_stream(lwp_handle h, void* caller_stream, int enable);

/* capacities of the post-processing lists (defaults 2048 / 128 / 4096 / 256); overflow => LWP_ERR_CAPACITY.  Refused while a
 * pipeline slot is pending; discards the results of an unfetched lwp_infer_poses_async run (lwp_fetch_poses: LWP_ERR_STATE). */
int lwp_set_capacity(lwp_handle h, int max_peaks_per_channel, int max_kpts_per_type,
                     int max_connections_per_limb, int max_pose_entries);

/* ---- skeleton: the grouping tables of modules/keypoints.py:5-8 (BODY_PARTS_KPT_IDS, BODY_PARTS_PAF_IDS) and group_keypoints'
 *      options (:51), for networks trained on another key-point set (TRAIN-ON-CUSTOM-DATASET.md: num_heatmaps = K + 1,
 *      num_pafs = 2 L).  limb_kpts / limb_pafs: num_limbs x 2 int (key-point types a, b; PAF channels x, y), in grouping order.
 *      limb_kpts == NULL restores the default (COCO tables, 18 types, pose_entry_size 20, min_paf_score 0.05).
 *      Checks (LWP_ERR_ARG with a message): 1 <= K <= 64 and K <= num_heatmaps (only the first K heat-map channels are read,
 *      like range(num_keypoints), demo.py:97); 1 <= L <= 320; 0 <= a, b < K, a != b; PAF ids < num_pafs (the two of a limb may
 *      be equal); K + 2 <= pose_entry_size <= 256.  Deliberate divergence: the reference silently overwrites key-point columns
 *      with the score and count when pose_entry_size < K + 2; this library refuses it.  min_paf_score: any double, used in
 *      the reference's strict float64 '>'.  Host state of the handle (not part of the weight blob); the workspaces are
 *      re-sized by K / L on the next call.  Every pose-producing export below uses the handle's skeleton: in their buffer
 *      shapes 18 / 19 / 20 read K / L / E (pose_entry_size).  The default skeleton runs COCO-specialised kernels; any other
 *      runs generic ones (LWP_POST_GENERIC=1 at lwp_create forces the generic kernels under the default skeleton too).
 *      Refused while a pipeline slot is pending (LWP_ERR_STATE); the results of an lwp_infer_poses_async run not
 *      yet fetched are discarded (lwp_fetch_poses then returns LWP_ERR_STATE), as after lwp_set_capacity.  lwp_get_skeleton: limb arrays of limb_cap rows (or NULL). */
int lwp_set_skeleton(lwp_handle h, int num_kpt_types, int num_limbs, const int* limb_kpts, const int* limb_pafs,
                     int pose_entry_size, double min_paf_score);
int lwp_get_skeleton(lwp_handle h, int* num_kpt_types, int* num_limbs, int* limb_kpts, int* limb_pafs, int limb_cap,
                     int* pose_entry_size, double* min_paf_score);

/* ---- weights: replaces net.load_state_dict(...) at the end of load_state (modules/load_state.py:15).
 *      names[i] = state_dict key, ptrs[i] = host float32 data (int64 for num_batches_tracked, ignored),
 *      shapes = n x 4 (unused dims 1), ndims[i].  Conv weights OIHW.  Every key of lwp_param_spec must
 *      be present with the right shape.  Folds eval-mode BatchNorm (eps 1e-5, modules/conv.py:7) into
 *      the preceding conv, repacks to the kernels' layouts and uploads one blob. */
int lwp_load_weights(lwp_handle h, const char* const* names, const void* const* ptrs,
                     const int64_t* shapes, const int* ndims, int n);

/* packed weight blob, for one-shot replication to other GPUs (RCCL broadcast done by the host side
 * on a device buffer; replaces nn.DataParallel's per-iteration replicate, train.py:74).  An LWP_F16 blob ends in a 16-byte
 * dtype tag; importing a blob of another dtype (or network) fails with LWP_ERR_ARG. */
int lwp_weights_blob_bytes(lwp_handle h, size_t* bytes);
int lwp_weights_blob_export(lwp_handle h, void* dst_device, size_t bytes);
int lwp_weights_blob_import(lwp_handle h, const void* src_device, size_t bytes);

/* ---- network forward: replaces net(tensor_img) (demo.py:68, val.py:94;
 *      PoseEstimationWithMobileNet.forward, models/with_mobilenet.py:114-123).
 *      in: N x 3 x H x W float32 (mem).  outs: 2*(1+nref) pointers (mem, same kind as out_mem) to
 *      N x {num_heatmaps | num_pafs} x h x w float32 in the order [heat0, paf0, heat1, paf1, ...].
 *      Any H, W >= 8: the map size is that of three stride-2 convs, h = ((H-1)/2+1 -> ... ) (the reference pads to
 *      the stride, val.py:36-49, but does not require it).
 *      Runs on the handle's stream and synchronises it before returning when out_mem is host; device outputs are handed
 *      to the caller's stream by an event when lwp_set_stream is in effect (else call lwp_synchronize before reading them).
 *      Any N: the kernels address a tensor with 32-bit byte offsets, so a batch whose tensors would reach 2 GiB (at 368 x 656:
 *      N > 138 in fp32, N > 277 in bf16) is processed in equal chunks inside the call — same results as separate calls.
 *      fp32 results depend on the batch size at the 1e-6 level only: kernels (tile shapes, split-K, the fused head pair up to
 *      4096 pixels) are chosen by problem size, and their summation orders differ. */
int lwp_forward(lwp_handle h, const float* in, int in_mem, int N, int H, int W,
                float* const* outs, int out_mem);

/* ---- frame pre-processing on the device: replaces demo.py:55-64 (scale = net_input_height / H; cv2.resize of the
 *      uint8 frame with fx = fy = scale, INTER_CUBIC; normalize, val.py:30-33; pad_width, val.py:36-49; HWC -> 1x3xHxW
 *      float32).  lwp_preprocess_dims is pure host arithmetic: the scaled size (round half to even of H*scale, W*scale),
 *      the padded size out_h x out_w, pad = [top, left, bottom, right] and scale, exactly as infer_fast returns them.
 *      lwp_preprocess_u8: img is H x W x 3 uint8 (mem), out is a DEVICE buffer of 3*out_h*out_w float32.
 *      pad_value / img_mean: 3 doubles each (the reference's defaults are (0,0,0) and (128,128,128)); img_scale 1/256.
 *      The pad value is written as is (the reference pads AFTER normalising).  Runs on the handle's stream. */
int lwp_preprocess_dims(int H, int W, int net_input_height, int stride, int* scaled_h, int* scaled_w,
                        int* out_h, int* out_w, int* pad, double* scale);
int lwp_preprocess_u8(lwp_handle h, const unsigned char* img, int img_mem, int H, int W, int net_input_height, int stride,
                      const double* pad_value, const double* img_mean, double img_scale, float* out_device);

/* ---- the same for N same-sized frames in one launch: replaces demo.py:55-68's per-frame preparation for a batch of camera
 *      frames (frame f of the batch is lane f of lwp_set_tracking mode 2).  imgs is N x H x W x 3 uint8 (mem), out a DEVICE
 *      buffer of N*3*out_h*out_w float32 (out_h, out_w of lwp_preprocess_dims).  The arithmetic is lwp_preprocess_u8's (integer
 *      resize, exact float64 normalise): every frame gets the bits a single-frame call gives it, N = 1 included.  Host frames go
 *      through the same pinned staging and are free on return; the stream ordering is lwp_preprocess_u8's.  The resize tables of
 *      a geometry are built once, kept on the device (up to 16 geometries) and never rewritten.  Checks (LWP_ERR_ARG with a
 *      message; they need no GPU and run with h == NULL, message via lwp_last_error(NULL)): null pointers, img_mem, 1 <= N <=
 *      65535, an empty scaled frame, negative padding, a padded frame below the network's 8 x 8 minimum. */
int lwp_preprocess_u8_batch(lwp_handle h, const unsigned char* imgs, int img_mem, int N, int H, int W, int net_input_height,
                            int stride, const double* pad_value, const double* img_mean, double img_scale, float* out_device);

/* ---- image side of ONE scale of the multi-scale driver: replaces val.py:84-93 for N same-sized uint8 frames
 *      (normalize, val.py:30-33: float64 (u8 - mean) * scale;  cv2.resize(normed_img, (0,0), fx=fy=ratio, INTER_CUBIC) on
 *      the float64 image: float32 cubic coefficients (A = -0.75), float64 left-to-right sums, horizontal pass then vertical
 *      pass;  pad_width(scaled, stride, pad_value, [base_height, max(scaled_w, base_height)]), val.py:36-49;  HWC -> NCHW
 *      float32, val.py:93).  lwp_scale_dims is pure host arithmetic: scaled size = round-half-even(H*ratio, W*ratio), the
 *      padded size out_h x out_w and pad = [top, left, bottom, right] exactly as pad_width returns them.
 *      lwp_preprocess_scaled_u8: imgs is N x H x W x 3 uint8 (mem), out a DEVICE buffer of N*3*out_h*out_w float32.
 *      Runs on the handle's stream (the resize tables of a geometry are built once and kept on the device). */
int lwp_scale_dims(int H, int W, double ratio, int base_height, int stride, int* scaled_h, int* scaled_w,
                   int* out_h, int* out_w, int* pad);
int lwp_preprocess_scaled_u8(lwp_handle h, const unsigned char* imgs, int img_mem, int N, int H, int W, double ratio,
                             int base_height, int stride, const double* pad_value, const double* img_mean, double img_scale,
                             float* out_device);
/* the same for float32 frames: val.normalize (val.py:30-33) starts with np.array(img, dtype=np.float32), so an image of any
 * other dtype than uint8 is the float32 case after that cast (done by the caller) */
int lwp_preprocess_scaled_f32(lwp_handle h, const float* imgs, int img_mem, int N, int H, int W, double ratio,
                              int base_height, int stride, const double* pad_value, const double* img_mean, double img_scale,
                              float* out_device);

/* ---- bicubic up-sampling: replaces cv2.resize(map, (0,0), fx=r, fy=r, INTER_CUBIC) on float maps
 *      (demo.py:72,76; val.py:98,105).  src: N x C x h x w (mem);  dst: N x (h*r) x (w*r) x C (mem). */
int lwp_upsample(lwp_handle h, const float* src, int src_mem, int N, int C, int hs, int ws, int ratio,
                 float* dst, int dst_mem);

/* ---- one scale of the multi-scale average: replaces val.py:96-101 / 103-108 (x`up_ratio` cubic up-sampling of one
 *      stage output, crop of the padding pad = [top, left, bottom, right], cubic resize to (dst_w, dst_h),
 *      accum = accum + maps / n_scales).  maps: N x C x hs x ws float32 (mem); accum: N x dst_h x dst_w x C float32 HWC (mem);
 *      the N frames share one geometry (same pad, same destination size).  init != 0: accum is taken as zero (the first
 *      scale of val.py:86-87) and need not be initialised by the caller. */
int lwp_multiscale_accumulate(lwp_handle h, const float* maps, int maps_mem, int N, int C, int hs, int ws, int up_ratio,
                              const int* pad, int dst_h, int dst_w, int n_scales, float* accum, int accum_mem, int init);

/* ---- extract_keypoints: replaces modules/keypoints.py:16-48 for one heat-map channel.
 *      heatmap: H x W float32 with row stride `row_stride` and pixel stride `pix_stride` (elements), host.
 *      It is thresholded IN PLACE (values < 0.1 -> 0) like the reference.  Outputs (host, capacity `cap`):
 *      xs, ys (int64), scores (float32) in the reference's order (x ascending, then y).  *count = number
 *      kept after the radius-6 suppression; ids are total_keypoint_num + index (caller side). */
int lwp_extract_keypoints(lwp_handle h, float* heatmap, int H, int W, int64_t row_stride, int64_t pix_stride,
                          int64_t* xs, int64_t* ys, float* scores, int cap, int* count);

/* ---- group_keypoints: replaces modules/keypoints.py:51-201 (with the handle's skeleton: K types, E = pose_entry_size).
 *      kpts: rows (x, y, score, id) float64 concatenated by type; type_counts[K] (18 by default).
 *      pafs: H x W x num_pafs float32 HWC (mem).  demo != 0 -> int() truncation, else round-half-even.
 *      pose_entries: cap_entries x E float64 out (20 by default): ids in columns 0..K-1, -1 up to E-3, score at E-2, count at
 *      E-1; *n_entries out. */
int lwp_group_keypoints(lwp_handle h, const double* kpts, const int* type_counts,
                        const float* pafs, int pafs_mem, int H, int W, int demo,
                        double* pose_entries, int cap_entries, int* n_entries);

/* ---- fused frame pipeline: replaces the body of run_demo's loop up to group_keypoints
 *      (demo.py:93-100: infer_fast -> 18 x extract_keypoints -> group_keypoints) for a batch.
 *      in: N x 3 x H x W float32, already normalised and padded (mem).  The up-sampled maps are never
 *      materialised: peaks and PAF samples are interpolated on the fly with the same arithmetic.
 *      Outputs (host): for frame f, kpt_counts[f*K + t] key-points of type t; kpts rows
 *      (x, y, score, id) float64 at kpts + f*kpt_cap*4; entries at entries + f*entry_cap*E;
 *      n_entries[f].  K / E: the handle's skeleton (18 / 20 by default, lwp_set_skeleton). */
int lwp_infer_poses(lwp_handle h, const float* in, int in_mem, int N, int H, int W,
                    int upsample_ratio, int demo,
                    int* kpt_counts, double* kpts, int kpt_cap,
                    double* entries, int entry_cap, int* n_entries);

/* same post-processing from already computed maps: the low-resolution stage outputs net(x) returns (demo.py:70,74),
 * heat N x num_heatmaps x h x w, paf N x num_pafs x h x w, LWP_LAYOUT_NCHW; or the full-resolution averaged maps of the
 * multi-scale path (val.py:129-134), N x h x w x C, LWP_LAYOUT_NHWC with upsample_ratio = 1.  float32 (mem). */
int lwp_poses_from_maps(lwp_handle h, const float* heat, const float* paf, int mem, int layout, int N, int hs, int ws,
                        int upsample_ratio, int demo,
                        int* kpt_counts, double* kpts, int kpt_cap,
                        double* entries, int entry_cap, int* n_entries);

/* enqueue-only variant for benchmarking / pipelining: same work, results stay on the device until
 * lwp_fetch_poses; does not synchronise.  `in` must be device memory. */
int lwp_infer_poses_async(lwp_handle h, const float* in_device, int N, int H, int W,
                          int upsample_ratio, int demo);
int lwp_fetch_poses(lwp_handle h, int* kpt_counts, double* kpts, int kpt_cap,
                    double* entries, int entry_cap, int* n_entries);

/* ---- pipelined streaming (video): two result slots.  lwp_pipeline_submit enqueues the network of one batch on the
 *      handle's main stream and its post-processing + result copy on a second stream, and returns at once;
 *      lwp_pipeline_fetch(slot) waits for that slot only.  With submit(k) issued before fetch(k-1), the
 *      post-processing and host fetch of batch k-1 overlap the network of batch k (replaces the strictly serial
 *      frame loop of run_demo, demo.py:91-114; results are identical).  A slot must be fetched before it is reused. */
int lwp_pipeline_submit(lwp_handle h, const float* in_device, int N, int H, int W, int upsample_ratio, int demo, int slot);
int lwp_pipeline_fetch(lwp_handle h, int slot, int* kpt_counts, double* kpts, int kpt_cap,
                       double* entries, int entry_cap, int* n_entries);

/* ---- one-call video step: replaces demo.py:55-68 + demo.py:91-118 for a batch of N same-sized uint8 frames (mem).  One call
 *      enqueues, in order: the upload of host frames, lwp_preprocess_u8_batch into an input tensor the handle owns, the
 *      network on the main stream, and grouping + (if on) the pose tail + the result copy on the slot's stream, exactly as
 *      lwp_pipeline_submit splits the work; it returns at once.  Host frames are free for reuse on return; DEVICE frames must
 *      stay untouched until the slot is fetched (like in_device of lwp_pipeline_submit).  Results: lwp_pipeline_fetch(slot),
 *      then lwp_get_poses(slot).  The tail's un-map of THIS submit is (stride, scale, pad_top, pad_left) as lwp_preprocess_dims
 *      yields them for (H, W, net_input_height, stride), with upsample_ratio: it rides in the tail launch by value, so two
 *      slots in flight may hold frames of different sizes, and the handle's lwp_set_unmap state is neither read nor written.
 *      With the tail off the entries and key-points are those of lwp_preprocess_u8 + lwp_pipeline_submit.  lwp_pipeline_submit's
 *      rules hold: a pending slot is LWP_ERR_STATE, a batch whose tensors would reach 2 GiB is walked in equal chunks, the lanes
 *      of tracking modes 2 / 3 belong to the slot's stream while a slot is pending, the capacities and the 256-pose limit of
 *      the tail apply.  A new frame geometry gets its own resize tables (never rewritten while another slot may read them).
 *      The call returns without waiting in the steady state; it WAITS for the main stream (the other slot's network included)
 *      when something has to grow or be built: a larger input tensor, a larger device frame buffer for host frames, and the
 *      17th distinct geometry (the oldest tables are freed); a geometry seen for the first time also costs four small blocking
 *      uploads of its tables.  The argument and slot checks (as lwp_preprocess_u8_batch, with h == NULL too, plus slot in
 *      {0, 1} and upsample_ratio in {4, 8}) come before anything is enqueued; an allocation that fails later (activations,
 *      grouping workspace, tracking state) is still reported after the upload and the pre-processing were enqueued — the slot
 *      is then not pending and nothing of it can be fetched. */
int lwp_pipeline_submit_u8(lwp_handle h, const unsigned char* imgs, int img_mem, int N, int H, int W, int net_input_height,
                           int stride, const double* pad_value, const double* img_mean, double img_scale, int upsample_ratio,
                           int demo, int slot);

/* ---- pose tail on the device: replaces the rest of run_demo's loop body (demo.py:101-118: map the key-points back to image
 *      coordinates, one Pose per entry, modules/pose.py:65-118 track_poses with its 1-Euro smoothing).  OFF by default: with
 *      mode 0 every export launches, computes and returns exactly what it did before.  With mode != 0 two more kernels follow the
 *      grouping kernels of lwp_infer_poses / lwp_infer_poses_async / lwp_poses_from_maps / lwp_pipeline_submit on the same
 *      stream, and their results travel in the same result block; lwp_get_poses reads them on the host after the fetch.
 *      (lwp_group_keypoints has no tail: it returns entries only.)
 *      lwp_set_tracking: mode 0 off, 1 pose rows only (ids -1), 2 lanes (frame f of a batch is the next frame of lane f),
 *      3 sequence (the N frames of a batch are N consecutive frames of lane 0; same results as N batch-1 calls).  A lane holds
 *      the previous frame's poses, their ids and filter states and its own id counter, on the device.  match_threshold:
 *      track_poses' `threshold` (3 in the reference; any int, <= 0 keeps the reference's corner case).  similarity_threshold:
 *      get_similarity's (0.5), must lie inside (0, 1); the kernel decides exp(-q) > t as q < -ln t with -ln t computed here once.
 *      smooth != 0: OneEuroFilter(freq 15, mincutoff 1, beta 0.05, dcutoff 1) per coordinate.  sigmas: K float32 values as
 *      Pose.sigmas holds them (already divided by 10); NULL = the COCO table, an error unless K is 18 (n_sigmas 0 or 18);
 *      otherwise n_sigmas must equal K.  The argument checks need no GPU and run with h == NULL against K = 18 (message via
 *      lwp_last_error(NULL)).  Refused with LWP_ERR_STATE while a pipeline slot is pending.  Every call clears all lanes (ids
 *      start at 0 again) and discards unfetched results; the workspaces are kept unless the tail goes on or off.  While
 *      tracking is on (mode 2 / 3) the serial exports are refused with LWP_ERR_STATE as long as a pipeline slot is pending (the
 *      lanes belong to one stream at a time), and EVERY pose-producing pass advances the lanes, lwp_time_pipeline and
 *      lwp_profile_launches / lwp_profile_classes included (one step per repetition).  A NaN confidence ranks last (as -inf).  lwp_set_skeleton and lwp_set_capacity clear all lanes too;
 *      lwp_set_skeleton with another K turns tracking off (the sigma table belonged to the old K).  The tail holds at most
 *      256 poses per frame: with max_pose_entries above 256 a pose-producing call fails with LWP_ERR_ARG while it is on.
 *      Pose rows: for entry n and type k, -1 if the entry column is -1.0, else (int)((x * stride / upsample_ratio - pad_left) /
 *      scale) (y with pad_top), float64, truncation toward zero (values beyond int32 saturate; Python would raise); confidence =
 *      entry column E - 2 (the reference writes the literal 18, which is E - 2 for its skeleton); poses keep entry order;
 *      bbox = (min_x, min_y, max_x - min_x + 1, max_y - min_y + 1) over key-points with x != -1, (0,0,0,0) if none.
 *      lwp_set_unmap: stride / scale / pad as lwp_preprocess_dims returns them (defaults 8, 1.0, 0, 0); used by the following calls.
 *      lwp_reset_tracking: lane -1 = all lanes (and lanes created later); the lane forgets its poses and gives next_id out first.
 *      lwp_get_poses: slot -1 = the last lwp_infer_poses / lwp_poses_from_maps / lwp_fetch_poses, 0 / 1 = a FETCHED pipeline
 *      slot.  n_poses[N]; keypoints N x pose_cap x K x 2 int32; confidence N x pose_cap float64; bbox N x pose_cap x 4 int32;
 *      ids N x pose_cap int32 (-1 in mode 1); last_ids (may be NULL) [N]: the lane's last given id after that frame (-1 in
 *      mode 1).  LWP_ERR_STATE if the tail was off for that run; LWP_ERR_CAPACITY if pose_cap is below a frame's pose count.
 *      lwp_track_poses: one tracking step of `lane` on poses the caller supplies (n x K x 2 int32 key-points, -1 = missing; n
 *      float64 confidences, which must be finite: LWP_ERR_ARG otherwise), on the same kernels; outputs n x K x 2, n x 4, n, and
 *      the lane's last given id.  Needs mode 2 or 3.  It uses frame 0 of the serial workspace: the results of an
 *      lwp_infer_poses_async run not yet fetched are discarded (lwp_fetch_poses: LWP_ERR_STATE), and lwp_get_poses(-1) has
 *      nothing to return until the next pose-producing call.
 *      near_count (may be NULL), and lwp_debug_tracking_near per frame of a fetched run: similarity decisions whose q lay within
 *      1e-12 (relative) of -ln t, i.e. where the device's compare could differ from NumPy's exp(-q) > t. */
int lwp_set_tracking(lwp_handle h, int mode, int match_threshold, double similarity_threshold, int smooth,
                     const float* sigmas, int n_sigmas);
int lwp_set_unmap(lwp_handle h, int stride, double scale, int pad_top, int pad_left);
int lwp_reset_tracking(lwp_handle h, int lane, int next_id);
int lwp_get_poses(lwp_handle h, int slot, int* n_poses, int* keypoints, double* confidence, int* bbox, int* ids,
                  int* last_ids, int pose_cap);
int lwp_track_poses(lwp_handle h, int lane, int n, const int* keypoints, const double* confidence, int* out_keypoints,
                    int* out_bbox, int* out_ids, int* last_id, unsigned* near_count);
int lwp_debug_tracking_near(lwp_handle h, int slot, unsigned* counts, int cap);

/* ---- pose overlay on the device: replaces demo.py:119-124 (pose.draw(img) per pose, cv2.addWeighted(orig_img, 0.6, img, 0.4, 0),
 *      one cv2.rectangle per pose) for H x W x 3 uint8 frames.  OFF by default: with mode 0 every export enqueues exactly what it
 *      did before.  The arithmetic is integer except the limb parameter, and exact:
 *        painted set  for each pose and each of the first n_draw_limbs limbs (a, b) of the handle's skeleton table (-1: all but the
 *                     last two, BODY_PARTS_KPT_IDS[:-2]): a disc dx*dx + dy*dy <= 9 at every end whose x != -1; if both ends are
 *                     present, steps = max(|bx - ax|, |by - ay|, 1) and for s = 0..steps a disc dx*dx + dy*dy <= 1 at
 *                     (trunc(qx), trunc(qy)), q = a + (b - a) * (s / steps) in float64 — one division, one multiplication, one
 *                     addition, each rounded (no fma), truncation toward zero; clipped to the frame.  This is what the package's
 *                     host rasteriser Pose.draw paints, bit for bit while |coordinate| <= 2^20; beyond that (pose rows saturate at
 *                     int32) the call still neither overflows nor reads or writes out of bounds, and a launch stays O(frame size)
 *                     per limb: only the steps whose stamps can reach the frame are walked.
 *        blend        painted pixel: out = (6 * src + 4 * color + 5) / 10 per channel, integer division (= addWeighted with
 *                     round-to-nearest, for every byte pair); any other pixel: out = src.  out is written from src, never in place.
 *        boxes        (boxes != 0) a one-pixel outline in box_color per pose, after the blend and not blended; corners (x, y) and
 *                     (x + w, y + h) inclusive, clipped; a pose without key-points has box (0,0,0,0) and paints pixel (0,0).
 *      OUT OF SCOPE: the id label (cv2.putText, demo.py:125-127) — there is no Hershey font data to pin it against; the ids are
 *      returned next to the frame (lwp_get_poses).  cv2.circle / cv2.line themselves: the stand-in rasteriser above is the
 *      contract, and it is not pinned against OpenCV (like the resizes).
 *      lwp_set_overlay: mode 0 off, 1 annotated frames kept on the device, 2 additionally copied to pinned host memory with the
 *      slot's results.  color / box_color: 3 bytes in the frame's channel order, NULL = (0, 224, 255) / (0, 255, 0).  The argument
 *      checks need no GPU and run with h == NULL (against 19 limbs).  LWP_ERR_STATE while a pipeline slot is pending.  The
 *      settings other than the mode also apply to lwp_draw_poses.
 *      lwp_pipeline_submit_u8 with mode != 0 (needs lwp_set_tracking mode >= 1, else LWP_ERR_STATE): the overlay kernels follow the
 *      pose tail on the slot's stream and read the frame's pose count, rows (the smoothed ones) and boxes from the slot's result
 *      block on the device.  Host frames are uploaded into a frame buffer the SLOT owns (the shared staging would be overwritten by
 *      the next submit while this slot has yet to read it); device frames are read in place until the fetch, as promised above.
 *      lwp_get_overlay: the N x H x W x 3 annotated frames of a FETCHED slot into dst (mem): device-to-device on the handle's
 *      stream (lwp_set_stream applies), or to host memory from the pinned copy (mode 2; mode 1: a blocking copy).  They stay valid
 *      until that slot is submitted again.  LWP_ERR_STATE if the slot ran without the overlay, LWP_ERR_ARG on another N, H or W.
 *      lwp_draw_poses: the same kernels on poses the caller supplies, the counterpart of lwp_track_poses: imgs N x H x W x 3 (mem),
 *      n_poses[N], keypoints N x pose_cap x K x 2 int32, bbox N x pose_cap x 4 int32 (host, as lwp_get_poses returns them), out
 *      N x H x W x 3 (mem), not overlapping imgs.  Needs no weights, no network and no tail; runs on the handle's stream and
 *      honours lwp_set_stream; complete on return unless out is device memory handed to the caller's stream.  Checks without a GPU
 *      (h == NULL too): null pointers, the mem flags, 1 <= N <= 65535, H, W >= 1, 0 <= n_poses[f] <= pose_cap <= 65535. */
int lwp_set_overlay(lwp_handle h, int mode, const unsigned char* color, const unsigned char* box_color, int boxes, int n_draw_limbs);
int lwp_get_overlay(lwp_handle h, int slot, unsigned char* dst, int dst_mem, int N, int H, int W);
int lwp_draw_poses(lwp_handle h, const unsigned char* imgs, int img_mem, int N, int H, int W, const int* n_poses,
                   const int* keypoints, const int* bbox, int pose_cap, unsigned char* out, int out_mem);

/* ---- training targets and the per-stage masked L2 loss on the device: replaces datasets/coco.py:48-61,71-159 (the mask resize,
 *      _generate_keypoint_maps / _add_gaussian, _generate_paf_maps / _set_paf) and modules/loss.py l2_loss as train.py:92-97
 *      sums it per stage.  Targets and loss only: backward, optimiser and augmentation are the sections below.
 *      lwp_train_targets: kpts is N x Pmax x K x 3 float64 (mem) holding (x, y, visibility) in image pixels, persons in label
 *      order (the main person, then processed_other_annotations); n_persons[N] (host) says how many rows of a frame count.  K, L,
 *      the limbs' key-point pairs and their PAF channel pairs are the handle's skeleton table (lwp_set_skeleton); the default
 *      table writes limb [1, 2] to channels 12 / 13, which is coco.py's BODY_PARTS_KPT_IDS layout.  Outputs (DEVICE, float32):
 *      keypoint_maps N x (K + 1) x h x w (last channel: 1 - max over the K), paf_maps N x 2L x h x w, h = H / stride, w = W / stride
 *      (integer division).  A key-point counts iff visibility <= 1.  The arithmetic is the reference's, in double, statement by
 *      statement (int() truncation, // on the clamped corners, exponent = d2 / 2 / sigma / sigma, cut at 4.6052, the increment
 *      rounded to float32 before a float32 add as NumPy 2 does, clip to 1 after every add; the PAF of the last person in label
 *      order wins a pixel), with two library calls in place of CPython's: exp() is the device's, and ** 0.5 is a correctly
 *      rounded sqrt.  Checks (LWP_ERR_ARG): 1 <= N <= 65535, 0 <= n_persons[f] <= Pmax <= 65535, 1 <= stride <= H, W, sigma > 0,
 *      paf_thickness >= 0, at most 2^28 map cells, PAF channel ids below 2L and each written by one limb only (the kernel
 *      takes the limbs inside a chunk of persons, the reference limb by limb: the orders agree only then), and for host key-points that every value is finite (int() raises in the
 *      reference; device key-points are not read by the host and must be finite).
 *      lwp_mask_downsample: mask N x H x W float32 (mem) -> out N x (H / stride) x (W / stride) float32 (DEVICE), the mean of each
 *      stride x stride block: cv2.resize(mask, fx = fy = 1 / stride, INTER_AREA) (coco.py:48) where the size divides — only
 *      then (LWP_ERR_ARG otherwise; at most 2^28 output cells).  Exact for the 0 / 1 masks get_mask makes; not pinned against cv2 (like the other resizes).
 *      lwp_stage_losses: outs = the n_outs = 2 * (num_refinement_stages + 1) tensors net(x) returned (DEVICE, contiguous NCHW
 *      float32; even entries N x num_heatmaps x hs x ws against keypoint_maps, odd entries N x num_pafs x hs x ws against
 *      paf_maps; a NULL entry is skipped and its loss is 0), mask N x hs x ws (DEVICE) broadcast over the channels.
 *      losses_host[i] = sum(((outs[i] - target) * mask)^2 / 2 / batch_size), every term and every sum in float64, in a fixed
 *      order without atomics: the same inputs give the same bits.  One launch reads the targets once for up to 16 tensors.
 *      LWP_ERR_ARG when n_outs is not 2 * (num_refinement_stages + 1), or when the skeleton's K + 1 / 2L differ from the
 *      network's num_heatmaps / num_pafs.  Complete on return (the sums are host memory).
 *      All three run on the handle's stream and honour lwp_set_stream; none needs weights. */
int lwp_train_targets(lwp_handle h, const double* kpts, int kpts_mem, const int* n_persons, int N, int Pmax, int H, int W,
                      int stride, double sigma, double paf_thickness, float* keypoint_maps_device, float* paf_maps_device);
int lwp_mask_downsample(lwp_handle h, const float* mask, int mem, int N, int H, int W, int stride, float* out_device);
int lwp_stage_losses(lwp_handle h, const float* const* outs, int n_outs, const float* keypoint_maps, const float* paf_maps,
                     const float* mask, int N, int hs, int ws, int batch_size, double* losses_host);
/* ---- the loss log: train.py:78,96-97,112-119's total_losses on the device.  lwp_stage_losses_log takes lwp_stage_losses'
 *      arguments with `divisor` in place of losses_host: it enqueues the same launches on the handle's stream and, in the kernel
 *      that forms the S = 2 * (num_refinement_stages + 1) sums, log[i] += losses[i] / divisor in float64, one thread per entry, in
 *      launch order, without atomics; the call is counted in an add count.  With more than 16 tensors there are two launches and
 *      each adds its own range.  It returns WITHOUT a host wait (the one wait left is that of a growing partials buffer, as in
 *      lwp_stage_losses); under lwp_set_stream the caller's stream is ordered behind the launches, otherwise the caller keeps the
 *      tensors untouched until a call that waits.  The log belongs to the handle and is zero at creation.  Checks: those of
 *      lwp_stage_losses, and divisor finite and > 0 (LWP_ERR_ARG).
 *      lwp_loss_log_read waits for the stream and copies the S sums and the add count; reset != 0 zeroes both behind the copy. */
int lwp_stage_losses_log(lwp_handle h, const float* const* outs, int n_outs, const float* keypoint_maps, const float* paf_maps,
                         const float* mask, int N, int hs, int ws, int batch_size, double divisor);
int lwp_loss_log_read(lwp_handle h, double* sums_host, int64_t* adds, int reset);
/* the kernels of the two calls alone (tools/targets_bench.py): the same arguments and checks, one upload, then `iters`
 * back-to-back launches between two HIP events on the handle's stream, with no per-call synchronise and no copy-back of the
 * sums.  ms_total out. */
int lwp_time_train_targets(lwp_handle h, const double* kpts, int kpts_mem, const int* n_persons, int N, int Pmax, int H, int W,
                           int stride, double sigma, double paf_thickness, float* keypoint_maps_device, float* paf_maps_device,
                           int iters, float* ms_total);
int lwp_time_stage_losses(lwp_handle h, const float* const* outs, int n_outs, const float* keypoint_maps, const float* paf_maps,
                          const float* mask, int N, int hs, int ws, int batch_size, int iters, float* ms_total);

/* ---- stage backward: the gradient of train.py:99-102's summed loss
 *        L = loss_scale * sum_i l2_loss(stages_output[i], target_i, mask, batch_size)      (modules/loss.py: sum(((out - target) * mask)^2) / 2 / batch_size)
 *      with respect to every parameter of initial_stage.* and refinement_stages.* (with_mobilenet.py:25-86) and to
 *      backbone_features, the output of cpm.conv (with_mobilenet.py:117).  fp32 handles only; the backbone is frozen, the cpm
 *      too unless the train scope is LWP_TRAIN_CPM; LWP_TRAIN_ALL trains both (lwp_set_train_scope below),
 *      and the refinement trunks' BatchNorms (modules/conv.py:8) stay at their running statistics: the result is what
 *      loss.backward() gives on the reference network in eval() mode, NOT in train() mode (no batch statistics, running_mean /
 *      running_var / num_batches_tracked get no gradient and are not updated).  The optimiser step is lwp_stage_adam_step below.
 *      lwp_train_forward: with_mobilenet.py:114-123 on in_device (N x 3 x H x W float32, DEVICE) into outs_device[2 * (nref + 1)]
 *      (DEVICE, NCHW float32) with the kernels, weights and reduction order of lwp_forward — the outputs are bit-identical —
 *      while from cpm.conv's output onward every layer's output is kept in a buffer of its own (each refinement stage has its
 *      own [features | heat | paf] concat input).  Where lwp_forward runs a stage's head pair as one kernel, the pair's hidden
 *      tensor is computed once more by the plain 1x1 kernel for the retained copy.  N must fit one pass (lwp_debug_frames_per_pass).
 *      lwp_stage_backward: keypoint_maps N x num_heatmaps x hs x ws, paf_maps N x num_pafs x hs x ws, mask N x hs x ws (DEVICE,
 *      as lwp_stage_losses takes them).  d out_i = loss_scale * (out_i - target_i) * mask^2 / batch_size (loss_scale carries
 *      train.py:102's 1 / batches_per_iter).  grads_device: ONE float32 DEVICE array of lwp_stage_grad_count's total; the
 *      gradient of parameter `key` sits at lwp_stage_grad_spec's offset with lwp_param_spec's shape (OIHW weights, biases, BN
 *      weight and BN bias), parameters in lwp_param_spec order.  accumulate != 0 adds to the array (train.py:96's
 *      batches_per_iter), else it is overwritten.  d_features_device: NULL, or N x num_channels x hs x ws NCHW (DEVICE),
 *      always overwritten.  All sums run in a fixed order without floating-point atomics: the same inputs give the same bits.
 *      LWP_ERR_ARG with a message: no lwp_train_forward of the same N, hs, ws precedes the call; a bf16 / fp16 handle; no
 *      weights loaded through lwp_load_weights (a weight blob has no raw parameters); the skeleton's K + 1 / 2L differ from
 *      num_heatmaps / num_pafs (as in lwp_stage_losses); batch_size < 1.
 *      Both run on the handle's stream and honour lwp_set_stream. */
int lwp_train_forward(lwp_handle h, const float* in_device, int N, int H, int W, float* const* outs_device);
int lwp_stage_backward(lwp_handle h, const float* keypoint_maps, const float* paf_maps, const float* mask, int N, int hs, int ws,
                       int batch_size, double loss_scale, int accumulate, float* grads_device, float* d_features_device);
/* layout of the gradient array: lwp_stage_grad_count returns the number of parameters with a gradient (total_floats out, may be
 * NULL); lwp_stage_grad_spec the state-dict key, shape and float offset of entry `index`.  No handle, no GPU. */
int lwp_stage_grad_count(int num_refinement_stages, int num_channels, int num_heatmaps, int num_pafs, int64_t* total_floats);
int lwp_stage_grad_spec(int num_refinement_stages, int num_channels, int num_heatmaps, int num_pafs, int index, char* name,
                        int name_cap, int64_t shape[4], int* ndim, int64_t* offset);
/* one backward per rep between HIP events around each launch (tools/backward_bench.py): ms[4], launches[4] by class:
 * 0 = loss gradient / ReLU masks / sums, 1 = data gradient, 2 = weight gradient, 3 = partial-sum reduction and BatchNorm chain rule */
int lwp_profile_stage_backward(lwp_handle h, const float* keypoint_maps, const float* paf_maps, const float* mask, int N, int hs, int ws,
                               int batch_size, double loss_scale, float* grads_device, float* d_features_device, int reps,
                               float* ms, int* launches);
/* tests: the output the last lwp_train_forward retained for layer `layer_index` (cpm.conv or a stage layer of lwp_layer_info's
 * list; a refinement block's last conv holds relu(z) + residual, as the forward kernel writes it) as NCHW float32 in dst (HOST);
 * and the number of pixel ranges the weight gradient of that layer was split into by the last lwp_stage_backward */
int lwp_debug_train_activation(lwp_handle h, int layer_index, float* dst, size_t dst_floats, int out_dims[4]);
int lwp_debug_backward_splits(lwp_handle h, int layer_index);

/* ---- train scope: which parameters lwp_train_forward retains for, lwp_stage_backward / lwp_train_backward differentiate and
 *      lwp_stage_adam_step updates.  LWP_TRAIN_STAGES (the default): initial_stage.* and refinement_stages.*, everything in
 *      front of cpm.conv's output frozen.  LWP_TRAIN_CPM: the cpm (with_mobilenet.py:7-21) as well: cpm.align, the three
 *      depthwise 3x3 + ELU / 1x1 + ELU trunk blocks and cpm.conv; the backbone stays frozen.  The cpm has no BatchNorm.
 *      lwp_set_train_scope: LWP_ERR_ARG on a bf16 / fp16 handle or an unknown scope; LWP_ERR_STATE while a pipeline slot or
 *      an lwp_infer_poses_async is pending, and while the Adam step count is above 0: the moments are laid out for the scope
 *      they were taken in, so call lwp_stage_adam_reset first, or set the scope before the first step.  The call
 *      invalidates the retained forward, as a step does, and releases the retaining plan's buffers and the optimiser state.
 *      In scope LWP_TRAIN_CPM:
 *      - the gradient array, lwp_stage_params_get and lwp_stage_adam_state_get / _set use lwp_train_grad_spec(LWP_TRAIN_CPM, ..)'s
 *        layout: the ten cpm.* parameters in lwp_param_spec order (cpm.align.0.weight / .bias, cpm.trunk.{0,1,2}.0.weight of
 *        shape (C, 1, 3, 3) and cpm.trunk.{0,1,2}.2.weight, cpm.conv.0.weight / .bias), then the stage layout as its unchanged
 *        tail, shifted by the cpm total.  With LWP_TRAIN_STAGES the three lwp_train_* layout functions return exactly what
 *        lwp_stage_grad_count / _spec / lwp_stage_adam_group return.  Parameter groups of the cpm (train.py:46-48): conv
 *        weights with groups == 1 x1 with weight decay, conv biases x2 without, depthwise weights x1 without.
 *      - lwp_train_forward keeps, each in a buffer of its own, the cpm's input (the backbone's last output), a = align(x),
 *        every trunk block's depthwise output after ELU and pointwise output after ELU, and the sum a + trunk(a).  The forward
 *        kernels, their variants and the blob are lwp_forward's, the stage outputs stay bit-identical.  Where the graph runs a
 *        trunk block as one fused launch, the depthwise activation comes from one more stand-alone depthwise launch on the same
 *        input (it may differ from the value inside the fused kernel in the last bit), and the last block's pointwise output in
 *        front of the residual add from one more launch of the block without the residual.
 *      - lwp_train_backward is lwp_stage_backward with one more optional output: d_backbone_device, NULL or N x 512 x hs x ws
 *        NCHW (DEVICE), the gradient at the cpm's input, computed only when asked for (cpm.align's data gradient is 512 wide).
 *        A non-NULL d_backbone_device in scope LWP_TRAIN_STAGES is LWP_ERR_ARG with a message.  lwp_stage_backward follows the
 *        handle's scope for the gradient layout; d_features_device keeps its meaning, and the stage gradients and d_features
 *        are bit-identical to those of scope LWP_TRAIN_STAGES.  New kernels: ELU gradient from the retained output
 *        (dZ = dY * (y > 0 ? 1 : y + 1)), depthwise data gradient (one fmaf chain per output in tap order), depthwise weight
 *        gradient (per-range partial sums in a fixed order, then a reduction in range order): no floating-point atomics.
 *      - lwp_stage_adam_step also updates the cpm parameters and repacks the cpm layers into the blob bit for bit as
 *        lwp_load_weights does.
 *      - tests: lwp_debug_train_activation answers from the backbone's last layer on.  lwp_debug_train_copy is the same read-out
 *        with the kind of retained tensor spelled out: LWP_KEPT_OUTPUT the layer's output (what lwp_debug_train_activation
 *        returns), LWP_KEPT_DEPTHWISE the retained depthwise copy of a fused trunk block (cin channels), LWP_KEPT_NO_RESIDUAL
 *        the retained output of a block in front of its residual add; LWP_ERR_ARG where the layer has no such copy.
 *        lwp_debug_backward_dw_splits is the number of pixel ranges of the layer's depthwise weight gradient (a depthwise
 *        layer or a fused block), lwp_debug_backward_splits that of its dense / pointwise one.
 *      LWP_TRAIN_ALL: the backbone model.* (with_mobilenet.py:92-105) as well, so every parameter train.py:41-55 hands to its
 *      optimiser.  The rules are LWP_TRAIN_CPM's; what differs:
 *      - layout: the 69 model.* parameters first, in lwp_param_spec order (model.0.0.weight, model.0.1.weight / .bias; for
 *        i = 1..11 model.i.0.weight of shape (cin, 1, 3, 3), model.i.1.weight / .bias, model.i.3.weight, model.i.4.weight / .bias),
 *        then the LWP_TRAIN_CPM layout as the unchanged tail, shifted by the backbone total.  Running mean, variance and
 *        num_batches_tracked are not parameters and never move.  Groups (train.py:42-45): conv weights with groups == 1 (stem
 *        and pointwise) x1 with weight decay, depthwise weights x1 without, BatchNorm weights x1 without, BatchNorm biases x2
 *        without.
 *      - lwp_train_forward keeps every backbone layer's output in a buffer of its own (and a copy of the image, which the stem's
 *        weight gradient reads); a fused depthwise + pointwise backbone block gets its depthwise activation (after BatchNorm and
 *        ReLU) from one more stand-alone depthwise launch, with the same last-bit caveat.  The stage outputs stay bit-identical
 *        to lwp_forward's.  lwp_debug_train_activation answers from model.0 on, lwp_debug_train_copy(.., LWP_KEPT_DEPTHWISE, ..)
 *        names a fused backbone block's copy.  None of this is allocated in the other scopes.
 *      - lwp_train_backward covers the backbone: BatchNorm at its running statistics (eval mode), ReLU masks from the retained
 *        outputs, depthwise gradients at stride 1 | 2 and dilation 1 | 2, the stem's weight gradient.  d_backbone_device keeps
 *        its meaning (the gradient at the cpm's input, which this scope always computes).  No gradient at the image.
 *      - lwp_stage_adam_step also updates model.* and refolds BatchNorm into the stem, depthwise, fused and pointwise forms of
 *        the blob bit for bit as lwp_load_weights does. */
enum { LWP_TRAIN_STAGES = 0, LWP_TRAIN_CPM = 1, LWP_TRAIN_ALL = 2 };
enum { LWP_KEPT_OUTPUT = 0, LWP_KEPT_DEPTHWISE = 1, LWP_KEPT_NO_RESIDUAL = 2 };
int lwp_debug_train_copy(lwp_handle h, int layer_index, int which, float* dst, size_t dst_floats, int out_dims[4]);
int lwp_debug_backward_dw_splits(lwp_handle h, int layer_index);
/* tests: the backbone's gradient kernels alone, on the handle's stream, synchronous.  All arrays DEVICE float32.
 * lwp_debug_dw_grad_sd: depthwise 3x3, stride 1 | 2, dilation 1 | 2, padding = dilation.  dz N x Ho x Wo x C (NHWC, Ho = (H - 1) /
 * stride + 1), x N x H x W x C, w [9][C]; out: dx N x H x W x C, G (C, 1, 3, 3), g (C) the per-channel sum of dz; C a multiple of 4.
 * max_chunk > 0 caps the pixels of a range (a multiple of 16), so that small maps take several ranges; *splits: ranges taken.
 * lwp_debug_stem_wgrad: the stem's weight gradient.  dz N x Ho x Wo x 32 (NHWC), x N x 3 x H x W (NCHW); out: G (32, 3, 3, 3),
 * g (32) the column sums of dz. */
int lwp_debug_dw_grad_sd(lwp_handle h, const float* dz, const float* x, const float* w, int N, int H, int W, int C, int stride, int dil,
                         int max_chunk, float* dx, float* G, float* g, int* splits);
int lwp_debug_stem_wgrad(lwp_handle h, const float* dz, const float* x, int N, int H, int W, int max_chunk, float* G, float* g, int* splits);
/* tests: the stage and cpm gradient kernels alone, on the handle's stream, synchronous.  All arrays DEVICE float32 unless said
 * otherwise.  A call that breaks a rule below returns LWP_ERR_ARG and launches nothing.
 * lwp_debug_conv_grad: a dense conv (ks 1 | 3, dil 1 | 2, padding = dil * (ks / 2), stride 1): weight gradient, its fixed-order
 *   reduction and data gradient.  dz (N H W rows of cout channels) and x (rows of cin channels) are NHWC windows: pointer, row
 *   stride and channel offset, offset + channels <= row stride.  w is the raw OIHW weight (cout, cin, ks, ks); the call packs it
 *   to the data gradient's [taps][cout_pad][cin_pad], zero-filled: LWP_PAD_GRAPH pads cout to a multiple of 64 and cin to a
 *   multiple of 32 (the fp32 blob's form), LWP_PAD_RAW leaves both (a fused block's folded matrix) and needs cout a multiple
 *   of 16 and cin a multiple of 4.  max_chunk > 0 caps the pixels of a range (a multiple of 16).  Channels >= acc_from (0..cin) of
 *   the dx window are added to, the others overwritten.  no_bias: db is not touched.  accumulate: dw (OIHW) and db are added to.
 *   *splits: pixel ranges taken.  Test sizes only: N H W < 2^24, cout and cin <= 4096.
 * lwp_debug_dw_grad: the cpm's depthwise 3x3 (stride 1, dilation 1, pad 1).  dz, x and dx are N H W rows of C channels at row strides
 *   that are multiples of 4, 16-byte aligned; w [9][C]; dw (C, 1, 3, 3).  beta: dx is added to.  accumulate: dw is added to.
 * lwp_debug_loss_grad: dst[s] = scale (outs[s] - target) mask^2 for S <= 16 NHWC windows of one row stride ld (outs and dst are
 *   HOST arrays of device pointers; even s: CH channels against keypoint_maps, odd s: CP against paf_maps, both NCHW; mask N x hw).
 * lwp_debug_relu_mask: g = y > res ? g : 0 over M rows of C channels (res NULL: y > 0).  lwp_debug_grad_add: dst = (beta ? dst : 0)
 *   + src.  lwp_debug_elu_grad: g *= y > 0 ? 1 : y + 1 (C and the row strides multiples of 4, pointers 16-byte aligned).
 * lwp_debug_pw_fold: out[o][ci] = float(double(w[o][ci]) * (gamma[o] / sqrt(double(var[o]) + 1e-5))).
 * lwp_debug_bn_chain: gradients G (cout, K) and g (cout) of a folded conv -> dW, db (NULL: none), dgamma, dbeta of the raw
 *   parameters; accumulate: all four are added to. */
enum { LWP_PAD_GRAPH = 0, LWP_PAD_RAW = 1 };
int lwp_debug_conv_grad(lwp_handle h, const float* dz, int dz_ld, int dz_off, const float* x, int x_ld, int x_off, const float* w, int N,
                        int H, int W, int cout, int cin, int ks, int dil, int pad_mode, int max_chunk, int acc_from, int no_bias,
                        int accumulate, float* dx, int dx_ld, int dx_off, float* dw, float* db, int* splits);
int lwp_debug_dw_grad(lwp_handle h, const float* dz, int dz_ld, const float* x, int x_ld, const float* w, int N, int H, int W, int C, int beta,
                      int accumulate, int max_chunk, float* dx, int dx_ld, float* dw, int* splits);
int lwp_debug_loss_grad(lwp_handle h, const float* const* outs, float* const* dst, int S, int ld, const float* keypoint_maps,
                        const float* paf_maps, const float* mask, int N, int CH, int CP, int hw, float scale);
int lwp_debug_relu_mask(lwp_handle h, float* g, int g_ld, const float* y, int y_ld, const float* res, int res_ld, int64_t M, int C);
int lwp_debug_grad_add(lwp_handle h, float* dst, int dst_ld, const float* src, int src_ld, int64_t M, int C, int beta);
int lwp_debug_elu_grad(lwp_handle h, float* g, int g_ld, const float* y, int y_ld, int64_t M, int C);
int lwp_debug_pw_fold(lwp_handle h, const float* w, const float* gamma, const float* var, float* out, int cout, int cin);
int lwp_debug_bn_chain(lwp_handle h, const float* G, const float* g, const float* W, const float* b, const float* gamma, const float* mean,
                       const float* var, float* dW, float* db, float* dgamma, float* dbeta, int cout, int K, int accumulate);
int lwp_set_train_scope(lwp_handle h, int scope);
int lwp_train_grad_count(int scope, int num_refinement_stages, int num_channels, int num_heatmaps, int num_pafs, int64_t* total_floats);
int lwp_train_grad_spec(int scope, int num_refinement_stages, int num_channels, int num_heatmaps, int num_pafs, int index, char* name,
                        int name_cap, int64_t shape[4], int* ndim, int64_t* offset);
int lwp_train_adam_group(int scope, int num_refinement_stages, int num_channels, int num_heatmaps, int num_pafs, int index, int* lr_mult,
                         int* weight_decay_on);
int lwp_train_backward(lwp_handle h, const float* keypoint_maps, const float* paf_maps, const float* mask, int N, int hs, int ws,
                       int batch_size, double loss_scale, int accumulate, float* grads_device, float* d_features_device,
                       float* d_backbone_device);

/* ---- backward precision: the operand type of the two matrix products of the dense-conv gradients (data gradient and weight
 *      gradient of every 1x1 / 3x3 conv: stage convs, the cpm's 1x1s, the backbone's folded pointwise matrices).  LWP_F32 (the
 *      default) runs v_mfma_f32_16x16x4_f32 and gives the bits it always gave.  LWP_BF16 / LWP_F16 run
 *      v_mfma_f32_16x16x32_{bf16,f16} on the SAME f32 arrays: the handle stays fp32, and so do the forward, the retained
 *      activations, every gradient buffer, the parameters and the optimiser.  There is no 16-bit copy of anything in memory, so
 *      nothing can go stale: a backward after lwp_stage_adam_step or lwp_load_weights reads the new weights.
 *      Rounding points: each operand element is converted once, f32 -> 16 bits, round to nearest even, fp16 subnormals kept, while
 *      it is staged into LDS: dZ after its multiplication by grad_scale, the retained input x, and the folded weight (the blob's
 *      [tap][cout_pad][cin_pad] copy or the folded pointwise matrix).  Products are exact and are accumulated in f32; the
 *      accumulator is multiplied by 1 / grad_scale before it is stored or added.  (LWP_F16: subnormal operands reach the MFMA
 *      as normal numbers times 2^-10, in products of their own, because the instruction would add them with fewer bits.)
 *      grad_scale is a power of two in [1, 2^24], so
 *      both multiplications are exact; with LWP_F32 it must be 1.
 *      What stays f32 and bit-identical to LWP_F32 mode for the same inputs: the pixel ranges (lwp_debug_backward_splits), the
 *      partial-sum layout and the fixed-order reduction, the bias column sums (an f32 sum of the unrounded, unscaled dZ), the
 *      accumulate / overwrite rules, the launch order; and every other kernel: depthwise gradients, the stem's weight gradient,
 *      the element-wise kernels, the BatchNorm chain rule, the pointwise fold, the loss gradient.  No floating-point atomics:
 *      the same inputs give the same bits.
 *      A value whose scaled magnitude passes the format's largest number (65504 for LWP_F16) becomes infinite, as the IEEE
 *      conversion does, and such infinities (or the NaNs they breed) reach the gradient array; a scaled value below the
 *      format's smallest subnormal becomes zero.  Choosing or adapting grad_scale (dynamic loss scaling) is the caller's.
 *      Out of scope: a 16-bit forward in training, a 16-bit optimiser, dynamic loss scaling.
 *      The setting may change between any two calls and changes no layout.  It is honoured by lwp_stage_backward,
 *      lwp_train_backward (all three scopes), lwp_profile_stage_backward and lwp_debug_conv_grad.
 *      LWP_ERR_ARG with a message: a bf16 / fp16 handle, an unknown dtype, a grad_scale that is no power of two or outside
 *      [1, 2^24], LWP_F32 with a grad_scale other than 1.  A refused call leaves the setting as it was. */
int lwp_set_backward_precision(lwp_handle h, int dtype, double grad_scale);
int lwp_get_backward_precision(lwp_handle h, int* dtype, double* grad_scale);

/* ---- stage fine-tuning step: the reference's optimiser (train.py:41-55 and :106, torch.optim.Adam with its parameter groups)
 *      for the parameters lwp_stage_backward differentiates, and the refold / repack of the changed layers into the forward's
 *      weight blob, all on the handle's stream: train_forward -> stage_backward -> step lowers the loss with no host round
 *      trip and no second copy of the weights.  fp32 handles whose weights came through lwp_load_weights only.
 *      Out of scope: BatchNorm train mode (the running statistics never move), a 16-bit forward in training, a
 *      16-bit optimiser, dynamic loss scaling, multi-GPU gradient reduction, amsgrad, loading torch's optimiser checkpoints.
 *      lwp_stage_adam_group: the parameter group of gradient-spec entry `index` (no handle, no GPU): learning-rate multiplier
 *      and weight-decay flag: initial_stage conv weight x1 / on, conv bias x2 / off; refinement_stages conv weight x4 / on,
 *      conv bias x8 / off, BatchNorm weight x1 / off, BatchNorm bias x2 / off.
 *      lwp_stage_adam_step: one step from grads_device (DEVICE, lwp_stage_grad_spec's layout).  The state (exp_avg, exp_avg_sq,
 *      zero) is allocated on first use; the step count t goes up by one.  Per element, in float64 with ONE rounding to float32
 *      at each of the three stores, in the order of torch's single-tensor Adam:
 *        g' = g + weight_decay p (groups with decay);  m += (g' - m)(1 - beta1);  v = beta2 v + (1 - beta2) g' g';
 *        denom = sqrt(v) / sqrt(1 - beta2^t) + eps;  p -= (lr_mult base_lr / (1 - beta1^t)) m / denom
 *      (the bias corrections and learning rates are host doubles).  Then every stage layer is folded and packed on the device
 *      exactly as lwp_load_weights packs it on the host: the blob afterwards has the very bits lwp_load_weights gives for the
 *      new raw values, and the handle is as if that had been called; a later lwp_forward needs no synchronise in between to
 *      see the new weights, and lwp_weights_blob_export / lwp_weights_blob_import / lwp_load_weights wait for the handle's
 *      stream before they copy, so they are ordered behind a queued step as well.  No floating-point atomics: the same inputs give the same bits.  The retained lwp_train_forward is
 *      invalidated (lwp_stage_backward then reports that no retaining forward precedes it).
 *      LWP_ERR_ARG with a message: a bf16 / fp16 handle; no raw parameters (weights not loaded, or imported as a blob); base_lr
 *      not finite or not positive; a beta outside [0, 1); eps or weight_decay negative or not finite.  LWP_ERR_STATE while a
 *      pipeline slot or an lwp_infer_poses_async is pending.
 *      lwp_stage_params_get: the current raw stage parameters into flat_device (DEVICE) in the gradient-spec layout.
 *      lwp_stage_adam_state_get / _set: exp_avg, exp_avg_sq (DEVICE, gradient-spec layout) and the step count, for checkpoints
 *      (before the first step: zeros and 0).  lwp_stage_adam_reset discards the state (zeros, step 0).
 *      lwp_time_stage_adam_step: `iters` back-to-back launches of each kernel alone between HIP events, ms[0] the Adam kernel,
 *      ms[1] the repack (totals, milliseconds), on scratch copies: the handle's weights and state do not move. */
int lwp_stage_adam_group(int num_refinement_stages, int num_channels, int num_heatmaps, int num_pafs, int index, int* lr_mult,
                         int* weight_decay_on);
int lwp_stage_adam_step(lwp_handle h, const float* grads_device, double base_lr, double beta1, double beta2, double eps,
                        double weight_decay);
int lwp_stage_params_get(lwp_handle h, float* flat_device);
int lwp_stage_adam_state_get(lwp_handle h, float* exp_avg_device, float* exp_avg_sq_device, int64_t* step);
int lwp_stage_adam_state_set(lwp_handle h, const float* exp_avg_device, const float* exp_avg_sq_device, int64_t step);
int lwp_stage_adam_reset(lwp_handle h);
int lwp_time_stage_adam_step(lwp_handle h, const float* grads_device, double base_lr, double beta1, double beta2, double eps,
                             double weight_decay, int iters, float* ms);

/* ---- training augmentation on the device: the pixel half of datasets/transformations.py (Scale -> Rotate -> CropPad -> Flip,
 *      train.py:33-38) and of coco.py:48,63-65, for a whole batch in one kernel launch.  The host half (the random draws, the
 *      label arithmetic, the geometry below) is lwpose_amd.datasets.transformations.plan_batch; this call renders only the
 *      pixels of the final crop, each straight from the source image: the warped-image pixel behind a crop pixel gives four
 *      fixed-point taps in the resized image, and each tap is evaluated on demand from four source pixels.  No intermediate
 *      image exists, and the result equals the staged resize -> warpAffine -> crop -> flip integer for integer.  The arithmetic
 *      restates OpenCV's plain C path and is not pinned against cv2.
 *      One record per sample:
 *        image / mask   src_h x src_w x 3 uint8 (interleaved) and src_h x src_w float32 with values in [0, 1] (not checked), both
 *                       in `mem` memory; mask == NULL means all ones (the mask taps are skipped, the result is 1 everywhere).
 *                       Host sources of a batch are packed and uploaded with ONE copy; device sources are read in place.
 *        rs_h, rs_w, rs_scale, area   cv2.resize(dsize = (0, 0), fx = fy = s): the rounded size, 1 / s, and 1 where OpenCV takes the
 *                       2 x 2 area average instead (|1 / s - 2| < DBL_EPSILON)
 *        m[6]           the INVERTED 2 x 3 matrix warpAffine walks (destination -> source), bound_h x bound_w its destination size
 *        should_crop, dst_*, img_*   CropPad's slice assignment resolved: crop rows dst_y0..dst_y1-1 and columns dst_x0..dst_x1-1
 *                       show warped pixel (img_y0 + y - dst_y0, img_x0 + x - dst_x0).  Everything else is crop_pad, mask 1.
 *        flip           1: the crop is mirrored (cv2.flip(.., 1))
 *        warp_pad, crop_pad   warpAffine's borderValue and CropPad's fill
 *      Outputs (DEVICE): image_out N x 3 x crop_h x crop_w float32 = (float(v) - 128) / 256; mask_out N x crop_h x crop_w uint8
 *      (the float mask TRUNCATED, as the reference's uint8 cropped_mask does: only 1.0 survives); mask_small_out
 *      N x (crop_h / stride) x (crop_w / stride) float32 = rint(float(block sum) * float(1 / stride^2)), INTER_AREA on a uint8
 *      image (lwp_mask_downsample, the float mean, is a different rule and is unchanged).
 *      Checks without a GPU (h == NULL too, LWP_ERR_ARG): null pointers, 1 <= N <= 65535, 1 <= stride <= 1024, crop_h and crop_w
 *      multiples of the stride, every size (source, resized, bound, crop) in 1..32767 (OpenCV saturates coordinates to short at
 *      32768), a non-NULL image, the mem flag, finite rs_scale > 0 and matrix, the dst rectangle inside the crop and
 *      its source inside the bound.  Runs on the handle's stream, honours lwp_set_stream, needs no weights. */
typedef struct lwp_augment_plan {
    const unsigned char* image;
    const float* mask;
    double rs_scale;
    double m[6];
    int mem;
    int src_h, src_w;
    int rs_h, rs_w, area;
    int bound_h, bound_w;
    int should_crop;
    int dst_y0, dst_y1, dst_x0, dst_x1;
    int img_y0, img_x0;
    int flip;
    unsigned char warp_pad[3], crop_pad[3];
} lwp_augment_plan;
int lwp_augment_batch(lwp_handle h, const lwp_augment_plan* plans, int N, int crop_h, int crop_w, int stride, float* image_out,
                      unsigned char* mask_out, float* mask_small_out);
/* the two kernels alone (tools/augment_bench.py): the same checks and the one upload, then `iters` back-to-back launch pairs
 * between two HIP events.  ms_total out. */
int lwp_time_augment_batch(lwp_handle h, const lwp_augment_plan* plans, int N, int crop_h, int crop_w, int stride, float* image_out,
                           unsigned char* mask_out, float* mask_small_out, int iters, float* ms_total);

/* ---- crowd masks on the device: datasets/coco.py:17-21 (get_mask) for a batch, from the uncompressed RLE dicts
 *      {"counts": [c0, c1, ..], "size": [h, w]} that scripts/prepare_train_labels.py collects from iscrowd annotations.  The runs
 *      alternate between zeros and ones, start with zeros and walk the image column by column: pixel (y, x) is position
 *      x * h + y.  A zero-length run is legal anywhere; positions past the last run are zeros.  The arithmetic restates
 *      maskApi.c's rleDecode and is not pinned against pycocotools.
 *      Inputs (HOST), CSR: image n of N owns segmentations image_seg_off[n] .. image_seg_off[n + 1] - 1, segmentation s the counts
 *      counts[seg_off[s]] .. counts[seg_off[s + 1] - 1]; heights / widths [N].  The host turns the counts into run ends and
 *      uploads [run ends | segment offsets | image records] with ONE copy; one kernel launch renders every image.
 *      Output (DEVICE): image n's heights[n] x widths[n] row-major float32 mask at masks_device + out_off[n] (out_off [N + 1],
 *      in floats): 1.0f where no segmentation of the image covers the pixel, 0.0f where any does.  An image without
 *      segmentations is all ones.
 *      Checks without a GPU (h == NULL too, LWP_ERR_ARG, each naming the sample): null pointers (counts may be NULL when there is
 *      no count), 1 <= N <= 65535, offsets that start at 0 and never descend, sizes in 1..32767, no negative count, the counts of
 *      a segmentation summing to at most height * width (in 64 bits), out_off leaving height * width floats an image.
 *      Runs on the handle's stream, honours lwp_set_stream, needs no weights. */
int lwp_crowd_masks(lwp_handle h, const int64_t* counts, const int64_t* seg_off, const int64_t* image_seg_off, const int* heights,
                    const int* widths, int N, const int64_t* out_off, float* masks_device);
/* the kernel alone (tools/crowd_mask_bench.py): the same checks and the one upload, then `iters` back-to-back launches between
 * two HIP events.  ms_total out. */
int lwp_time_crowd_masks(lwp_handle h, const int64_t* counts, const int64_t* seg_off, const int64_t* image_seg_off,
                         const int* heights, const int* widths, int N, const int64_t* out_off, float* masks_device, int iters,
                         float* ms_total);
/* lwp_augment_batch whose float masks come from crowd RLEs: sample n's mask is rendered from its segmentations (CSR as above)
 * at plans[n].src_h x src_w into a workspace the handle owns, behind the batch's one upload, in which the run tables ride;
 * the augment kernel then reads it in place.  A sample with segmentations must have plans[n].mask == NULL (LWP_ERR_ARG); one
 * without keeps its mask as given: NULL stays all ones with the mask taps skipped.  Everything else, the checks of both calls
 * included, is as lwp_augment_batch and lwp_crowd_masks say. */
int lwp_augment_batch_crowd(lwp_handle h, const lwp_augment_plan* plans, int N, int crop_h, int crop_w, int stride,
                            const int64_t* counts, const int64_t* seg_off, const int64_t* image_seg_off, float* image_out,
                            unsigned char* mask_out, float* mask_small_out);

/* ---- JPEG files: replaces cv2.imread(path, cv2.IMREAD_COLOR) in front of the sample path (datasets/coco.py:33, val.py:124,
 *      demo.py:20) for baseline files.  The host parses the markers and decodes the Huffman data (csrc/jpeg_host.cpp, no GPU);
 *      the device dequantises, runs libjpeg's default integer inverse DCT (jidctint.c's slow-but-accurate form: column pass
 *      descaled by 11, then row pass descaled by 18), fancy up-sampling and the table-driven YCbCr conversion, and stores
 *      interleaved BGR (csrc/jpeg_kernels.hip).  Every step is integer arithmetic, restated from libjpeg and pinned
 *      bit for bit against libjpeg-turbo as Pillow bundles it; agreement with cv2 itself is NOT pinned (cv2 is not a
 *      dependency).  The Exif orientation is reported and never applied, unlike cv2.imread from version 3.1 on.
 *      IN SCOPE: SOF0 (baseline sequential Huffman, 8-bit), one interleaved scan, 1 component (grey; B = G = R = Y) or 3
 *      (YCbCr), luma sampling 1x1 / 2x1 / 2x2 with both chroma components at 1x1, 8-bit quantisation tables, up to 4 + 4
 *      Huffman tables, DRI / RSTn, 0xFF fill bytes in front of markers, APPn / COM skipped, APP14 Adobe with transform 1 or
 *      none.  REFUSED with LWP_ERR_ARG, the message naming the reason and the byte offset: SOF1 / SOF2 (progressive) / SOF3
 *      and above, arithmetic coding, 12-bit samples, 4 components, Adobe transform 0 or 2, any other sampling, several scans,
 *      DNL, 16-bit quantisation tables, a missing table, a width or height of 0, and every malformed or truncated stream (a
 *      segment length past the end, entropy data that ends before the last MCU, a Huffman code that matches no symbol, a DC
 *      category above 11, an AC size above 10, a run past coefficient 63, a wrong or missing RSTn, a missing EOI).  libjpeg
 *      warns and carries on in several of these cases; this library refuses them.
 *      lwp_jpeg_header: blocks_w / blocks_h are each component's block-padded grid (mcus_x * h_samp by mcus_y * v_samp 8x8
 *      blocks); a single-component file reports sampling 1x1 whatever its frame header states.
 *      COEFFICIENT LAYOUT (lwp_debug_jpeg_blocks; what the device entropy decoder below fills too): int16, 64 per block in natural
 *      (de-zig-zagged, row-major) order, DC prediction undone, not dequantised; blocks in plane order, component by component,
 *      each component's blocks row-major over its block-padded grid; qtables: 4 slots of 64 uint16 in natural order, component
 *      c using slot quant_table[c]. */
typedef struct lwp_jpeg_header {
    int width, height, components;
    int h_samp[3], v_samp[3], quant_table[3];
    int restart_interval;                  /* MCUs between restart markers, 0: none */
    int mcus_x, mcus_y;
    int orientation;                       /* Exif tag 0x0112 of APP1 (1..8), 0: none; reported only */
    int blocks_w[3], blocks_h[3];
    int64_t total_blocks;                  /* 64 coefficients each */
} lwp_jpeg_header;
/* the header of one file (HOST bytes): parsed up to its scan header.  No handle, no GPU; message via lwp_last_error(NULL). */
int lwp_jpeg_info(const unsigned char* data, size_t len, lwp_jpeg_header* out);
/* the host half alone, for tests: coefficients (coef_cap int16 available; LWP_ERR_CAPACITY below 64 * total_blocks of
 * lwp_jpeg_info) and quantisation tables (qtables[256]) of one file.  No handle, no GPU; safe to call from several threads. */
int lwp_debug_jpeg_blocks(const unsigned char* data, size_t len, int16_t* coef, size_t coef_cap, uint16_t* qtables);
/* N files (HOST bytes data[i], len[i]) -> out[i], a DEVICE pointer to height * width * 3 bytes of row-major BGR that the caller
 * sized from lwp_jpeg_info.  1 <= N <= 65535.  All N files are parsed and entropy-decoded before anything is enqueued: a
 * refused file fails the whole call with its index in the message (the lowest, if several are) and no output is written.  From
 * 256 KiB of input on, the files' entropy decode is shared among up to 16 host threads that live for the call; the result does
 * not depend on it.  Coefficients, tables and the
 * per-image descriptors go up in ONE copy through pinned staging; two launches (inverse DCT into block-padded uint8 planes
 * in a workspace of the handle; up-sample + colour + store) cover the whole batch, files of different sizes and samplings
 * mixed.  Runs on the handle's stream and honours lwp_set_stream like the other device-returning calls; the staging is not
 * rewritten while the copy of an earlier call may be pending.  Workspace and staging show in lwp_debug_live_resources and go
 * with lwp_destroy.  Needs no weights.  Two calls on the same bytes return the same bits. */
int lwp_jpeg_decode_batch(lwp_handle h, int N, const unsigned char* const* data, const size_t* len, unsigned char* const* out);
/* the two kernels alone (tools/jpeg_bench.py): the same checks, decode and upload, then `iters` back-to-back launches of each
 * stage between HIP events.  ms_total[2] out: stage A, stage B. */
int lwp_time_jpeg_decode_batch(lwp_handle h, int N, const unsigned char* const* data, const size_t* len, unsigned char* const* out,
                               int iters, float* ms_total);

/* ---- JPEG files, entropy decode on the device (csrc/jpeg_entropy_kernels.hip).  An opt-in mode of
 *      lwp_jpeg_decode_batch / lwp_time_jpeg_decode_batch: the default stays the host decode, and the pixels, the refusals and
 *      their messages are the same in both modes.  In device mode the host only parses the headers and walks each scan once
 *      (csrc/jpeg_host.cpp's jpeg_scan_segments: FF 00 un-stuffed into the pinned staging, the scan cut at the RSTn markers, RST
 *      numbering / count and the trailer checked, the Huffman tables flattened); the call then issues ONE upload [un-stuffed
 *      scans | Huffman tables | quantisation tables | records], zero-fills the coefficients and runs self-synchronising
 *      parallel Huffman decoding (one lane a subsequence of subseq_bytes of one restart interval; decoder state = bit position,
 *      block in MCU, coefficient index; sync inside a workgroup, then across workgroups, both with round caps that make the
 *      result exact for any stream; write pass; DC scan in stream order), which fills exactly the COEFFICIENT LAYOUT above.
 *      The N status words are copied back and the call WAITS for them (the one host wait host mode does not have) before
 *      stage A is enqueued, so a refused file still fails the whole call with its index (the lowest) and nothing is written.
 *      The message of a refusal is the host decoder's, which is run on the refused file; a file the device refuses and the
 *      host accepts is LWP_ERR_INTERNAL naming the file and both verdicts.  A scan of 2^28 or more un-stuffed bytes is
 *      LWP_ERR_CAPACITY in device mode.  Staging event, lwp_set_stream ordering, lwp_debug_live_resources and lwp_destroy as
 *      for host mode. */
enum { LWP_JPEG_ENTROPY_HOST = 0, LWP_JPEG_ENTROPY_DEVICE = 1 };
/* subseq_bytes: 0 (the default, 128) or a multiple of 4 from 4 to 1024; 32 bits hold the longest symbol (16 code bits and 11
 * magnitude bits).  LWP_ERR_ARG for any other value or mode. */
int lwp_set_jpeg_entropy(lwp_handle h, int mode, int subseq_bytes);
/* the pre-pass and the entropy kernels alone, for tests: status_out[i] 0 accepted, non-zero refused (by the header, the
 * pre-pass or the kernels) without failing the call; an accepted file's coefficients (64 * total_blocks int16) go to the HOST
 * buffer coef_out[i] and its tables to qtables_out[i][256].  subseq_bytes 0: the handle's setting. */
int lwp_debug_jpeg_entropy_batch(lwp_handle h, int N, const unsigned char* const* data, const size_t* len, int subseq_bytes,
                                 int16_t* const* coef_out, uint16_t* const* qtables_out, int* status_out);
/* the pre-pass alone.  No handle, no GPU.  bytes_out (bytes_cap available; len suffices): the un-stuffed scan; segs_out
 * (segs_cap segments available): four uint32 a segment (un-stuffed byte offset, byte length, first MCU, MCU count); tables_out
 * (may be NULL): 6 * 1488 bytes, the DC tables of components 0..2 and then their AC tables as the kernels read them (512 uint16
 * of 9-bit look-up, 17 int32 each of maxcode / mincode / valptr, 256 symbols, 4 bytes of padding); qtables_out (may be NULL):
 * 256 uint16.  *status_out: 0 accepted so far, 1 refused, 2 the scan is too long for device mode.  LWP_ERR_ARG if the header
 * itself is refused. */
int lwp_debug_jpeg_scan(const unsigned char* data, size_t len, unsigned char* bytes_out, size_t bytes_cap, size_t* n_bytes,
                        uint32_t* segs_out, size_t segs_cap, size_t* n_segs, unsigned char* tables_out, uint16_t* qtables_out,
                        int* status_out);
/* the entropy kernels alone (tools/jpeg_entropy_bench.py): the checks, pre-pass and upload of device mode, then `iters`
 * back-to-back runs of the memset and the four kernels between HIP events.  rounds[2] out: the most sync rounds a workgroup
 * took, and the most rounds across workgroups. */
int lwp_time_jpeg_entropy_batch(lwp_handle h, int N, const unsigned char* const* data, const size_t* len, int subseq_bytes,
                                int iters, float* ms_total, int* rounds);

/* ---- JPEG files, written: replaces cv2.imwrite(path.jpg, img) and, behind demo.VideoWriter, a Motion-JPEG cv2.VideoWriter
 *      (the reference only shows its result, demo.py:128-166).  The whole encoder runs on the device
 *      (csrc/jpeg_encode_kernels.hip); what crosses to the host is the compressed scan, not pixels.  Every step is
 *      libjpeg's default compression path in integer arithmetic, restated and pinned byte for byte against the files Pillow
 *      (libjpeg-turbo) writes of the same pixels; agreement with cv2.imwrite itself is NOT pinned (cv2 is not a dependency).
 *        colour        jccolor.c, 16-bit fixed point: Y = (19595 R + 38470 G + 7471 B + 32768) >> 16, Cb and Cr likewise
 *        sampling      4:4:4, 4:2:2 (h2v1, bias 0, 1, 0, 1 .. along the columns), 4:2:0 (h2v2, bias 1, 2, 1, 2 ..); no smoothing
 *        edges         a component has ceil(ceil(W h / hmax) / 8) by ceil(ceil(H v / vmax) / 8) REAL blocks; the right edge repeats
 *                      the last pixel up to them; the bottom edge repeats the last pixel row up to a multiple of vmax rows only,
 *                      and the last DOWN-SAMPLED row from there; the other blocks of the MCU-padded grids are DUMMY blocks: 63
 *                      zeros and the DC of the block before them in MCU order (jccoefct.c)
 *        forward DCT   jfdctint.c (CONST_BITS 13, PASS1_BITS 2) on sample - 128, rows then columns
 *        quantiser     sign(c) * ((|c| + (8 q >> 1)) / (8 q)); q from jpeg_quality_scaling of Annex K's two tables, clamped to 1..255
 *        entropy code  Annex K's four Huffman tables; the last byte of the scan and of every restart interval padded with one-bits;
 *                      00 stuffed behind every FF; RSTn between the intervals
 *      The stage in front of the entropy code leaves its coefficients in exactly the COEFFICIENT LAYOUT of the decoder above.
 *      FILE LAYOUT (Pillow's): SOI, APP0 JFIF 1.1 (units 0, density 1 x 1), DQT 0, DQT 1, SOF0 (components 1, 2, 3 with tables
 *      0, 1, 1), DHT DC 0, AC 0, DC 1, AC 1, DRI if restart_interval > 0, SOS, the scan, EOI.
 *      OUT OF SCOPE: grey output, optimised Huffman tables, progressive and arithmetic coding, 4:4:0 / 4:1:1, custom
 *      quantisation tables, Exif.  A height or width outside 1..65535 is LWP_ERR_ARG with the image's index. */
enum { LWP_JPEG_444 = 0, LWP_JPEG_422 = 1, LWP_JPEG_420 = 2 };     /* Pillow's subsampling numbers */
/* bytes that hold the file of a height x width frame whatever its pixels: the header, every block at its longest code with
 * every byte stuffed, a marker an interval.  Far above what pictures take (about 416 bytes a block).  No handle, no GPU. */
int lwp_jpeg_encode_bound(int height, int width, int subsampling, int restart_interval, size_t* bound_out);
/* N frames (frames[i]: heights[i] x widths[i] x 3 bytes of row-major BGR, all in HOST memory or all in DEVICE memory as mem says;
 * host frames go up in ONE copy with the per-image records, device frames are read in place) -> N whole files.  1 <= N <= 65535,
 * sizes mixed; quality 1..100, subsampling LWP_JPEG_444 / 422 / 420 and restart_interval (MCUs, 0..65535) hold for the batch.
 * Six launches and one memset cover the batch; the call enqueues everything, WAITS once for the N scan lengths, checks the
 * capacities and then copies the scans out through pinned staging.  out[i]: HOST memory of cap[i] bytes that receives file i,
 * or NULL: then only len_out[i] is reported (a sizing call; the scan stays in the handle's workspace until the next call and is
 * not fetched).  len_out[i]: the length of file i.  cap[i] below that is LWP_ERR_CAPACITY with the image's index (the lowest) in
 * the message, and NO out[i] is written; lwp_jpeg_encode_bound always suffices.  Runs on the handle's stream and waits for the
 * caller's stream as lwp_set_stream says; workspace and staging show in lwp_debug_live_resources and go with lwp_destroy.  Needs
 * no weights.  The same frames give the same bytes. */
int lwp_jpeg_encode_batch(lwp_handle h, int N, const unsigned char* const* frames, int mem, const int* heights, const int* widths,
                          int quality, int subsampling, int restart_interval, unsigned char* const* out, const size_t* cap,
                          size_t* len_out);
/* the first stage alone, for tests: the quantised coefficients of frame i (64 * total_blocks int16 in the COEFFICIENT LAYOUT;
 * total_blocks as lwp_jpeg_info reports it of the header) to the HOST buffer coef_out[i], the batch's tables to qtables_out[256]
 * (slots 0 and 1). */
int lwp_debug_jpeg_encode_blocks(lwp_handle h, int N, const unsigned char* const* frames, int mem, const int* heights,
                                 const int* widths, int quality, int subsampling, int16_t* const* coef_out, uint16_t* qtables_out);
/* the other stages alone, for tests: the entropy code of the CALLER's coefficients.  coef[i]: HOST memory, 64 * total_blocks
 * int16 in the COEFFICIENT LAYOUT, which is what lwp_debug_jpeg_encode_blocks returns; a DC outside -1024..1023 or an AC term
 * outside -1023..1023 (no 8-bit picture has more, and the kernels' tables end there) is LWP_ERR_ARG with the image's index
 * before anything is enqueued.  The call plans and uploads as lwp_jpeg_encode_batch does, copies the coefficients where the
 * first stage would have left them and runs the memset and the other five launches.  out[i] (cap[i] bytes, or NULL) receives
 * the stuffed scan alone, RSTn markers included: no header and no EOI; len_out[i] its length.  cap[i] below that is
 * LWP_ERR_CAPACITY and no out[i] is written. */
int lwp_debug_jpeg_encode_scan(lwp_handle h, int N, const int16_t* const* coef, const int* heights, const int* widths,
                               int subsampling, int restart_interval, unsigned char* const* out, const size_t* cap, size_t* len_out);
/* the header bytes alone, SOI up to and including SOS (at most 640 bytes; LWP_ERR_CAPACITY if cap is below them).  No handle,
 * no GPU. */
int lwp_debug_jpeg_encode_header(int height, int width, int quality, int subsampling, int restart_interval, unsigned char* out,
                                 size_t cap, size_t* n_out);
/* the kernels alone (tools/jpeg_encode_bench.py): the checks and the upload, one run of all stages, then `iters` back-to-back
 * launches of each stage between HIP events.  ms_total[6] out: A colour / sampling / DCT / quantiser, B bit counts, C offsets,
 * D memset and code write, E FF counts, F stuffing. */
int lwp_time_jpeg_encode_batch(lwp_handle h, int N, const unsigned char* const* frames, int mem, const int* heights,
                               const int* widths, int quality, int subsampling, int restart_interval, int iters, float* ms_total);

/* ---- COCO key-point evaluation: replaces pycocotools' COCOeval(gt, dt, 'keypoints') evaluate() + accumulate() behind
 *      val.py:17-27, with COCOeval's default parameters (the 17 OKS sigmas, IoU thresholds 0.5:0.05:0.95, 101 recall
 *      thresholds, maxDets 20, area ranges all [0, 1e10] / medium [32^2, 96^2] / large [96^2, 1e10], inclusive at both ends) and
 *      ONE category.  All arithmetic is float64 on the GPU (csrc/eval_kernels.hip); summarize() is a mean over the
 *      returned arrays and stays with the caller (val.run_coco_eval).
 *      Inputs (HOST), CSR over n_images images in ascending image id: image i owns detections dt_off[i] .. dt_off[i + 1] - 1 and
 *      ground truths gt_off[i] .. gt_off[i + 1] - 1, each in its file's order (ties in score keep it).
 *        dt_kp [ND][17][3], dt_score [ND]      x, y and a third value that is not read; the detection's area is the box of all
 *                       17 (x, y), zeros of missing key-points included, as loadRes computes it
 *        gt_kp [NG][17][3]                     x, y, visibility (visible: > 0)
 *        gt_area [NG], gt_bbox [NG][4], gt_iscrowd [NG], gt_ignore [NG]   gt_ignore is COCOeval's _prepare flag: iscrowd or
 *                       num_keypoints == 0
 *      Per image: the 20 best detections (stable), their OKS against every ground truth, and for each of the 3 x 10 (range,
 *      threshold) pairs COCOeval's greedy matching.  Over the data set: the selected detections in descending score order
 *      (stable), the running tp / fp counts, precision's running maximum from the end and the 101 recall look-ups.
 *      Outputs (HOST): precision [10][101][3] and scores [10][101][3] indexed [threshold][recall][range], recall [10][3],
 *      npig [3] (ground truths that count per range).  A range with npig == 0 holds -1 throughout.
 *      Checks before any launch (h == NULL too, LWP_ERR_ARG): null pointers (an array with no element may be NULL),
 *      n_images >= 1, offsets that start at 0 and never descend, fewer than 2^31 detections and ground truths, finite scores,
 *      coordinates, areas and boxes.  One upload, the kernels on the handle's stream, one copy back; every byte of scratch is
 *      released before the call returns.  Needs no weights.  Two calls on the same input return the same bits. */
int lwp_coco_eval(lwp_handle h, int n_images, const int64_t* dt_off, const double* dt_kp, const double* dt_score,
                  const int64_t* gt_off, const double* gt_kp, const double* gt_area, const double* gt_bbox, const int* gt_iscrowd,
                  const int* gt_ignore, double* precision, double* recall, double* scores, int64_t* npig);
/* the per-image half alone, for tests: the same inputs and checks, then for image `image`: n_sel = min(D, 20) and order[r], the
 * index within the image of the detection at rank r; oks [n_sel][G] row-major, columns in input ground-truth order (oks_cap
 * doubles available, LWP_ERR_CAPACITY below n_sel * G); matched / ignored [30][20] bytes indexed [range * 10 + threshold][rank]
 * (ranks from n_sel on are 0); npig3 [3], the image's ground truths that count per range. */
int lwp_debug_coco_oks(lwp_handle h, int n_images, const int64_t* dt_off, const double* dt_kp, const double* dt_score,
                       const int64_t* gt_off, const double* gt_kp, const double* gt_area, const double* gt_bbox, const int* gt_iscrowd,
                       const int* gt_ignore, int image, int* n_sel, int* order, double* oks, int64_t oks_cap, unsigned char* matched,
                       unsigned char* ignored, int* npig3);

/* ---- device-resident validation: the detection loop of val.py:113-160 without a fetch.  A DETECTION STORE on the device takes
 *      the poses of every validated image straight from the grouping's result block (val.py:52-78 restated by an append
 *      kernel), the ground truth is uploaded once per data set, and lwp_coco_finish runs the kernels of lwp_coco_eval on the
 *      store: no per-image synchronise, no Python object between the grouping and AP / AR.
 *      lwp_coco_open: the ground-truth arrays exactly as lwp_coco_eval takes them (HOST; the same checks, with a NULL handle too),
 *      uploaded once, and a store of row_cap >= 0 detection rows ([17][3] float64 key-points, a float64 score, the image index)
 *      with per-image start / count tables, a row cursor and a sticky status word, all on the device.  A second open replaces
 *      the first; lwp_coco_release frees everything (so does lwp_destroy; a release without a store is LWP_OK).  The memory
 *      shows in lwp_debug_live_resources.  lwp_coco_reset forgets the detections and the status and keeps the ground truth.
 *      lwp_coco_add_maps: arguments and checks of lwp_poses_from_maps for DEVICE maps; image_index[N] (HOST) is frame f's
 *      position in the ground truth's ascending image-id order.  Enqueues the grouping on the serial workspace and the append
 *      kernel behind it and RETURNS WITHOUT SYNCHRONISING: under lwp_set_stream the caller's stream is ordered before and behind
 *      it, as for lwp_infer_poses_async.  Frame f's rows follow frame f - 1's, in entry order (no atomic places a row; COCOeval
 *      breaks score ties by this order).  A pose row is 17 x (x + 0.5, y + 0.5, 1.0) in COCO's key-point order, (0, 0, 0) for a
 *      key-point that was not found (the neck has no slot); its score is entry[18] * max(0, entry[19] - 1), one float64
 *      multiply.  Checked on the host before anything is enqueued: LWP_ERR_STATE without a store, for an image that was
 *      already added (the message names it), under a custom skeleton (COCO's mapping is defined for the default 18 / 19 / 20
 *      only) and with tracking mode 2 or 3 on (no lane may advance on validation frames); LWP_ERR_ARG for an index outside
 *      0 .. n_images - 1.  The serial workspace then holds nothing to fetch: a following lwp_fetch_poses is LWP_ERR_STATE.
 *      lwp_coco_add_rows: n >= 0 ready-made rows (HOST, finite) of one image through the same cursor; enqueue only.
 *      Host arrays of both add calls (the image indices, the rows) reach the kernels through a pinned ring of 1 MiB, grown to the
 *      largest single request: the ONE exception to "no synchronise" is that a call which finds the ring full waits for the
 *      stream once before it reuses the ring from its start (about every 2500 rows of lwp_coco_add_rows, every 65 000 calls of
 *      lwp_coco_add_maps with a few frames each).
 *      STATUS: what a fetch would have reported is kept on the device, the first error wins, and lwp_coco_counts / lwp_coco_rows /
 *      lwp_coco_finish return it until lwp_coco_reset: a frame whose grouping overflowed a capacity is LWP_ERR_CAPACITY (the
 *      message names the image and the bits), the reference's unbound 'ratio' LWP_ERR_UNBOUND, a non-finite value
 *      LWP_ERR_ARG.  Rows beyond row_cap are not written while the cursor keeps counting: LWP_ERR_CAPACITY, and the message
 *      names the row_cap that would have fitted.
 *      lwp_coco_counts: *n_rows and, unless NULL, per_image_counts[n_images].  lwp_coco_rows: the rows IN THE EVALUATION'S ORDER
 *      (images ascending, within an image the order they were added): dt_image [n], dt_kp [n][17][3], dt_score [n] for the n
 *      rows lwp_coco_counts reported; row_cap is what the arrays hold (LWP_ERR_CAPACITY below n).  Each of the two synchronises
 *      once: lwp_coco_rows forms the offsets on the device, so the tables and the gathered rows come back together.
 *      lwp_coco_finish: one copy of the tables (counts and status), the host forms the offsets, a gather kernel compacts the store
 *      into lwp_coco_eval's layout in scratch, then the same match / sort / accumulate launches and one copy back: outputs as
 *      lwp_coco_eval's, bit for bit equal to it on the same rows.  The store is left intact: finish twice returns the same
 *      bits, and finish, more adds, finish is allowed. */
int lwp_coco_open(lwp_handle h, int n_images, const int64_t* gt_off, const double* gt_kp, const double* gt_area, const double* gt_bbox,
                  const int* gt_iscrowd, const int* gt_ignore, int row_cap);
int lwp_coco_release(lwp_handle h);
int lwp_coco_reset(lwp_handle h);
int lwp_coco_add_maps(lwp_handle h, const float* heat, const float* paf, int layout, int N, int hs, int ws, int upsample_ratio,
                      int demo, const int* image_index);
int lwp_coco_add_rows(lwp_handle h, int image_index, int n, const double* dt_kp, const double* dt_score);
int lwp_coco_counts(lwp_handle h, int64_t* n_rows, int* per_image_counts);
int lwp_coco_rows(lwp_handle h, int* dt_image, double* dt_kp, double* dt_score, int64_t row_cap);
int lwp_coco_finish(lwp_handle h, double* precision, double* recall, double* scores, int64_t* npig);
/* the append kernel alone, for tests: N frames of host pose entries (frame f's n_entries[f] rows of 20 doubles, back to back)
 * and key-point rows (kpt_counts[f] rows of 4 doubles, back to back) are loaded into the serial workspace's result block, then
 * appended as image_index[N] like the frames of lwp_coco_add_maps; synchronises. */
int lwp_debug_coco_rows(lwp_handle h, int N, const double* entries, const int* n_entries, const double* kpts, const int* kpt_counts,
                        const int* image_index);

/* ---- measurement helpers (bench.py): time `iters` back-to-back enqueues with HIP events on the
 *      handle's own stream.  what: 0 = forward only, 1 = full infer_poses.  ms_total out. */
int lwp_time_pipeline(lwp_handle h, const float* in_device, int N, int H, int W, int upsample_ratio,
                      int demo, int what, int iters, float* ms_total);
/* per-kernel-class device time of ONE pass, measured with HIP events around each launch on the
 * handle's stream: classes 0=stem 1=depthwise 2=pointwise-1x1 3=dense-3x3 4=post 5=other.
 * ms[6], launches[6] out. */
int lwp_profile_classes(lwp_handle h, const float* in_device, int N, int H, int W, int upsample_ratio,
                        int demo, int reps, float* ms, int* launches);
/* per-launch device time of one pass (averaged over reps): ms[i], kclass[i] for launch i in issue order.
 * kclass[i] & 0xff = kernel class as above; kclass[i] >> 8 = 1 + index of the first layer the launch covers
 * (a fused head pair is ONE launch covering two layers), 0 for a post-processing kernel. */
int lwp_profile_launches(lwp_handle h, const float* in_device, int N, int H, int W, int upsample_ratio,
                         int demo, int reps, float* ms, int* kclass, int cap, int* n_launches);
int lwp_synchronize(lwp_handle h);

/* ---- introspection / per-layer parity (tests): the layer list mirrors the module tree of
 *      models/with_mobilenet.py:92-112.  lwp_debug_layer_output runs the first layer_index+1 layers on
 *      `in` (host, N x 3 x H x W) and copies that layer's output to dst (host) as NCHW float32
 *      N x cout x h x w; dims are returned in out_dims[4]. */
int lwp_layer_count(lwp_handle h);
int lwp_layer_info(lwp_handle h, int layer_index, char* name, int name_cap, int* kind, int* cin, int* cout,
                   int* ksize, int* stride, int* dilation, int64_t* macs_per_pixel /* algorithmic multiply-adds */);
/* average device time (ms) of `iters` back-to-back launches of one layer on the current buffers.  A head pair that lwp_forward
 * runs as one kernel is timed at its first layer and its second layer reports 0; a folded 1x1 is NOT applied: a dense 3x3 is
 * timed alone, and so is the 1x1 behind it */
int lwp_debug_time_layer(lwp_handle h, int layer_index, int N, int H, int W, int iters, float* ms_avg);
int lwp_debug_layer_output(lwp_handle h, const float* in, int N, int H, int W, int layer_index,
                           float* dst, size_t dst_floats, int out_dims[4]);
/* name of the kernel variant the LAST lwp_debug_layer_output / lwp_profile_launches pass picked for a layer, e.g.
 * "dw_tiled<cc=64,s=1,d=1,ph=8>" or "gemm_bf16_ar<256,4,2,3>" ("" before any such pass; the second layer of a fused head
 * pair reports the pair's kernel).  Lets a test prove that the kernel it means to cover is the one that ran: the launchers
 * choose by problem size, and the A/B switches (environment, read once per handle in lwp_create) only override that choice. */
int lwp_debug_layer_variant(lwp_handle h, int layer_index, char* name, int name_cap);
/* the host's f32 -> fp16 conversion of LWP_F16 weight packing (round to nearest even, subnormals kept, inf beyond 65520),
 * n values; no handle, no GPU */
int lwp_debug_f32_to_f16(const float* src, uint16_t* dst, int64_t n);
/* which neighbouring layers of the layer list may share ONE launch, as the graph builder marks them once per graph (the
 * handle's switches and the launchers' size limits decide at run time whether a marked step is taken): fuse[i] for layer i,
 * its name at names + i * name_stride (names may be NULL).  LWP_MARK_HEADS_PAIR: layer i and i + 1 are a stage's merged head
 * pair; LWP_MARK_FOLD_NEXT_1X1: layer i + 1, a 1x1, may ride in the epilogue of layer i, a dense 3x3 (16-bit graphs only).
 * fuse_dwpw / merge_heads as LWP_FUSE_DWPW / LWP_MERGE_HEADS give them to lwp_create.  *n_layers out; LWP_ERR_CAPACITY when
 * cap is below it or a name does not fit name_stride.  The retaining plan of lwp_train_forward is a copy of this list with
 * the same marks at the same indices: for LWP_F32, fuse[i] from cpm.conv on is read from that copy.  No handle, no GPU. */
enum { LWP_MARK_NONE = 0, LWP_MARK_HEADS_PAIR = 1, LWP_MARK_FOLD_NEXT_1X1 = 2 };
int lwp_debug_graph_fusions(int num_refinement_stages, int num_channels, int num_heatmaps, int num_pafs, int dtype, int fuse_dwpw,
                            int merge_heads, int* fuse, char* names, int name_stride, int cap, int* n_layers);
/* frames one launch sequence of an N x 3 x H x W call takes (N unless a tensor of the pass would reach the kernels' 2 GiB
 * addressing range: lwp_forward / lwp_infer_poses* / lwp_pipeline_submit then walk the batch in equal chunks of this size) */
int lwp_debug_frames_per_pass(lwp_handle h, int N, int H, int W);
/* intermediate counts of the grouping kernels for frame `frame` of the handle's LAST lwp_infer_poses / lwp_infer_poses_async /
 * lwp_poses_from_maps call (after its results were fetched): candidate peaks per key-point type before the NMS [18], key-points per
 * type after it [18], scored connection candidates per limb [19], connections picked per limb [19].  Tests / tools: which
 * form of nms_kernel / match_kernel (register form up to 64 candidates, LDS form beyond) a workload exercises. */
int lwp_debug_post_counts(lwp_handle h, int frame, int* peaks18, int* kpts18, int* candidates19, int* picked19);
/* the same for any skeleton: peaks[K], kpts[K], candidates[L], picked[L]; K and L must be the skeleton's (LWP_ERR_ARG otherwise).
 * lwp_debug_post_counts itself keeps its [18] / [19] contract and returns LWP_ERR_STATE under a non-default skeleton. */
int lwp_debug_post_counts_ex(lwp_handle h, int frame, int* peaks, int* kpts, int* candidates, int* picked, int K, int L);
/* which grouping kernels the handle launches: 1 = the generic forms (a custom skeleton, or LWP_POST_GENERIC=1 at lwp_create),
 * 0 = the COCO-specialised ones */
int lwp_debug_post_generic(lwp_handle h);
/* what the library holds right now, over all handles of the process: out[0] bytes of device memory, out[1] bytes of pinned
 * host memory, out[2] events, out[3] streams.  A destroyed handle has given back everything it took.  No handle, no GPU. */
int lwp_debug_live_resources(int64_t out[4]);

#ifdef __cplusplus
}
#endif
#endif /* LWPOSE_H */
