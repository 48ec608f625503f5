/*
 * flope_amd.h -- C-ABI of the MI355X-native flower-pose hot path.
 *
 * The reference (wvu-irl/flope) has no FFI of its own: its seam is Python
 * duck-typing on an nn.Module and two predictor classes.  This
 * header is therefore the build-defined boundary the Python facade
 * (flope_amd/sunflower/...) binds with ctypes; every entry point names the
 * reference call it replaces.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, no C++/torch types.
 *   - every function returns 0 on success, a negative FLOPE_E* code otherwise;
 *     flope_last_error() returns the message of the last failure on the handle
 *     (or of the last handle-less failure when h == NULL).
 *   - "dev" pointers are device (HBM) addresses owned by the caller
 *     (tensor.data_ptr()); "host" pointers are ordinary host memory.
 *   - kernels are enqueued on the hipStream_t passed as `void* stream`
 *     (0 = the null stream); nothing synchronises internally and nothing is
 *     allocated inside flope_forward / flope_procrustes / flope_crop_* /
 *     flope_depth_* (workspace is allocated by flope_create).
 *   - a handle is bound to one device and is not thread-safe.
 */
#ifndef FLOPE_AMD_H
#define FLOPE_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct flope_engine* flope_handle;

/* error codes */
#define FLOPE_OK            0
#define FLOPE_EINVAL       -1   /* bad argument / shape */
#define FLOPE_EHIP         -2   /* a HIP runtime call failed */
#define FLOPE_ESTATE       -3   /* call order (e.g. forward before load_weights) */
#define FLOPE_EWEIGHTS     -4   /* state_dict entry missing / wrong shape / not finite */

/* arithmetic type of the trunk (activations + conv weights as stored in HBM;
 * accumulation, bias, residual add and the whole head are always fp32) */
#define FLOPE_DT_BF16       0   /* MFMA v_mfma_f32_16x16x32_bf16 */
#define FLOPE_DT_F16        1   /* MFMA v_mfma_f32_16x16x32_f16  */
#define FLOPE_DT_F32        2   /* strict mode: plain fp32 direct convolution (no MFMA) */
/* FLOPE_DT_F32 with flope_set_option(h, "f32mfma", 1): the same float32 buffers and stages, the stem and the 19 trunk convs on
 * v_mfma_f32_16x16x4_f32 (exact float32 products and sums; differs from the strict mode in summation order only).
 * With flope_set_option(h, "f32m_ksplit", 1) on top of it: split-K for small batches -- a trunk conv whose launch would leave most
 * of the chip idle runs as S workgroups per tile, each a share of K from +0, and an ordered second launch adds bias + share 0 +
 * share 1 + ... + residual in that fixed order (another summation order again, still float32 throughout). */

/* layout / dtype of the crop batch handed to flope_forward */
#define FLOPE_IN_F32_NCHW   0   /* reference API: float32 [B,3,H,W] in [0,1] (posenet.py:31) */
#define FLOPE_IN_BF16_NHWC  1   /* bfloat16 [B,H,W,3] in [0,1]  (BASELINE cfg2) */
#define FLOPE_IN_F16_NHWC   2   /* float16  [B,H,W,3] in [0,1] */
#define FLOPE_IN_U8_NHWC    3   /* uint8    [B,H,W,3] 0..255, scaled by 1/255 on load */

/* activation taps for flope_read_stage (parity tests) */
#define FLOPE_STAGE_STEM    0   /* conv1+bn1+relu          [B,64,H/2,W/2] */
#define FLOPE_STAGE_POOL    1   /* maxpool                 [B,64,H/4,W/4] */
#define FLOPE_STAGE_LAYER(li, bi)  (2 + ((li) - 1) * 2 + (bi))   /* li 1..4, bi 0..1 */
#define FLOPE_STAGE_FEAT    10  /* global average pool     [B,512]  */
#define FLOPE_STAGE_HIDDEN  11  /* fc.0 + ReLU             [B,2048] */
/* inside a BasicBlock (element-wise conv tests: every conv's own input and output) */
#define FLOPE_STAGE_MID(li, bi)    (12 + ((li) - 1) * 2 + (bi))  /* conv1+bn1+relu of the block, li 1..4, bi 0..1 */
#define FLOPE_STAGE_DS(li)         (20 + ((li) - 2))             /* 1x1 stride-2 shortcut conv + bn of layer li.0, li 2..4;
                                                                  * FLOPE_ESTATE when the last forward folded it into conv2 (option dsfuse) */

/* ---- life cycle ----------------------------------------------------------
 * Replaces PoseResNet().to(device)   (sunflower/models/posenet.py:6-22,
 * fast_pose_predictor.py:31): builds the fixed launch plan and allocates every
 * activation buffer for crops of height x width up to max_batch.  Never fetches
 * ImageNet weights (the reference does, posenet.py:10). */
int flope_create(int device_id, int height, int width, int max_batch, int dtype,
                 int backbone_out_dim, flope_handle* out);
int flope_destroy(flope_handle h);
const char* flope_last_error(flope_handle h);

/* Replaces model.load_state_dict(torch.load(path, weights_only=True))
 * (scripts/test_posenet.py:51, fast_pose_predictor.py:32).  Entries are host
 * fp32, contiguous, named exactly as in the reference's 124-entry state_dict
 * (num_batches_tracked entries may be omitted).  The library folds eval-mode
 * BatchNorm into each conv, converts to the trunk dtype, repacks into the
 * MFMA tile order and uploads. */
int flope_load_weights(flope_handle h, int n, const char* const* names,
                       const float* const* host_ptrs, const int* ndims,
                       const int64_t* const* shapes);

/* ---- the hot path ----------------------------------------------------------
 * Replaces  r9 = model(image_batch); R = procrustes_to_rotmat(r9)
 * (fast_pose_predictor.py:126-127, scripts/test_posenet.py:142-144).
 * x_dev: crop batch in `in_format`; r9_dev: float32 [B,9] (may be NULL);
 * R_dev: float32 [B,9] row-major 3x3 rotations (may be NULL).  batch <= max_batch. */
int flope_forward(flope_handle h, const void* x_dev, int in_format, int batch,
                  float* r9_dev, float* R_dev, void* stream);

/* PoseResNet.extract_features (posenet.py:24-29): float32 [B,backbone_out_dim]. */
int flope_extract_features(flope_handle h, const void* x_dev, int in_format, int batch,
                           float* feat_dev, void* stream);

/* Stand-alone  roma.special_procrustes(M.reshape(-1,3,3))
 * (sunflower/utils/conversion.py:54-58): float32 [n,9] -> float32 [n,9]. */
int flope_procrustes(const float* M_dev, float* R_dev, int n, void* stream);

/* nullify_yaw_batch (sunflower/utils/mvg.py:240-251): R' = R * Rz(atan2(-R01,R00))^T,
 * float32 [n,9] -> float32 [n,9] (in place allowed). */
int flope_nullify_yaw(const float* R_dev, float* out_dev, int n, void* stream);

/* Pose assembly (fast_pose_predictor.py:131-144): optional yaw-nullification of R,
 * then Rt = [[R, xyz],[0,0,0,1]] as float32 [n,16]; xyz_dev float32 [n,3] (NULL -> 0). */
int flope_compose_pose(const float* R_dev, const float* xyz_dev, int n, int nullify_yaw,
                       float* Rt_dev, void* stream);

/* flope_forward + flope_compose_pose in one launch sequence: the head kernel that solves the
 * Procrustes problem also nullifies the yaw (if asked) and writes Rt = [[R', xyz],[0,0,0,1]]
 * as float32 [batch,16].  xyz_dev float32 [batch,3] or NULL (zeros); r9_dev / R_dev optional. */
int flope_forward_poses(flope_handle h, const void* x_dev, int in_format, int batch,
                        const float* xyz_dev, int nullify_yaw, float* r9_dev, float* R_dev,
                        float* Rt_dev, void* stream);

/* Crop-batch assembly (4 copies in the reference: fast_pose_predictor.py:108-123,
 * pose_predictor.py:138-153, scripts/test_posenet.py:124-140,
 * scripts/generate_metrics_utils.py:17-35): for each square box
 * [xmin,ymin,xmax,ymax] crop frame and mask, Lanczos-4 resize both to size x size,
 * out = img * (mask/255) / 255.  frame_dev uint8 [H,W,3], mask_dev uint8 [H,W],
 * boxes_dev int32 [n,4]; out_dev float32 [n,3,size,size] (FLOPE_IN_F32_NCHW) or
 * 16-bit [n,size,size,3] (FLOPE_IN_BF16_NHWC / FLOPE_IN_F16_NHWC). */
int flope_crop_resize_mask(const uint8_t* frame_dev, const uint8_t* mask_dev,
                           int frame_h, int frame_w, const int32_t* boxes_dev, int n,
                           int size, int out_format, void* out_dev, void* stream);

/* Test hook for the call above: the Lanczos-4 tables of one axis resized n_src -> n_dst, evaluated on the device by
 * the same code the crop kernel runs: s0_dev int32 [n_dst] (position of the first of the eight taps, unclamped),
 * coef_dev int16 [n_dst,8] (cv2's x2048 fixed-point weights).  Parity tests compare them bit for bit with the oracle. */
int flope_lanczos4_table(int n_src, int n_dst, int32_t* s0_dev, int16_t* coef_dev, void* stream);

/* Detector post-processing of `get_bbox_mask` (fast_pose_predictor.py:50-54): sum of the n
 * instance masks (float32 [n,h,w], any values) -> clip to [0,1] -> x255 -> uint8 -> bilinear
 * resize to the frame (cv2.resize default INTER_LINEAR, 8-bit fixed-point arithmetic) ->
 * out_dev uint8 [H,W].  n == 0 gives an all-zero mask.  scratch_dev: >= h*w bytes. */
int flope_merge_masks_resize(const float* masks_dev, int n, int h, int w, uint8_t* scratch_dev,
                             uint8_t* out_dev, int H, int W, void* stream);

/* Depth statistics + back-projection (image_manipulation.py:39-96, mvg.py:387-408):
 * valid = (near < d < far) & (mask > 128), eroded by the 10x10 ellipse; per box the
 * mean of valid depths, count >= 50 => reliable; xyz = K^-1 [u,v,1]^T * d/|K^-1[u,v,1]|.
 * depth_dev: depth_format 0 = uint16 [H,W] raw units, 1 = float32 [H,W]; metres = value /
 * depth_div (1000 at fast_pose_predictor.py:90, 10000 at pose_predictor.py:118, 1 for the
 * float-metres argument of get_depth_value itself), boxes int32 [n,4]
 * (un-squared boxes), K = {fx,fy,cx,cy}.  Outputs: depth_val float32 [n] (metres),
 * reliable int32 [n], xyz float32 [n,3].  scratch_dev: >= H*W + 16 + 512*n bytes
 * (valid mask, then 32 strip partials of 16 bytes per box). */
int flope_depth_lift(const void* depth_dev, int depth_format, const uint8_t* mask_dev,
                     int frame_h, int frame_w, float depth_div, float near_plane, float far_plane,
                     const int32_t* boxes_dev, int n, const float* K4_host,
                     uint8_t* scratch_dev, float* depth_val_dev, int32_t* reliable_dev,
                     float* xyz_dev, void* stream);

/* ---- introspection (parity tests / DESIGN.md numbers) ----------------------- */
/* Copy one internal activation of the LAST forward to float32: conv stages (STEM, POOL,
 * LAYER, MID, DS) as NCHW [B,C,h,w]; FEAT / HIDDEN as [B,n].  dims_out[4] receives the shape.
 * Every block owns its MID and DS buffers, so all taps of one forward can be read after it -- unless that forward ran under
 * option "inplace": then only the stages whose buffer still holds them are served (STEM, every layer's last block output LAYER(l, 1)
 * and last conv1 output MID(l, 1), FEAT, HIDDEN) and the others fail with FLOPE_ESTATE and a message that names the option.  What
 * counts is the option's value during the last forward, not its value now. */
int flope_read_stage(flope_handle h, int stage, int batch, float* dst_dev,
                     int64_t* dims_out, void* stream);
/* runtime knobs (A/B variants inside one build); returns previous value or <0
 *   "f32mfma" (default 0): FLOPE_DT_F32 engines run the stem and every trunk conv on the exact-fp32 MFMA kernel (conv_f32m_kernel)
 *   instead of naive_conv_kernel; may be flipped between forwards (both weight images are loaded).  Stored and ignored by
 *   FLOPE_DT_F16 / BF16 engines.
 *   "f32m_ksplit" (default 0; stored clamped to 0..32): split-K of conv_f32m_kernel.  0 = off: launches, labels and every bit of
 *   every output as without the option.  1 = the planner picks a share count S in {1, 2, 4, 8, 16, 32} per conv launch (allowed only
 *   where the batch runs in one slice, tiles * S <= compute units and every share keeps >= 4 K steps; the stem is never split).
 *   2..32 = force that S, rounded down to a power of two, wherever a split is allowed (tests, A/B runs).  Split launches show as
 *   "layer[split-K xS]" in flope_launch_info; flope_forward_launches counts the conv once (its finalize launch belongs to it).
 *   NOTE: with the option on, S depends on the batch, so a crop's bits depend on HOW MANY crops run with it -- not on its position
 *   in the batch, not on its neighbours, not on the run.  May be flipped between forwards.  Stored and ignored by FLOPE_DT_F16 /
 *   BF16 engines and by FLOPE_DT_F32 engines with "f32mfma" = 0.
 *   "inline0" (default 1): where a forward runs as several batch slices, slice 0 is enqueued on the caller's stream itself and only
 *   the other slices on internal streams forked from / joined to it.  Slice 0 starts without a cross-queue hop, the other slices
 *   start one hop later (so option "lag"'s sleeping wave is skipped), and the join waits for one event fewer.  Slice 0's kernels
 *   inherit what the caller's stream carries (priority, CU mask).  0 = every slice on an internal stream, the last one behind
 *   "lag".  Same launches, same bits; no effect where the batch runs in one slice.  May be flipped between forwards.
 *   "inplace" (default 0): a BasicBlock's second conv stores its output over its residual input (the block input, or the
 *   materialised shortcut with "dsfuse" = 0; a conv2 with a folded shortcut keeps its own buffer), and the first conv of block X.1
 *   stores into block X.0's conv1 buffer: a layer touches two activation maps instead of five, which keeps them resident in the
 *   Infinity Cache.  Same launches, same bits; every buffer stays allocated, so the option may be flipped between forwards.
 *   flope_read_stage then serves only part of the stages (see there).
 *   "coldyw" (default 2): conv_s1r (layer 2's three 128 -> 128 convs on 224 x 224 crops).  1 = the look-ahead LDS-DMA pieces of
 *   the next band are issued by the SIMD's younger waves (4 - 7) alone, where they wait for the matrix pipe anyway; 2 = that, and
 *   the first band of a workgroup runs while its weights arrive instead of behind them; 0 = the schedule before both.  Same
 *   launches, same bits; may be flipped between forwards. */
int flope_set_option(flope_handle h, const char* name, int value);
/* developer aid of diagnostic builds (-DFLOPE_STAG_DBG, option "dbg" = 64): in-kernel clock stamps that conv launch i of
 * the last forward left in the split-K workspace at byte offset i * 1048576 ({clk0, clk1, rt0, rt1} uint64 per workgroup and
 * wave group; per-double-step stamps 64 KB further with "dbg" = 128) -> host memory.  A production build leaves the workspace untouched. */
int flope_debug_read_ws(flope_handle h, void* dst_host, size_t offset, size_t bytes);
/* developer aid: the packed 16-bit epilogue helpers of csrc/common.h applied to n caller-supplied 32-bit words on the device
 * (which: 0 pk_out16<bf16>, 1 pk_out16<f16>, 2 pk_relu16<bf16>, 3 pk_relu16<f16>, 4 pk_max16_nonneg(w[i], w[i+1])) -- lets a test
 * run the device code of every conv / stem epilogue over all 65,536 patterns (tests/test_gpu_parity.py). */
int flope_debug_pk16(int which, int relu, const void* in_dev, void* out_dev, int n, void* stream);
/* algorithmic FLOPs of one forward for `batch` crops (2*MAC, convs + 2 FCs) */
double flope_forward_flops(flope_handle h, int batch);
/* number of kernel launches flope_forward enqueues */
int flope_forward_launches(flope_handle h);
/* Profile mode (flope_set_option(h, "profile", 1)): flope_forward records a HIP event on the
 * caller's stream before every launch and after the last.  flope_profile_read waits for the
 * last event and writes the GPU time (ms) of each launch of the most recent forward; returns
 * the number written or <0.  flope_launch_info: "layer|kernel" label and algorithmic FLOPs. */
int flope_profile_read(flope_handle h, float* ms_out, int cap);
/* option "profile" = 2: the last forward with its batch slices on their own streams, as in production, as a time line: event i was
 * recorded on slice slice_out[i]'s stream in front of that slice's next launch (behind its last one); ms_out[i] = milliseconds since the
 * fork (event 0).  With "inline0" slice 0's events are recorded on the caller's stream, where that slice runs.  Returns the number of
 * events, < 0 on error.  Developer aid (tools/slice_timeline.py). */
int flope_profile_timeline(flope_handle h, float* ms_out, int* slice_out, int cap);
int flope_launch_info(flope_handle h, int idx, int batch, char* name, int name_cap, double* flops);
/* human-readable launch plan (one line per conv: tile config, patch/gather, LDS bytes) */
int flope_describe_plan(flope_handle h, char* buf, int buflen);
/* what a handle was created with (max_batch, FLOPE_DT_*, crop height / width, device ordinal); any pointer may be NULL */
int flope_engine_geometry(flope_handle h, int* max_batch, int* dtype, int* height, int* width, int* device_id);
/* which kernels the head behind layer4.1 runs on under the handle's current options and backbone_out_dim (flope_amd/csrc/plan.h:
 * head_plan, the rule the launchers themselves ask).  *fc1: 0 fc1_packed_kernel, 1 fc1_kernel (row-major weights), 2 fc1_simple_kernel;
 * *fc2: 0 fc2_procrustes_k4_kernel, 1 fc2_procrustes_kernel with 16-byte loads, 2 the same with the scalar K loop.  Either pointer may
 * be NULL.  (flope_launch_info labels the head's launches "fc1_kernel" / "fc2_procrustes_kernel" whichever ran.) */
int flope_head_plan(flope_handle h, int* fc1, int* fc2);
/* library / build identification */
const char* flope_version(void);
/* A stream restricted to the compute units set in mask[words] (bit i of word i / 32 = CU i in the runtime's enumeration;
 * hipExtStreamCreateWithCUMask).  Used by the live loop to give the detector and the pose network disjoint parts of the chip
 * (FastPosePredictor.iter_flower_poses); any entry point of this library accepts such a stream. */
int flope_stream_create_cu_mask(int device_id, const uint32_t* mask, int words, void** out_stream);
int flope_stream_destroy(int device_id, void* stream);

/* ---- frame -> poses behind the detector (r05) ------------------------------------------------
 * Replaces the body of FastPosePredictor.get_flower_poses AFTER get_bbox_mask (fast_pose_predictor.py:55-56, 60-156): the box
 * loop (squarify_bb / bb_in_frame, mvg.py:324-351), get_depth_value + get_points3d (:88-106), the crop batch (:108-123), the
 * network, procrustes_to_rotmat, nullify_yaw_batch and the [N,4,4] assembly (:125-144), the depth-reliability filter (:97-102).
 * Inputs are the detector's device-resident outputs (flope_yolo_detect: det rows float32 [max_det,8] + count; or any detector's
 * xyxy rows in that layout), the uint8 BGR frame [H,W,3], the uint8 frame mask [H,W] and the depth image (format / divisor as for
 * flope_depth_lift).  Three calls per frame so that several frames can be in flight (one `slot` each):
 *   flope_frame_select   asynchronous: int16 boxes -> squarify -> in-frame filter on the device, in detection order
 *   flope_frame_enqueue  waits on the host for the NUMBER of surviving boxes (4 bytes: grids are sized by the host), then enqueues
 *                        everything else and the copy of the results to pinned host memory; returns that number (0: nothing to do)
 *   flope_frame_finish   waits for the results; poses_out float64 [n,16] row-major 4x4, flowers without reliable depth dropped;
 *                        returns n (0 = the reference's `None`)
 * flope_frame_to_poses = the three in sequence on slot 0.  max_boxes bounds the in-frame boxes of one frame (ultralytics' max_det = 300);
 * a frame with more is refused by flope_frame_enqueue.  More boxes than the engine's max_batch run as several forwards.
 * Call order: enqueue without select, finish without enqueue, or select on a slot that holds an unfinished frame is FLOPE_ESTATE
 * and changes nothing; a failed call leaves the slot idle (and, on a guarded handle, its guard slot un-armed): flope_frame_finish
 * on it is FLOPE_ESTATE and returns no rows, and the next flope_frame_select is accepted.  flope_frame_enqueue refuses
 * depth_div <= 0 and an unknown depth_format itself, before anything is launched.
 * The PoseResNet engine must outlive the frame handle and must not run another forward concurrently. */
typedef struct flope_frame* flope_frame_handle;
int flope_frame_create(flope_handle pose_engine, int frame_h, int frame_w, int max_boxes, int slots, flope_frame_handle* out);
int flope_frame_destroy(flope_frame_handle f);
const char* flope_frame_last_error(flope_frame_handle f);
int flope_frame_select(flope_frame_handle f, int slot, const float* det_dev, const int32_t* count_dev, int max_det, void* stream);
int flope_frame_enqueue(flope_frame_handle f, int slot, const uint8_t* frame_dev, const uint8_t* mask_dev, const void* depth_dev,
                        int depth_format, float depth_div, const float* K4_host, float near_plane, float far_plane, void* stream);
int flope_frame_finish(flope_frame_handle f, int slot, double* poses_out, int cap);
int flope_frame_to_poses(flope_frame_handle f, const float* det_dev, const int32_t* count_dev, int max_det, const uint8_t* frame_dev,
                         const uint8_t* mask_dev, const void* depth_dev, int depth_format, float depth_div, const float* K4_host,
                         float near_plane, float far_plane, double* poses_out, int cap, void* stream);
/* test hook: the boxes flope_frame_select kept, as detected (good_host) and squared (sq_host), int32 [n,4] each; returns n */
int flope_frame_read_boxes(flope_frame_handle f, int slot, int32_t* good_host, int32_t* sq_host, int cap);

/* ---- guarded mode: the f16 trunk, repaired per crop in float32 where the crop's own M is ill-conditioned ------------------------
 * The rotation error of a 16-bit trunk is its error dM of the head output amplified by Procrustes: |dR| gap <= 3 |dM| with
 * gap(M) = s2 + sign(det M) s3 (singular values of M, M's own units).  f16 keeps |dR| <= 1e-3 where gap >= 0.5; the float32 trunk on
 * the exact-fp32 MFMA (option "f32mfma") keeps it everywhere, at a tenth of the rate.  A guard handle borrows one engine of each
 * kind: the whole batch runs in f16, the device computes every crop's gap, and only the crops with !(gap >= gap_min) (a non-finite
 * M included) run again in float32 and overwrite their rows, which are then bit for bit what the float32 engine gives for those
 * crops alone; every other row is the f16 engine's, untouched.
 *   fast: a FLOPE_DT_F16 engine; exact: a FLOPE_DT_F32 engine (the caller sets "f32mfma" on it, or not) with the same device, crop
 *   size and backbone_out_dim; both with weights loaded before the first forward and alive for as long as the guard is.  bf16 is
 *   refused (it would need gap_min = 6.9: every crop repaired).  max_repair <= exact's max_batch: crops per float32 forward (more
 *   flagged crops run as several).  slots (1..16): forwards that may await their repair at the same time.
 *   flope_guard_forward  asynchronous like flope_forward_poses (same arguments; Rt_dev may be NULL as well, at least one output is
 *                        needed): f16 forward into the caller's outputs on `stream`; the selection kernel (gap per crop, index
 *                        list, the NUMBER of flagged crops to pinned host memory, an event) runs behind it on a stream of the
 *                        guard's own, so later work on `stream` does not wait for it.  gap_dev: float32 [batch] or NULL, valid
 *                        once flope_guard_repair has returned.
 *   flope_guard_repair   waits on the host for that number (4 bytes -- the one host wait of the mode, as in flope_frame_enqueue: HIP
 *                        grids are sized on the host).  0: returns 0 and enqueues nothing.  Otherwise enqueues, per max_repair
 *                        crops: gather -> flope_forward_poses(exact) -> scatter into rows idx[i] of r9 / R / Rt; returns the number
 *                        of crops repaired.  x_dev, xyz_dev and the outputs must stay alive and unchanged from forward until
 *                        repair returns; `stream` should be the forward's stream (or one ordered behind it).
 *   flope_guard_forward_repaired = the two in sequence on slot 0.
 * Call order: repair without forward, or forward on a slot that awaits its repair, is FLOPE_ESTATE; a failed call leaves the slot
 * idle.  Repairs share the exact engine and one staging batch: like forwards of one engine they must not run concurrently. */
typedef struct flope_guard* flope_guard_handle;
int flope_guard_create(flope_handle fast, flope_handle exact, int max_repair, int slots, flope_guard_handle* out);
int flope_guard_destroy(flope_guard_handle g);
const char* flope_guard_last_error(flope_guard_handle g);
/* threshold of the selection (default 0.5: the domain tests/test_gpu_parity.py asserts for f16); returns the previous value */
float flope_guard_set_gap_min(flope_guard_handle g, float gap_min);
int flope_guard_forward(flope_guard_handle g, int slot, const void* x_dev, int in_format, int batch, const float* xyz_dev, int nullify_yaw,
                        float* r9_dev, float* R_dev, float* Rt_dev, float* gap_dev, void* stream);
int flope_guard_repair(flope_guard_handle g, int slot, void* stream);
int flope_guard_forward_repaired(flope_guard_handle g, const void* x_dev, int in_format, int batch, const float* xyz_dev, int nullify_yaw,
                                 float* r9_dev, float* R_dev, float* Rt_dev, float* gap_dev, void* stream);
/* test hook: the crops the slot's last repair found flagged, ascending, int32 [n]; returns n */
int flope_guard_read_selection(flope_guard_handle g, int slot, int32_t* idx_host, int cap);
/* test hook: guard_select_kernel exactly as flope_guard_forward launches it (one workgroup of 256 threads), on a caller's
 * M_dev [n, 9] with threshold gap_min, on `stream`.  gap_dev: float32 [n] (may be NULL); sel_dev: int32 [1 + n] -- the number of
 * flagged rows, then their indices in ascending order.  Waits for the kernel; returns the number of flagged rows (the value the
 * kernel stored to mapped host memory, as flope_guard_repair reads it), or < 0.  Needs no handle. */
int flope_guard_select_rows(const float* M_dev, int n, float gap_min, float* gap_dev, int32_t* sel_dev, void* stream);
/* flope_frame_* over a guard: slot i of the frame uses slot i of the guard (slots <= the guard's).  Crops are float32 NCHW;
 * flope_frame_enqueue calls flope_guard_forward, flope_frame_finish runs flope_guard_repair before it reads the poses (its host
 * wait is where the guard's belongs); a frame with more boxes than the f16 engine's max_batch repairs all but its last forward
 * inside flope_frame_enqueue. */
int flope_frame_create_guarded(flope_guard_handle g, int frame_h, int frame_w, int max_boxes, int slots, flope_frame_handle* out);
/* test hook (guarded frame handles): gap of every crop of the slot's last finished frame, float32 [n]; returns n */
int flope_frame_read_gaps(flope_frame_handle f, int slot, float* gap_host, int cap);

/* ---- Multi-frame tracker on the device (reference sunflower/predictor/flower_model.py:146-213) ----
 * FlowerModel.assign_meas_to_state with its state in device memory: world pose = camera pose x flower pose, measurement =
 * [translation | scalar-last quaternion], nearest ANCHOR (a track's first measurement, never overwritten) under the gate
 * dist_th_m (d < dist_th_m matches), one identity-model Kalman filter per track as the scalar recursion
 *     p += q;  k = p / (p + r);  x += k (z - x);  p = (1 - k)^2 p + k^2 r;  quaternion part divided by its norm
 * (all float64, csrc/track_math.h).  Within a frame every distance goes to the anchors as they stood at the start of the frame,
 * a track opened in a frame is invisible to the rest of it, two measurements may update one track (in measurement order), and
 * new tracks get their indices in measurement order.
 *   _create   max_tracks >= 1, max_meas >= 1, dist_th_m, q, r and p0 finite and positive; otherwise FLOPE_EINVAL.
 *   _update   asynchronous on `stream`, ordered behind the handle's previous update whatever stream that used (an event of the
 *             handle).  Rt_dev [n,16] row-major 4x4 poses in the camera frame, float32 (rt_f64 = 0, widened exactly) or float64
 *             (rt_f64 = 1); rel_dev int32 [n] or NULL = all reliable; rows with rel == 0 are skipped; cam16_host: row-major 4x4
 *             camera pose, read before the call returns.  n = 0 is a no-op, n > max_meas is FLOPE_EINVAL and enqueues nothing.
 *             Two launches, no allocation, no host wait.  An update that would open more than max_tracks tracks applies
 *             nothing of its frame and sets a flag that stays until _reset: later updates apply nothing either, and _count,
 *             _read and _read_assoc return FLOPE_ESTATE.
 *   _count    waits for the last update; the number of tracks.
 *   _read     waits; anchors / means float64 [tracks,7], p float64 [tracks], hits int32 [tracks] (any may be NULL); returns the
 *             number of tracks, FLOPE_EINVAL when it exceeds cap.
 *   _read_assoc  test hook: the last update's association, int32 [n]: >= 0 the matched track, -1 - t = opened track t,
 *             INT32_MIN = skipped as unreliable; returns n, FLOPE_ESTATE before the first update.
 *   _reset    waits, then empties the state and clears the flag.
 *   _debug_sentinels  test hook: waits; how many of the sentinel words behind the state arrays have changed (0 is right). */
typedef struct flope_track* flope_track_handle;
int flope_track_create(int device_id, int max_tracks, int max_meas, double dist_th_m, double q, double r, double p0, flope_track_handle* out);
int flope_track_destroy(flope_track_handle t);
const char* flope_track_last_error(flope_track_handle t);
int flope_track_reset(flope_track_handle t);
int flope_track_update(flope_track_handle t, const void* Rt_dev, int rt_f64, const int32_t* rel_dev, int n, const double* cam16_host, void* stream);
int flope_track_count(flope_track_handle t);
int flope_track_read(flope_track_handle t, double* anchors, double* means, double* p, int32_t* hits, int cap);
int flope_track_read_assoc(flope_track_handle t, int32_t* assoc_host, int cap);
int flope_track_debug_sentinels(flope_track_handle t);
/* test hook: waits; the first `rows` rows of every state array as they are in device memory and count2 = {tracks, overflow flag},
 * whatever the flag says (what an update that overflowed has left behind); returns rows */
int flope_track_debug_read(flope_track_handle t, double* anchors, double* means, double* p, int32_t* hits, int32_t* count2, int rows);
/* What a consumer on the device needs of the handle's state behind its last update (flope_tf_stream_step_tracker): device
 * pointers that stay valid until _destroy, the event a reader's stream must wait for, and host-side counts.  Enqueues nothing and
 * waits for nothing.  n: the measurements of the last update, -1 when there was none since _create / _reset.  serial: counts the
 * updates of the handle that enqueued anything (n > 0), from 1; it is kept on the host and never reset, so two views with one
 * serial speak of the same update.  The arrays are overwritten by the next update: a reader orders that update behind itself. */
typedef struct flope_track_view {
  const int32_t* assoc;        /* [max_meas]: the last update's association (flope_track_read_assoc's encoding) */
  const double* meas;          /* [max_meas][7]: its measurements, world position then quaternion x y z w; rows the update skipped are stale */
  const double* means;         /* [max_tracks][7]: the filtered means */
  const int32_t* count;        /* [2]: tracks, overflow flag */
  void* event;                 /* a hipEvent_t recorded behind every update */
  int device, max_tracks, max_meas, n;
  unsigned long long serial;
} flope_track_view;
int flope_track_device_view(flope_track_handle t, flope_track_view* out);
/* The slot's device-resident poses and depth-reliability flags (the rows flope_frame_finish would return) into the tracker,
 * behind the slot's pose kernels on the slot's stream, without a host wait.  Legal between a flope_frame_enqueue that returned
 * n > 0 and that slot's flope_frame_finish; a slot whose enqueue returned 0 is a no-op returning 0; an idle slot is FLOPE_ESTATE; a
 * guarded frame handle is FLOPE_EINVAL (the guard's repairs land in flope_frame_finish). */
int flope_frame_track(flope_frame_handle f, int slot, flope_track_handle t, const double* cam16_host);

/* ---- TransformerEncoder (reference scripts/tf_encoder.py:5-27) -------------
 * Replaces `TransformerEncoder(input_dim, model_dim, out_dim, num_heads, num_layers, ff_dim,
 * dropout)` + `.load_state_dict()` + `forward(x)` in eval mode (dropout = identity):
 *   embedding Linear -> num_layers x post-norm nn.TransformerEncoderLayer (ReLU, batch_first,
 *   no mask, no positional encoding) -> out_layer Linear.
 * dtype FLOPE_DT_F32: fp32 everywhere (any dimensions).  FLOPE_DT_F16 / BF16: 16-bit activations,
 * fp32 accumulation; linears with N % 128 == 0 and K % 64 == 0 and attention with head_dim 64
 * (seq_len <= 512) run on MFMA, everything else on generic kernels.  With flope_tf_set_option(h, "attn_tiled", 1) attention with
 * head_dim 32 / 64 / 96 / 128 runs on MFMA at any seq_len (tf_attn_tiled streams K and V through LDS in 64-key blocks).
 * FLOPE_DT_F32 with flope_tf_set_option(h, "f32mfma", 1): the same float32 buffers and launch sequence, every linear with
 * K % 4 == 0 and every attention with head_dim % 4 == 0, head_dim <= 128 and 16 score rows of seq_len floats within 160 KiB of LDS
 * on v_mfma_f32_16x16x4_f32 (exact float32 products and sums: differs from the strict mode in summation order only); the other
 * ops of the handle stay on the generic kernels, LayerNorm is unchanged.
 * max_tokens bounds batch*seq_len of any later forward (the token count of a ragged one).  Same ownership / error rules as above. */
typedef struct flope_tf_encoder* flope_tf_handle;
int flope_tf_create(int device_id, int input_dim, int model_dim, int out_dim, int num_heads,
                    int num_layers, int ff_dim, int max_tokens, int dtype, flope_tf_handle* out);
int flope_tf_destroy(flope_tf_handle h);
const char* flope_tf_last_error(flope_tf_handle h);
/* names as in the reference module's state_dict(): embedding.{weight,bias},
 * transformer_encoder.layers.<i>.{self_attn.in_proj_weight, self_attn.in_proj_bias,
 * self_attn.out_proj.{weight,bias}, linear1.*, linear2.*, norm1.*, norm2.*}, out_layer.* */
int flope_tf_load_weights(flope_tf_handle h, int n, const char* const* names,
                          const float* const* host_ptrs, const int* ndims,
                          const int64_t* const* shapes);
/* x_dev float32 [batch, seq_len, input_dim] -> y_dev float32 [batch, seq_len, out_dim] */
int flope_tf_forward(flope_tf_handle h, const float* x_dev, int batch, int seq_len, float* y_dev,
                     void* stream);
/* returns the previous value, or <0 (FLOPE_EINVAL for an unknown name)
 *   "generic" (default 0): 1 forces the generic kernels on 16-bit handles (A/B checks);
 *   "f32mfma" (default 0): FLOPE_DT_F32 handles run every eligible linear and attention on the exact-fp32 MFMA kernels
 *       (tf_linear_f32m, tf_attn_f32m) instead of the generic ones; may be flipped between forwards (flope_tf_load_weights on a
 *       float32 handle uploads both weight images).  Stored and ignored by FLOPE_DT_F16 / BF16 handles;
 *   "f32mlds" (default 0; 0 .. 160): KiB of untouched LDS every tf_linear_f32m launch reserves; more than 80 leaves one
 *       workgroup per CU (measurement knob: DESIGN.md 16);
 *   "attn_tiled" (default 0; 0 .. 2, FLOPE_EINVAL outside): which 16-bit attention launches take the streaming MFMA kernel
 *       tf_attn_tiled (head_dim % 32 == 0, head_dim <= 128, any seq_len).  0: none.  1: those that would otherwise run
 *       the generic kernel; shapes the resident kernel takes (head_dim 64, seq_len <= 512) keep it.  2: every eligible launch, also in
 *       place of the resident kernel (A/B and tests).  "generic" = 1 overrides it; buffers that are not 16-byte aligned run generic.
 *       May be flipped between forwards.  Stored and ignored by FLOPE_DT_F32 handles;
 *   "fused" (default 0; 0 or 1, FLOPE_EINVAL outside): 1 = a FLOPE_DT_F32 forward whose longest sequence fits one workgroup's 64 KiB
 *       of LDS (flope_amd/csrc/tf_fused_plan.h) runs as ONE launch, one sequence per workgroup (tf_fused_f32), and
 *       returns the bits of the launch sequence; any other forward runs that sequence, silently.  Stored and ignored by 16-bit
 *       handles and while "f32mfma" = 1; may be flipped between forwards; flope_tf_attention / _linear / _layernorm ignore it;
 *   "causal" (default 0; 0 or 1, FLOPE_EINVAL outside): 1 = query i attends to keys j <= i of its own sequence (torch's
 *       mask = generate_square_subsequent_mask(seq_len)) in flope_tf_forward, _forward_varlen (causal inside each
 *       sequence; rows behind a sequence still come back as out_layer.bias, never read -- torch computes something there once a mask
 *       is given), _attention and _attention_varlen.  Every dtype and every attention kernel has the form, "fused" included; the
 *       kernel a shape picks, its grid, block and LDS (and so flope_tf_forward_plan's answer) are those of the option at 0, and
 *       keys above the diagonal are skipped, not loaded and masked.  flope_tf_forward_flops / _flops_varlen count attention as
 *       num_layers model_dim sum len (len + 1) MACs under it.  Row i of a causal forward depends on rows <= i only: the forward of a
 *       prefix is the prefix of the forward, bit for bit.  May be flipped between calls.  The only other [L, L] mask with a form
 *       is the banded causal one of "window";
 *   "window" (default 0; FLOPE_EINVAL below 0; returns the old value, as the others do): W >= 1 together with "causal" = 1 is
 *       sliding-window causal attention: query i attends to keys j of its own sequence with i - W < j <= i, torch's
 *       banded [L, L] mask.  0 = no window.  Honoured only with "causal" = 1: with "causal" = 0 and W > 0, flope_tf_forward,
 *       _forward_varlen, _forward_plan, _attention and _attention_varlen return FLOPE_EINVAL with a message (a window without causal
 *       is refused).  With lengths the window lies inside each packed sequence; rows behind a sequence keep coming back as
 *       out_layer.bias.  Under a window, with "window_mfma" = 0, EVERY attention launch is tf_attn_generic (its WINDOW instantiation,
 *       whatever the dtype and shape: flope_tf_attention* return FLOPE_TF_ATTN_GENERIC), keys outside the window are not loaded, the forward is always the
 *       launch sequence (flope_tf_forward_plan answers FLOPE_TF_FWD_LAUNCHES, "fused" is not taken), and flope_tf_forward_flops /
 *       _flops_varlen count attention over sum_t min(t + 1, W) keys per sequence.  W >= seq_len gives the bits of the generic causal
 *       kernel.  Windows inside tf_attn_f32m and tf_fused_f32 are a follow-up;
 *   "window_mfma" (default 0; 0 or 1, FLOPE_EINVAL outside; returns the old value; stored and ignored by float32 handles, as
 *       "attn_tiled" is): 1 = under "causal" = 1 and "window" > 0 a 16-bit launch whose pick without a window is tf_attn_mfma or
 *       tf_attn_tiled stays on that kernel, its WINDOW instantiation: same grid, block and LDS, a wave starts at the
 *       32-key step that holds its first query's first visible key, tf_attn_tiled does not load the 64-key blocks below the
 *       workgroup's window, and flope_tf_attention* return FLOPE_TF_ATTN_MFMA64 / _TILED.  Every other launch under a window
 *       (float32, option "generic", head dims without such a kernel, misaligned buffers) stays tf_attn_generic.  W >= seq_len gives
 *       the bits of the same kernel under "causal" alone.  flope_tf_stream_step is untouched (tf_attn_step, the generic order), so
 *       its rows equal the windowed forward's in bits where that forward's attention is tf_attn_generic and within the MFMA
 *       kernels' tolerances elsewhere; _prefill stays the ragged windowed forward in bits.  With 0 every launch is as above;
 *   "step_split" (default 0; 0 or 1, FLOPE_EINVAL outside; returns the old value; honoured by every dtype): 1 =
 *       flope_tf_stream_step and _extend compute a token's attention with its visible keys split over the four waves of a workgroup
 *       (tf_attn_step_split / tf_attn_extend_split) where the head slice is a power-of-two count of 16-byte vectors
 *       (tf_step_split_ok: head_dim 8, 32, 64, 128 in every dtype); other shapes keep tf_attn_step / tf_attn_extend and their bits.
 *       The result is then NOT the causal forward's bits: it is a deterministic function of the track's own keys, element-wise
 *       within a derived bound of fp64, and every invariant among _step, _extend, ring capacity and the call's other tracks stays
 *       bit-exact.  Read when a call enqueues, so it may be flipped between calls on one state (the cache layout is the same).
 *       _prefill, the forwards, flope_tf_attention and option "fused" neither read nor are changed by it;
 *   "extend_mfma" (default 0; 0 or 1, FLOPE_EINVAL outside; returns the old value; stored and ignored by float32 handles): 1 =
 *       flope_tf_stream_extend computes its attention with tf_attn16_extend where tf_extend_mfma_ok: a 16-bit dtype and
 *       head_dim 32 / 64 / 96 / 128 -- tf_attn_tiled's LDS ring and 32-key MFMA step over the track's cache and then the call's chunk,
 *       in the absolute 32-key steps of the whole track, on linear and windowed states alike.  Its rows are then, bit for bit, rows
 *       position .. position + length - 1 of the causal (windowed) forward of the track where that forward's attention is
 *       tf_attn_mfma / tf_attn_tiled (under a window: with "window_mfma" = 1), for any split of the track into chunks, and the cache
 *       it leaves is _prefill's.  Other shapes keep the choice below it ("step_split"'s kernel, or tf_attn_extend) and their bits; it
 *       takes precedence over "step_split" for _extend only.  Read when a call enqueues, so it may be flipped between calls on one
 *       state (the cache layout is the same).  _step, _prefill, the forwards, flope_tf_attention and flope_tf_stream_attention
 *       neither read nor are changed by it.  Stale cache rows are still never read (NaN included).  A NaN the caller FEEDS as a token
 *       is a real key, and in a matrix product a masked probability of 0 does not hide it: a query is NaN when such a key lies in
 *       one of the 32-key steps its wave of 32 chunk rows takes (those from the step of the wave's first query's first visible key
 *       to the step of its last query), at or above the first key its workgroup of 128 chunk rows sees and below position + length
 *       -- a key below the query's own window, or a later token of the same chunk, included.  Fed one token per call, a ring
 *       forgets NaN tokens as fast as under option 0;
 *   "mask_mfma" (default 0; 0 or 1, FLOPE_EINVAL outside; returns the old value; stored and ignored by float32 handles): 1 = attention
 *       under a compiled mask (flope_tf_forward_masked / flope_tf_attention_masked, fixed and ragged) runs tf_attn_tiled_masked
 *       (FLOPE_TF_ATTN_MASKED16 = 5) where tf_attn_pick_masked says so: a 16-bit dtype, "generic" = 0, head_dim 32 / 64 /
 *       96 / 128 and 16-byte aligned buffers -- tf_attn_tiled's LDS ring and 32-key MFMA step over the key blocks of the mask's tile
 *       map; "attn_tiled" is not consulted.  Other handles and shapes keep tf_attn_masked and its bits.  The result is then NOT
 *       tf_attn_masked's bits: where the mask is all-clear, causal, a causal band or block-diagonal at multiples of 32 it is
 *       tf_attn_tiled's for that pattern, bit for bit (the band: with "window_mfma" = 1), every other mask is held element-wise
 *       within a derived bound of fp64.  A key that no query of the sequence allows is still never read into a product (NaN there
 *       reaches no output); a key that holds NaN and is allowed by SOME query of a 128-row query block makes every row of that block
 *       that takes its 32-key step NaN, the rows that mask it included.  Read when a call enqueues, so it may be flipped between
 *       calls; every mask carries its tile map, a forward builds and allocates nothing.  No other call reads or is changed by it;
 *   "bias_mfma" (default 0; 0 or 1, FLOPE_EINVAL outside; returns the old value; stored and ignored by float32 handles): 1 = attention
 *       under a compiled BIAS (flope_tf_bias_create; fixed and ragged) runs the BIASED instantiation of tf_attn_tiled_masked
 *       (FLOPE_TF_ATTN_BIASED16 = 7) where tf_attn_pick_biased says so: a 16-bit dtype, "generic" = 0, head_dim 32 / 64 /
 *       96 / 128 (every head_dim whose instantiation was built without scratch: all four) and 16-byte aligned buffers -- the walk of
 *       "mask_mfma" over the tile map of the bias's allowed set with one fma per score, fma(bias, log2e, fl(s scale log2e)).  An option
 *       of its own: "mask_mfma" has no say over a bias, "bias_mfma" none over a plain mask.  Other handles and shapes keep
 *       FLOPE_TF_ATTN_BIASED and its bits.  The result is NOT tf_attn_masked's bits: an all-zero bias gives the bits of the compiled
 *       mask of its allowed set under "mask_mfma" = 1, every other bias is held element-wise within a derived bound of fp64.  A seq_len
 *       too long for tf_attn_masked's score rows is accepted where the pick is 7.  The bias entry of a masked pair may be LOADED
 *       (it is -inf) and is never USED; a key that no query of the sequence allows is never read into a product, as under
 *       "mask_mfma", with the same rule for a NaN key that some query of a 128-row block allows.  Read when a call enqueues; every
 *       bias carries its tile map on the device behind its planes, a forward builds and allocates nothing;
 *   "skinny" (default 0; 0 or 1, FLOPE_EINVAL outside; returns the old value; stored and ignored by float32 handles): 1 = a linear
 *       that would run tf_gemm_mfma (FLOPE_TF_LIN_MFMA) on 1 .. 32 rows runs tf_gemm_skinny instead (FLOPE_TF_LIN_SKINNY = 5;
 *       DESIGN.md 48): one wave per 16-row feature tile of the same packed weights (N / 16 workgroups of 64 lanes where tf_gemm_mfma
 *       has N / 128 of 256), the operands loaded from global memory straight into registers, no LDS.  Each output element takes the
 *       same MFMAs over the same operands in the same order, so rows < `rows` hold tf_gemm_mfma's BITS: the option changes no result
 *       of any call.  Every caller of a linear takes it with no setting of its own: flope_tf_forward* at batch * seq_len <= 32,
 *       flope_tf_stream_step / _step_assoc / _step_tracker / _extend / _prefill at that many rows, flope_tf_linear.  Reads token and
 *       residual rows 0 .. 15 (rows <= 16) or 0 .. 31 only, which lie inside the roundup(rows, 128) rows tf_gemm_mfma requires, and
 *       writes those rows only: rows `rows` .. 15 / 31 of the result may hold anything, as under 0, later rows are left alone.  More
 *       than 32 rows, option "generic", float32 results and unpacked linears keep their kernel.  Read when a call enqueues;
 *   "skinny_ln" (default 0; 0 or 1, FLOPE_EINVAL outside; returns the old value; stored and ignored wherever the rule below says no,
 *       option "skinny" at 0 and float32 handles included): 1 = a LayerNorm of the forward that stands directly in front of a linear
 *       option "skinny" takes -- a layer's first in front of its linear1, its second in front of the next layer's in_proj -- is not
 *       launched; the linear runs as tf_gemm_skinny_ln (FLOPE_TF_LIN_SKINNY_LN = 6), which normalises the pre-norm rows
 *       in its token load, stores the post-norm rows and runs tf_gemm_skinny's MFMAs: rows < `rows` of both results hold the BITS of
 *       the two launches, so the option changes no result of any call; it takes 2 num_layers - 1 launches out of a forward.  The
 *       rule: option "skinny" takes the linear (1 .. 32 rows), K = model_dim, model_dim % 64 == 0 and model_dim <= 512.  The last
 *       LayerNorm (in front of out_layer) keeps its launch.  flope_tf_last_ln counts both.  Read when a call enqueues.  Under
 *       "norm_first" both LayerNorms of every layer stand in front of such a linear: all 2 num_layers are folded;
 *   "norm_first" (default 0; 0 or 1), "activation" (default FLOPE_TF_ACT_RELU = 1; 1 or FLOPE_TF_ACT_GELU = 2, torch's "gelu": the
 *       erf form) and "final_norm" (default 0; 0 or 1): the architecture (flope_amd/csrc/tf_arch_plan.h) -- torch's
 *       nn.TransformerEncoderLayer(norm_first=, activation=) and nn.TransformerEncoder(norm=LayerNorm).  Another value is
 *       FLOPE_EINVAL.  Stated BEFORE the weights are loaded: once flope_tf_load_weights has succeeded they return FLOPE_ESTATE.
 *       With "final_norm" the state_dict must hold transformer_encoder.norm.weight / .bias [model_dim].  Every forward, ragged,
 *       causal, windowed, masked and biased, and every stream call runs the architecture; option "fused" is stored and ignored
 *       under any but the default one (the forward is the launch sequence).  The defaults are the handle of before: the same
 *       launches, kernels and bits. */
#define FLOPE_TF_ACT_RELU 1
#define FLOPE_TF_ACT_GELU 2
int flope_tf_set_option(flope_tf_handle h, const char* name, int value);
/* softmax(q k^T / sqrt(head_dim)) v per head on a caller's buffer: qkv_dev [batch, seq_len, 3*model_dim] and out_dev
 * [batch, seq_len, model_dim] in the handle's dtype (float32 for FLOPE_DT_F32).  Launches exactly what flope_tf_forward
 * would launch for this (batch, seq_len) under the handle's current options; needs no weights.  Returns the
 * FLOPE_TF_ATTN_* id of the kernel launched (flope_amd/csrc/tf_attn_plan.h: 0 generic, 1 tf_attn_mfma, 2 tf_attn_tiled,
 * 3 tf_attn_f32m), or < 0.  batch*seq_len <= max_tokens. */
int flope_tf_attention(flope_tf_handle h, const void* qkv_dev, int batch, int seq_len, void* out_dev, void* stream);
/* algorithmic FLOPs of one forward (2*MAC: linears + QK^T + PV), attention counted over the keys options "causal" / "window" leave */
double flope_tf_forward_flops(flope_tf_handle h, int batch, int seq_len);
/* One loaded linear on a caller's buffers: y = act(x W^T + b (+ res)), x_dev [rows, K] -> y_dev [rows, N], res_dev [rows, N] or NULL,
 * relu != 0: ReLU behind the residual.  name: "embedding", "out_layer", "layers.<i>.in_proj", ".out_proj", ".linear1", ".linear2".
 * Launches exactly what flope_tf_forward launches for that linear at this row count under the handle's current options and
 * returns the FLOPE_TF_LIN_* id of the kernel, or < 0 and nothing launched.  Needs loaded weights (FLOPE_ESTATE) and
 * rows <= max_tokens.  FLOPE_DT_F16 / BF16 handles: x_dev is float32 where x_f32 != 0 (the network input; with the MFMA linear only
 * for "embedding", whose 16-bit copy the handle holds), y_dev is float32 where y_f32 != 0, res_dev is always 16-bit.  An MFMA linear
 * with K % 64 != 0 (an "embedding" of such an input_dim) reads rows of roundup(K, 64) zero-padded columns, which only that copy
 * has: it takes x_f32 != 0, a 16-bit x_dev is FLOPE_EINVAL.  Two contracts:
 *   padded rows   tf_gemm_mfma (FLOPE_TF_LIN_MFMA) takes no row count: it reads x_dev and res_dev and writes y_dev in whole
 *                 128-row tiles.  All three must be allocated for roundup(rows, 128) rows; rows >= `rows` of x_dev and res_dev may
 *                 hold anything (NaN included) and never reach a row < `rows`; rows >= `rows` of y_dev are overwritten.  The
 *                 library cannot check an allocation's size: the caller's duty (flope_amd.TransformerEncoder.linear does it).
 *   alignment     x_dev, res_dev and y_dev 16-byte aligned, otherwise FLOPE_EINVAL (the 16-bit kernels load and store 16 bytes).
 * FLOPE_DT_F32 handles: all buffers float32 (x_f32 / y_f32 ignored), aligned to 4 bytes; a pointer that is not 16-byte aligned is
 * legal and sends an f32mfma linear to the generic kernel.  ReLU and residual together have no tf_linear_f32m form (FLOPE_EINVAL). */
#define FLOPE_TF_LIN_GENERIC      0   /* tf_linear_generic: any shape */
#define FLOPE_TF_LIN_ROWWAVE      1   /* tf_linear_rowwave: N <= 16, no residual */
#define FLOPE_TF_LIN_ROWWAVE_VEC  2   /* tf_linear_rowwave_vec: 16-bit input, N <= 16, K % 8 == 0, N K floats within 48 KiB of LDS */
#define FLOPE_TF_LIN_MFMA         3   /* tf_gemm_mfma: 16-bit, N % 128 == 0, K % 64 == 0 (embedding: K zero-padded) */
#define FLOPE_TF_LIN_F32M         4   /* tf_linear_f32m: float32, option f32mfma, K % 4 == 0 */
#define FLOPE_TF_LIN_SKINNY       5   /* tf_gemm_skinny: option skinny, where tf_gemm_mfma would run on 1 .. 32 rows; its bits (rows 0 .. 15 / 31 touched only) */
int flope_tf_linear(flope_tf_handle h, const char* name, const void* x_dev, int x_f32, const void* res_dev, void* y_dev, int y_f32,
                    int rows, int relu, void* stream);
/* flope_tf_linear with the activation named: act = 0 (none), FLOPE_TF_ACT_RELU or FLOPE_TF_ACT_GELU (tf_gelu_f32 of
 * flope_amd/csrc/tf_act.h on the float32 accumulator, in front of the store).  The same kernel id as relu != 0 gives.
 * Another act, or GELU together with res_dev, is FLOPE_EINVAL and launches nothing. */
int flope_tf_linear_act(flope_tf_handle h, const char* name, const void* x_dev, int x_f32, const void* res_dev, void* y_dev, int y_f32,
                        int rows, int act, void* stream);
/* The FLOPE_TF_LIN_* id flope_tf_linear would return for linear `name` at `rows` rows under the handle's current options, in the form
 * flope_tf_forward runs that linear: "embedding" with a float32 input, "out_layer" with a float32 result, ".out_proj" and ".linear2"
 * with a residual, ".linear1" with the handle's activation, all buffers aligned.  Launches nothing and touches no buffer.  The same refusals: weights not
 * loaded (FLOPE_ESTATE), an unknown name, rows < 1 or rows > max_tokens (FLOPE_EINVAL). */
int flope_tf_linear_plan(flope_tf_handle h, const char* name, int rows);
/* The forward's launch of a LayerNorm together with the linear behind it (option "skinny_ln") on a caller's buffers:
 * normed_dev [rows, model_dim] = LayerNorm(x_dev [rows, model_dim]; gamma_dev, beta_dev float32 [model_dim], eps 1e-5) and
 * y_dev [rows, N] = act(normed W^T + b) of linear `name`, all three in the handle's 16-bit dtype, relu != 0: ReLU.  Returns
 * FLOPE_TF_LIN_SKINNY_LN, or < 0 and nothing launched: FLOPE_EINVAL wherever the option's rule says no for this handle, linear and row
 * count (flope_tf_linear_ln_plan tells without an error).  The buffer rules of flope_tf_linear: x_dev, normed_dev and y_dev 16-byte
 * aligned (gamma_dev and beta_dev too) and allocated for roundup(rows, 128) rows; the launch reads rows 0 .. 15 (rows <= 16) or 0 .. 31
 * of x_dev and writes those rows of normed_dev and y_dev only; rows >= `rows` of x_dev may hold anything (NaN included), which reaches
 * those rows of the results only.  x_dev, normed_dev and y_dev must not overlap (FLOPE_EINVAL). */
#define FLOPE_TF_LIN_SKINNY_LN    6   /* tf_gemm_skinny_ln: option skinny_ln, a LayerNorm and the skinny linear behind it in one launch; the bits of the two */
int flope_tf_linear_ln(flope_tf_handle h, const char* name, const void* x_dev, const float* gamma_dev, const float* beta_dev, void* normed_dev,
                       void* y_dev, int rows, int relu, void* stream);
/* flope_tf_linear_ln with the activation named, as flope_tf_linear_act names it */
int flope_tf_linear_ln_act(flope_tf_handle h, const char* name, const void* x_dev, const float* gamma_dev, const float* beta_dev, void* normed_dev,
                           void* y_dev, int rows, int act, void* stream);
/* FLOPE_TF_LIN_SKINNY_LN where flope_tf_linear_ln would launch for linear `name` at `rows` rows under the handle's current options,
 * otherwise the FLOPE_TF_LIN_* id of the linear of the separate form (no residual; ".linear1" with the handle's activation).  Launches nothing. */
int flope_tf_linear_ln_plan(flope_tf_handle h, const char* name, int rows);
/* The LayerNorms of the last forward of any kind that went through the per-kernel launches (flope_tf_forward*, flope_tf_stream_step* /
 * _extend / _prefill): *launched stand-alone launches, *folded run inside the next linear's launch (option "skinny_ln").  Either
 * pointer may be NULL.  (0, 0) before the first forward. */
int flope_tf_last_ln(flope_tf_handle h, int* launched, int* folded);
/* The LayerNorm flope_tf_forward runs for this handle's dtype and model_dim (eps 1e-5, biased variance) on a caller's buffers:
 * in_dev [rows, model_dim] -> out_dev [rows, model_dim] in the handle's dtype, gamma_dev / beta_dev device float32 [model_dim].
 * Needs no weights.  Returns the FLOPE_TF_LN_* id of the kernel, or < 0 and nothing launched.  rows <= max_tokens; 16-bit handles
 * take in_dev and out_dev 16-byte aligned (FLOPE_EINVAL otherwise), float32 handles 4-byte aligned.  Only `rows` rows are touched. */
#define FLOPE_TF_LN_SCALAR        0   /* tf_layernorm: any model_dim, float32 handles always */
#define FLOPE_TF_LN_VEC           1   /* tf_layernorm_vec: 16-bit, model_dim % 8 == 0 and <= 2048 */
int flope_tf_layernorm(flope_tf_handle h, const void* in_dev, void* out_dev, const float* gamma_dev, const float* beta_dev, int rows,
                       void* stream);
/* Ragged batches: x_dev float32 [batch, seq_len, input_dim] whose sequence b consists of rows 0 .. lengths_host[b] - 1,
 * 1 <= lengths_host[b] <= seq_len (nn.TransformerEncoder's src_key_padding_mask for right-padded batches).  Rows behind a sequence are
 * padding: never read, they may hold NaN.  y_dev float32 [batch, seq_len, out_dim] is fully written: rows < lengths_host[b] are the
 * encoder applied to that sequence alone, bit for bit what flope_tf_forward gives it at (1, lengths_host[b]); rows behind them hold
 * out_layer.bias (what the reference module returns there).  Inside the handle the batch is T = sum of lengths packed tokens:
 * padding costs no FLOPs and no bytes behind the input gather, and the limit is T <= max_tokens (batch*seq_len may exceed it).
 * lengths_host is a host array of batch ints (grid sizes and the kernel choice need its maximum and its sum); it is read before the
 * call returns.  One attention kernel per launch, chosen for the longest sequence.  FLOPE_EINVAL for batch < 1, a length of 0 (torch
 * returns NaN there; this library does not), a length > seq_len, or T > max_tokens.  All options keep their meaning. */
int flope_tf_forward_varlen(flope_tf_handle h, const float* x_dev, int batch, int seq_len, const int* lengths_host, float* y_dev,
                            void* stream);
/* flope_tf_attention for a ragged batch: packed qkv_dev [T, 3*model_dim] -> packed out_dev [T, model_dim] in the handle's dtype,
 * sequence b = rows sum(lengths_host[0 .. b-1]) onwards.  Launches exactly what flope_tf_forward_varlen would for these lengths under
 * the handle's current options; needs no weights.  Returns the FLOPE_TF_ATTN_* id of the kernel launched, or < 0.  T <= max_tokens. */
int flope_tf_attention_varlen(flope_tf_handle h, const void* qkv_dev, int batch, const int* lengths_host, void* out_dev, void* stream);
/* What flope_tf_forward (lengths_host NULL) or flope_tf_forward_varlen (lengths_host: batch ints) of this shape would run under the
 * handle's current options: FLOPE_TF_FWD_LAUNCHES, the sequence of 2 + 7 num_layers kernels (also for an empty fixed-length batch,
 * which runs nothing), or FLOPE_TF_FWD_FUSED, the single launch of option "fused".  < 0 for the argument errors the forward itself
 * reports (buffers aside).  Enqueues nothing and leaves the handle's state alone. */
#define FLOPE_TF_FWD_LAUNCHES     0
#define FLOPE_TF_FWD_FUSED        1
int flope_tf_forward_plan(flope_tf_handle h, int batch, int seq_len, const int* lengths_host);
/* What the last flope_tf_forward / flope_tf_forward_varlen of this handle that passed its checks enqueued: FLOPE_TF_FWD_FUSED when the
 * single launch ran, FLOPE_TF_FWD_LAUNCHES otherwise (also before any forward).  Recorded by the forward itself, not planned again. */
int flope_tf_last_forward(flope_tf_handle h);
/* algorithmic FLOPs of one ragged forward: the linears on T tokens, attention on the sum of lengths squared; 0 for an invalid batch */
double flope_tf_forward_flops_varlen(flope_tf_handle h, int batch, const int* lengths_host);
/* Streaming causal forward: one new token per track and call instead of the whole track again.  A stream state owns
 * the keys and values every layer has seen of `tracks` tracks, up to `capacity` tokens each: ONE device allocation
 * [num_layers][tracks][capacity][2*model_dim] in the handle's dtype (float for FLOPE_DT_F32, with or without "f32mfma"), a row being
 * k followed by v.  capacity <= 4096 (kTfStreamMaxCapacity of flope_amd/csrc/tf_encoder_stream.h: the step kernel keeps one score per
 * key in 64 KiB of LDS); outside that, or tracks < 1: FLOPE_EINVAL.  A failed allocation is FLOPE_EHIP and the message names the
 * size.  A handle may have several states, each with its own cache; they share the handle's scratch buffers, as forwards do, and
 * end with the handle: after flope_tf_destroy every call on a state but _close returns FLOPE_ESTATE.
 * How many tokens a track holds (its position) lives on the host, in the state: _step and _prefill check it there and advance it
 * when they enqueue, _reset only clears it (stale cache rows are never read), _position returns it.  So the CALLS ON ONE STATE MUST
 * BE ORDERED ON ONE STREAM BY THE CALLER, and forwards of the handle that run between them on that stream or a synchronised one.
 *   _step     x_dev float32 [n, input_dim] -> y_dev float32 [n, out_dim]: row r is the next token of track tracks_host[r] (NULL: n ==
 *             tracks and row r is track r) and comes back as the encoder's output at that token, which attends to the track's tokens so
 *             far and itself.  Tracks distinct and in range, 1 <= n <= min(tracks, max_tokens), no track already at capacity:
 *             otherwise FLOPE_EINVAL with the offending index in the message, nothing enqueued and no position advanced.  Launches
 *             what flope_tf_forward launches for n rows under the handle's options (the same linear and LayerNorm kernels), with
 *             tf_attn_step in place of the attention kernel: one wave per (row, head) computes tf_attn_generic's causal row over
 *             the cache in that kernel's summation order and appends the token's k and v.  Where the forward's attention is
 *             FLOPE_TF_ATTN_GENERIC for the track's length, y_dev's row is, bit for bit, row `position` of the causal forward of the
 *             track so far; elsewhere (tf_attn_f32m, tf_attn_mfma, tf_attn_tiled) the attention order differs and the rows agree
 *             within those kernels' tolerances.  Neither reads nor writes option "causal" or what flope_tf_last_forward reports.
 *   _prefill  loads n tracks' histories: the causal ragged forward of x_dev [n, seq_len, input_dim] with lengths_host (NULL: all
 *             seq_len) -> y_dev [n, seq_len, out_dim], the bits of flope_tf_forward_varlen under "causal" = 1 (always as the
 *             launch sequence; "fused" gives the same bits), which also copies every layer's k and v of the valid rows into cache
 *             rows 0 .. length - 1 of track tracks_host[b] (NULL as above) and sets those tracks' positions to their lengths,
 *             whatever they held.  Limits of flope_tf_forward_varlen, lengths <= capacity, tracks as for _step.  Option "causal"
 *             is as it was when the call returns.
 *   _reset    positions of the n tracks of tracks_host (NULL: every track, n ignored) back to 0; enqueues nothing.
 * flope_tf_stream_open_window: a state that is never full -- sliding-window causal attention over a RING cache.
 * 1 <= window <= capacity <= 4096 (FLOPE_EINVAL outside, the message names the figure); the allocation has the same shape, and the
 * token at absolute position p lives in row p % capacity.  Positions are absolute and unbounded: _step refuses a track only once it
 * holds INT_MAX tokens (the message says so), and _position returns the absolute count.  Everything above holds with these changes:
 *   _step     the token at position p attends to keys max(0, p + 1 - window) .. p; its k and v overwrite row p % capacity, which held
 *             key p - capacity, outside every window that includes p.  LDS and time are bounded by `window`, not by the track's age.
 *             y_dev's row is, bit for bit and for every dtype, row p of the forward of the track so far under "causal" = 1,
 *             "window" = window (whose attention is tf_attn_generic by construction) -- alone or behind a _prefill, for any capacity
 *             >= window; while p < window also the row of a state opened without a window.
 *   _prefill  the ragged forward under "causal" = 1 and "window" = window, in bits; lengths are limited by flope_tf_forward_varlen
 *             alone, not by capacity: of a sequence of len tokens the last min(len, capacity) go to the ring (token i to row
 *             i % capacity), and the track is left at position len.  Options "causal" and "window" are as they were on return.
 * flope_tf_stream_open is window = 0: the linear cache and the refusals above.
 *   _extend    appends SEVERAL tokens per track in one call, behind what the track holds: x_dev float32 [n, seq_len,
 *             input_dim] -> y_dev [n, seq_len, out_dim], sequence b being the next lengths_host[b] tokens (1 .. seq_len, right-padded;
 *             NULL: all seq_len) of track tracks_host[b] (NULL as above).  The token at chunk row i takes position p = position + i and
 *             attends to keys 0 .. p of its track (a windowed state: max(0, p + 1 - window) .. p): those below the track's position
 *             from the cache, the chunk's own -- the query's among them -- from the call's packed qkv rows, never from a cache row the
 *             call writes.  The chunks run packed as one ragged launch sequence: the linears, LayerNorms, gather and scatter of
 *             flope_tf_forward_varlen at sum(lengths) rows, tf_attn_extend in place of the attention kernel (one wave per query, the
 *             four waves of a workgroup on consecutive queries of one sequence and head, tf_attn_generic's causal order), and behind
 *             it in every layer tf_cache_append, which copies the chunk's k and v to rows position + i (a ring: (position + i) %
 *             capacity, the chunk's last min(length, capacity) tokens).  Afterwards the track holds position + length tokens and a
 *             later _step or _extend continues it.  y_dev's valid rows are, bit for bit, for every dtype and option, what _step
 *             returns for the same tokens fed one call at a time, and so is the cache; any split of a track into chunks gives the same
 *             bits; hence they are rows position .. position + length - 1 of the causal (windowed) forward of the track wherever _step's
 *             are.  Rows behind a length come back as out_layer's bias, as from flope_tf_forward_varlen.  Refused with FLOPE_EINVAL,
 *             before anything is enqueued or any position moves, the offending index in the message: n outside 1 .. tracks (or
 *             tracks_host NULL with n != tracks), a track out of range or named twice, a length outside 1 .. seq_len, sum(lengths) >
 *             max_tokens, NULL buffers; a linear state: position + length > capacity; a windowed state: position + length > INT_MAX
 *             (a chunk may be longer than capacity: the ring keeps its last capacity tokens).  FLOPE_ESTATE without weights or after
 *             flope_tf_destroy.  Neither reads nor writes options "causal" / "window" or what flope_tf_last_forward reports, and
 *             never runs the single launch of option "fused".
 * Option "step_split" (flope_tf_set_option) picks the attention kernel of _step and _extend:
 *   _step_plan: FLOPE_TF_STEP_ROW (tf_attn_step / tf_attn_extend, one wave per token and head, the causal forward's bits) or
 *             FLOPE_TF_STEP_SPLIT (tf_attn_step_split / tf_attn_extend_split, one workgroup per token and head), whichever a _step or
 *             _extend of this state would launch now.  Enqueues nothing; FLOPE_ESTATE after flope_tf_destroy.
 *   _attention: A TEST HOOK, in the spirit of flope_tf_linear: the step's attention launch alone on a caller's tensor.  qkv_dev
 *             [n, seq_len, 3 model_dim] and att_dev [n, model_dim] in the handle's dtype (float for FLOPE_DT_F32), both 16-byte
 *             aligned.  For sequence b of length len = lengths_host[b] (NULL: seq_len), row b of att_dev is what _step's attention
 *             launch writes for a token whose q | k | v is row len - 1, on a track that holds the k | v columns of rows 0 .. len - 2:
 *             those are loaded with tf_cache_append into layer 0's part of tracks 0 .. n - 1 (a windowed state: the ring keeps the last
 *             `capacity` of them), then the kernel _step would run runs: the handle's option, the state's window.  Returns its
 *             FLOPE_TF_STEP_* id or < 0.  It OVERWRITES those cache rows and leaves tracks 0 .. n - 1 at position 0; needs no weights.
 *             Refused with FLOPE_EINVAL, nothing enqueued: n outside 1 .. min(tracks, max_tokens), a length outside 1 .. seq_len, on
 *             a linear state a length above capacity, NULL or misaligned buffers, a handle with num_layers = 0.
 * Option "extend_mfma" (flope_tf_set_option) picks the attention kernel of _extend in front of "step_split":
 *   _extend_plan: FLOPE_TF_EXTEND_ROW (tf_attn_extend), FLOPE_TF_EXTEND_SPLIT (tf_attn_extend_split) or FLOPE_TF_EXTEND_MFMA
 *             (tf_attn16_extend), whichever an _extend of this state would launch now (a call that would carry a track within 256
 *             positions of INT_MAX keeps the other two).  Enqueues nothing; FLOPE_ESTATE after flope_tf_destroy.
 *   _attention_extend: A TEST HOOK, as _attention is: the extend's attention launch alone on a caller's tensor.  qkv_dev [n, seq_len,
 *             3 model_dim] and att_dev [n, seq_len, model_dim] in the handle's dtype, both 16-byte aligned; lengths_host and
 *             cached_host: n ints each.  Of sequence b, rows 0 .. cached[b] - 1 are a track's history: their k | v columns are loaded
 *             with tf_cache_append into layer 0's part of track b (a windowed state: the ring keeps the last `capacity` of them); rows
 *             cached[b] .. lengths[b] - 1 are the chunk, packed into the handle's buffers.  Then the kernel _extend would run now
 *             runs once over all n chunks (the handle's options, the state's window) and rows cached[b] .. lengths[b] - 1 of att_dev
 *             are written; every other row of att_dev is left untouched.  Returns the FLOPE_TF_EXTEND_* id or < 0.  It OVERWRITES
 *             those cache rows and the handle's scratch buffers and leaves tracks 0 .. n - 1 at position 0; needs no weights.
 *             Refused with FLOPE_EINVAL, nothing enqueued: n outside 1 .. min(tracks, max_tokens), NULL lengths_host / cached_host,
 *             a length outside 1 .. seq_len, cached[b] outside 0 .. lengths[b] - 1, on a linear state a length above capacity, chunks
 *             of more than max_tokens rows together, NULL or misaligned buffers, a handle with num_layers = 0.
 * flope_tf_stream_open_bias: a state whose attention carries a DISTANCE TABLE, a relative bias such as ALiBi -- the
 * encoder has no positional term, so without one a track's last row is a function of the set of poses behind it, not of their order.
 *   table_host: float32 [planes][distances], planes = 1 (every head) or num_heads, distances = window ? window : capacity (window = 0
 *             is the linear state).  The query at position p of head h scores key j (the keys the state shows it, as above) as
 *             fl(fl(q . k * scale) + table[h or 0][p - j]); everything else is the unbiased state's.  Every entry must be finite: -inf
 *             is no way to mask here, visibility stays with `window`.  The table is copied to the device once, synchronously, into an
 *             allocation the state owns until _close (or flope_tf_destroy); it cannot be changed on an open state.
 *   Contracts: _step returns, in bits, the last row of the forward of the track so far under flope_tf_bias_create's bias
 *             [h][i][j] = table[h][i - j] for the visible j, -inf elsewhere (Python: distance_bias(table, L, window)), in EVERY dtype
 *             and under every option, because a compiled bias sends each of them to tf_attn_masked's BIASED form, whose order over a
 *             contiguous key range is this row's.  _prefill returns that forward's rows in bits (it runs tf_attn_extend's biased form
 *             at position 0 behind its cache copy).  _extend returns the bits of the same tokens fed by _step, whatever the split.  A
 *             zero table gives the bits of the unbiased state.
 *   Plans:    _step_plan returns FLOPE_TF_STEP_BIASED and _extend_plan FLOPE_TF_EXTEND_BIASED on such a state, whatever "step_split"
 *             and "extend_mfma" say (they do not reach it, as a compiled bias overrides mask_mfma / f32mfma / generic); the two test
 *             hooks run the biased kernels and return these ids.
 *   Refused with FLOPE_EINVAL, nothing allocated, the figure named: planes other than 1 or num_heads, distances other than
 *             window ? window : capacity, a NULL table, a NaN or +-inf entry (the message names (plane, distance)), and what
 *             _open / _open_window refuse.  FLOPE_EHIP: the allocation failed (the message names its size).
 *   _bias_planes: the planes of the state's table, 0 for a state without one; < 0 on error. */
#define FLOPE_TF_STEP_ROW         0
#define FLOPE_TF_STEP_SPLIT       1
#define FLOPE_TF_EXTEND_ROW       0
#define FLOPE_TF_EXTEND_SPLIT     1
#define FLOPE_TF_EXTEND_MFMA      2
#define FLOPE_TF_STEP_BIASED      2
#define FLOPE_TF_EXTEND_BIASED    3
/* what a row that feeds nothing carries in place of its track (flope_tf_stream_read_feed; csrc/tf_stream_feed.h) */
#define FLOPE_TF_FEED_SKIPPED     (-1)   /* the tracker skipped the row as unreliable */
#define FLOPE_TF_FEED_OVERFLOW    (-2)   /* the tracker's overflow flag is set: every row of the call */
#define FLOPE_TF_FEED_RANGE       (-3)   /* the track is none of the stream's */
#define FLOPE_TF_FEED_DUPLICATE   (-4)   /* an earlier row of the frame names the same track */
#define FLOPE_TF_FEED_FULL        (-5)   /* the track holds INT_MAX tokens */
/* what flope_tf_stream_step_tracker takes a token from */
#define FLOPE_TF_FEED_MEAS        0      /* the frame's measurement of the row */
#define FLOPE_TF_FEED_MEAN        1      /* the filtered mean of the row's track after the frame's updates */
typedef struct flope_tf_stream_s* flope_tf_stream;
int flope_tf_stream_open(flope_tf_handle h, int tracks, int capacity, flope_tf_stream* out);
int flope_tf_stream_open_window(flope_tf_handle h, int tracks, int capacity, int window, flope_tf_stream* out);
int flope_tf_stream_open_bias(flope_tf_handle h, int tracks, int capacity, int window, int planes, int distances, const float* table_host,
                              flope_tf_stream* out);
int flope_tf_stream_bias_planes(flope_tf_stream s);
int flope_tf_stream_close(flope_tf_stream s);
int flope_tf_stream_reset(flope_tf_stream s, int n, const int* tracks_host);
/* tokens held by `track`, or < 0 */
int flope_tf_stream_position(flope_tf_stream s, int track);
int flope_tf_stream_step(flope_tf_stream s, const float* x_dev, int n, const int* tracks_host, float* y_dev, void* stream);
int flope_tf_stream_prefill(flope_tf_stream s, const float* x_dev, int n, int seq_len, const int* lengths_host, const int* tracks_host,
                            float* y_dev, void* stream);
int flope_tf_stream_extend(flope_tf_stream s, const float* x_dev, int n, int seq_len, const int* lengths_host, const int* tracks_host,
                           float* y_dev, void* stream);
int flope_tf_stream_step_plan(flope_tf_stream s);
int flope_tf_stream_attention(flope_tf_stream s, const void* qkv_dev, int n, int seq_len, const int* lengths_host, void* att_dev, void* stream);
int flope_tf_stream_extend_plan(flope_tf_stream s);
int flope_tf_stream_attention_extend(flope_tf_stream s, const void* qkv_dev, int n, int seq_len, const int* lengths_host, const int* cached_host,
                                     void* att_dev, void* stream);
/* A DEVICE-POSITIONED stream state: the state above with its positions in device memory, stepped by an association
 * that only the device knows -- the device tracker's (flope_track_*): the host sees neither a pose nor a track id.
 *   _open_device  windowed only, 1 <= window <= capacity <= 4096: a ring is never full and a score row never holds more than
 *             `window` keys, so every launch is sized with smax = window without knowing a position.  planes = 0 with a NULL table
 *             opens an unbiased state; otherwise (planes, distances, table_host) are _open_bias's, refusals included.  The cache has
 *             the shape of every other state's; beside it the state owns int pos_dev[tracks] (zeroed), a table of 2 max_rows ints and a
 *             float32 token buffer [max_rows][input_dim], all allocated here.  max_rows: 1 .. max_tokens, the most rows one call takes.
 *             On such a state _step, _extend, _prefill, _reset, _position, _attention and _attention_extend return FLOPE_ESTATE and
 *             the message names the call to use instead; the calls below return FLOPE_ESTATE on every other state, which behaves
 *             exactly as before.
 *   The feed rule (csrc/tf_stream_feed.h, one definition for host and device).  Row m of a frame has association a in the tracker's
 *             encoding (a >= 0: matched track a; a < 0: opened track -1 - a; INT32_MIN: skipped).  It FEEDS its track iff the
 *             overflow flag is clear (else every row is FLOPE_TF_FEED_OVERFLOW), it was not skipped (_SKIPPED), the track is below the
 *             state's `tracks` (_RANGE), no row e < m of the frame names the same track (_DUPLICATE: the first measurement in
 *             measurement order is the frame's token) and the track's position is below INT_MAX (_FULL).  A feeding row takes the
 *             table entry (track, position) and advances the position by one; every other row takes (code, 0) and moves nothing.
 *   _step_assoc   x_dev float32 [n, input_dim], assoc_dev int32 [n], overflow_dev one int32 (non-zero: the flag; may be NULL = clear)
 *             -> y_dev float32 [n, out_dim], asynchronous on `stream`.  tf_stream_feed_kernel applies the rule on the device and
 *             copies the feeding rows of x_dev into the token buffer (the others become zero rows); then _step's launch sequence
 *             runs for n rows -- the forward's linears and LayerNorms, the attention kernel _step_plan names (ROW, SPLIT under
 *             "step_split", BIASED on a state with a table) at smax = window, which leaves a row alone whose table entry is a code;
 *             one last launch writes out_layer's bias into the rows of y_dev whose entry is a code, the value the library returns
 *             behind a ragged length.  A feeding row of y_dev is, in bits, what _step returns on a host-positioned state of the same
 *             window, capacity and table for the same tokens; so is the cache.  n = 0 enqueues nothing and returns 0.
 *   _step_tracker the same with n, the association, the flag and the 7-vectors taken from the tracker's device memory behind its
 *             last update (`stream` is made to wait for the tracker's event): columns 0 .. 6 of a feeding row's token are the row's
 *             measurement (source FLOPE_TF_FEED_MEAS) or its track's filtered mean after the frame's updates (FLOPE_TF_FEED_MEAN),
 *             world position then quaternion [x y z w], each rounded once to float32; columns 7 .. input_dim - 1 are zero.
 *             tf_stream_feed_kernel is the only launch of the call that reads the tracker's memory.  Returns the row count n.
 *             FLOPE_EINVAL: input_dim < 7, a source other than the two, n > max_rows, another device.  FLOPE_ESTATE: no update
 *             since flope_track_create / _reset, or the update that was fed to this state last (a host-side serial number of
 *             flope_track_update tells them apart).
 *   Refused by both, nothing enqueued and no position moved: NULL buffers, n outside 0 .. max_rows, a state that is not
 *             device-positioned (FLOPE_ESTATE), weights not loaded or the handle destroyed (FLOPE_ESTATE).
 *   Contracts: THE CALLS ON ONE STATE ARE ORDERED ON ONE STREAM BY THE CALLER, as above.  THE TRACKER'S NEXT UPDATE MUST BE ORDERED
 *             BEHIND _step_tracker BY THE CALLER (it overwrites what the call reads); issuing both on one stream does that, as the
 *             frame handle's pose stream does.  After flope_track_reset the caller resets the stream state too (_reset_device): the
 *             tracker's track numbers start again.  A call that fails on the way with FLOPE_EHIP may have moved positions.
 *   _reset_device every position back to 0, an asynchronous memset on `stream`.
 *   _read_positions  waits for the state's last call; int32 [tracks] into pos_host (cap >= tracks); returns tracks.
 *   _read_feed    waits for the state's last call; the table of the last _step_assoc / _step_tracker: track_host[m] the track row m
 *             fed or its FLOPE_TF_FEED_* code, pos_host[m] the position its token took (0 beside a code); returns the row count
 *             (0 before the first call), FLOPE_EINVAL when it exceeds cap.
 *   _read_tokens  test hook: waits; the float32 token rows [n][input_dim] of the last call into tok_host (cap_rows >= n); returns n. */
int flope_tf_stream_open_device(flope_tf_handle h, int tracks, int capacity, int window, int max_rows, int planes, int distances,
                                const float* table_host, flope_tf_stream* out);
int flope_tf_stream_step_assoc(flope_tf_stream s, const float* x_dev, const int32_t* assoc_dev, const int32_t* overflow_dev, int n, float* y_dev,
                               void* stream);
int flope_tf_stream_step_tracker(flope_tf_stream s, flope_track_handle t, int source, float* y_dev, void* stream);
int flope_tf_stream_reset_device(flope_tf_stream s, void* stream);
int flope_tf_stream_read_positions(flope_tf_stream s, int32_t* pos_host, int cap);
int flope_tf_stream_read_feed(flope_tf_stream s, int32_t* track_host, int32_t* pos_host, int cap);
int flope_tf_stream_read_tokens(flope_tf_stream s, float* tok_host, int cap_rows);
/* Any [L, L] attention mask (scripts/tf_encoder.py: nn.TransformerEncoder.forward(mask=)), compiled once into a
 * device-resident object and passed to any number of forwards.  A mask holds, for one sequence length L, the (query i, key j) pairs
 * that may attend: query i is a softmax over exactly its allowed keys, and a masked key is never loaded, neither its k nor its v (NaN
 * there reaches no output).  Attention under a mask runs tf_attn_masked -- the generic kernel's order over the allowed keys, for every
 * dtype and head_dim, whatever kernel the unmasked shape picks, unless option "mask_mfma" sends a 16-bit launch to tf_attn_tiled_masked
 * (flope_tf_set_option) -- and the forward is always the launch sequence.  Where a row's
 * allowed keys are one contiguous range the row is the generic kernel's for that range, operation for operation.
 *   _mask_create   (nn.TransformerEncoder.forward(mask=) of scripts/tf_encoder.py, the mask argument) allow_bits_host: uint32 words
 *             [seq_len][ceil(seq_len / 32)], bit j % 32 of word j / 32 of row i set = query i may attend to key j, padding bits zero.
 *             Allocates and uploads synchronously: masks are made once, a forward allocates nothing.  A handle may own several
 *             masks; they end with the handle: after flope_tf_destroy every call on a mask but _mask_destroy returns FLOPE_ESTATE.
 *             FLOPE_EINVAL (flope_tf_last_error names the index): NULL arguments, seq_len < 1 or > max_tokens, a set padding bit,
 *             a row without a key (the reference returns NaN for that row and, a layer later, for its whole batch element).
 *   _mask_info     seq_len and the number of allowed pairs (either pointer may be NULL).
 *   _forward_masked  (nn.TransformerEncoder.forward(src, mask=, src_key_padding_mask=) of scripts/tf_encoder.py) flope_tf_forward
 *             (lengths_host NULL) or flope_tf_forward_varlen (lengths_host: batch ints) under mask m, whose seq_len must equal the
 *             call's.  A sequence of n tokens is encoded alone under the top-left n x n corner of the mask; rows behind it are never
 *             read and come back as out_layer.bias.  Never the single launch of option "fused"; neither reads nor writes options
 *             "causal" / "window"; flope_tf_last_forward reports FLOPE_TF_FWD_LAUNCHES after it.  FLOPE_EINVAL, before anything is
 *             enqueued: NULL arguments, a seq_len that differs from the mask's, a length outside 1 .. seq_len, a length n under which
 *             a row below n has no key (the message names b and the row), too many tokens, a mask of another handle.
 *   _attention_masked  flope_tf_attention (lengths_host NULL: qkv_dev [batch, seq_len, 3*model_dim]) or flope_tf_attention_varlen
 *             (lengths_host: packed rows) under mask m: the attention launch of _forward_masked alone.  Returns
 *             FLOPE_TF_ATTN_MASKED (4), under option "mask_mfma" FLOPE_TF_ATTN_MASKED16 (5) where tf_attn_pick_masked picks it, or < 0
 *             with the refusals above.  The refusal of a seq_len too long for tf_attn_masked's score rows in LDS applies only where
 *             that kernel is the pick.
 *   _last_forward_masked  the FLOPE_TF_ATTN_* id of the attention launches of the last _forward_masked that enqueued anything
 *             (FLOPE_TF_ATTN_MASKED, or FLOPE_TF_ATTN_MASKED16 under option "mask_mfma"); -1 before the first.
 *   _mask_tiles    the mask's tile map (flope_amd/csrc/tf_attn_mask.h; any pointer may be NULL): its query blocks of 128 rows, the
 *             64-key blocks listed over all of them (of query_blocks * ceil(seq_len / 64)), and the 8 (wave, 32-key step) tiles of
 *             every listed block by class: no allowed pair, some, all.
 *   _forward_flops_masked  algorithmic FLOPs of _forward_masked: the linears on every token, attention on the allowed pairs (of each
 *             length's corner with lengths_host); 0 for an invalid call. */
typedef struct flope_tf_mask* flope_tf_mask_handle;
int flope_tf_mask_create(flope_tf_handle h, int seq_len, const uint32_t* allow_bits_host, flope_tf_mask_handle* out);
int flope_tf_mask_destroy(flope_tf_mask_handle m);
int flope_tf_mask_info(flope_tf_mask_handle m, int* seq_len, long long* allowed_pairs);
int flope_tf_forward_masked(flope_tf_handle h, const float* x_dev, int batch, int seq_len, const int* lengths_host, flope_tf_mask_handle m,
                            float* y_dev, void* stream);
int flope_tf_attention_masked(flope_tf_handle h, const void* qkv_dev, int batch, int seq_len, const int* lengths_host, flope_tf_mask_handle m,
                              void* out_dev, void* stream);
double flope_tf_forward_flops_masked(flope_tf_handle h, int batch, const int* lengths_host, flope_tf_mask_handle m);
int flope_tf_last_forward_masked(flope_tf_handle h);
int flope_tf_mask_tiles(flope_tf_mask_handle m, int* query_blocks, long long* blocks_listed, long long* steps_none, long long* steps_some,
                        long long* steps_all);
/* An additive attention bias (nn.TransformerEncoder.forward(mask=) with a float mask of scripts/tf_encoder.py), compiled
 * once as a mask is: the [L, L] set of allowed pairs a compiled mask holds plus a float32 value for every allowed pair, in one plane for
 * all heads or one plane per head.  Query i of head h is softmax_j(q . k_j / sqrt(head_dim) + bias[h][i][j]) over exactly its allowed
 * keys; a masked key is never loaded: not its k, not its v, and its bias entry is never used (never loaded either unless option
 * "bias_mfma" picks the MFMA kernel, which may load its -inf and discards it).  The bias is kept as float32 on every handle dtype.
 *   _bias_create   bias_host: float32 [planes][seq_len][seq_len], planes = 1 or num_heads; -inf = masked, any finite value = allowed
 *             with that value added to the scaled score (the sum is a rounding of its own).  Returns the handle type of _mask_create:
 *             _forward_masked, _attention_masked (fixed and ragged: a sequence of n tokens under the top-left n x n corner of every
 *             plane), _mask_destroy, _mask_info, _forward_flops_masked (the adds are not counted) and _mask_tiles take it as they
 *             take a mask.  One device allocation bits | first | last | bias | start | tiles, uploaded synchronously; a failed allocation is
 *             FLOPE_EHIP and the message names the size (at seq_len 4096 a plane is 64 MiB).  FLOPE_EINVAL before anything is
 *             enqueued, the index (plane, row, col) in flope_tf_last_error: NULL arguments, seq_len < 1 or > max_tokens, planes
 *             neither 1 nor num_heads, an entry that is +inf or NaN, a plane whose masked entries differ from plane 0's (a per-head
 *             difference is written as a large negative finite value), a row without a key.
 *             Attention under a bias runs the BIASED instantiation of tf_attn_masked (FLOPE_TF_ATTN_BIASED = 6, what _attention_masked returns and
 *             _last_forward_masked reports) on every dtype and under every option, "mask_mfma", "f32mfma" and "generic" included:
 *             tf_attn_masked's order with the one add, so an all-zero bias gives tf_attn_masked's bits for the same allowed set.
 *             The one exception is option "bias_mfma" = 1 on a 16-bit handle (above): FLOPE_TF_ATTN_BIASED16 = 7.
 *   _mask_bias_planes  the planes of a compiled bias, 0 for a plain mask. */
int flope_tf_bias_create(flope_tf_handle h, int seq_len, int planes, const float* bias_host, flope_tf_mask_handle* out);
int flope_tf_mask_bias_planes(flope_tf_mask_handle m);

/* ---- YOLO11-seg detector front end ---------------------------------------------------
 * Replaces `self.yolo = YOLO(yolo_path)` (sunflower/predictor/fast_pose_predictor.py:36) and the
 * `results = self.yolo(image)` + mask / box post-processing of `get_bbox_mask` (:44-57).  The network and
 * its pre/post-processing are those of ultralytics 8.3.27 (environment.yml:231; not vendored by the reference):
 * LetterBox(imgsz, auto, stride 32) + BGR->RGB + /255 -> yolo11-seg graph (Conv+BN+SiLU, C3k2, SPPF, C2PSA,
 * upsample/concat neck, Segment head) -> DFL decode -> NMS -> coef.proto masks cropped, upsampled, > 0.
 * One handle = one device, one frame size.  dtype FLOPE_DT_F16 / FLOPE_DT_BF16 (16-bit maps, fp32 accumulation,
 * fp32 head outputs / decode / NMS), or FLOPE_DT_F32 = strict mode: float32 maps and plain float32 fused-multiply-add
 * convolutions over the same graph in program order (no MFMA, no 16-bit rounding; ~50x slower) -- the arithmetic the
 * reference runs ultralytics in (fast_pose_predictor.py:49), so that the INTEGER outputs of get_bbox_mask (int16 boxes,
 * uint8 mask, :52-56) can be compared for equality with a float32 pipeline.  Frame size / imgsz combinations whose
 * stride-32 map exceeds 2,560 tokens (imgsz above ~1600 for 16:9 frames) are rejected by flope_yolo_load_weights. */
typedef struct flope_yolo* flope_yolo_handle;
int flope_yolo_create(int device_id, int frame_h, int frame_w, int imgsz, int dtype, flope_yolo_handle* out);
int flope_yolo_destroy(flope_yolo_handle h);
const char* flope_yolo_last_error(flope_yolo_handle h);
/* letterboxed network input size for this frame size (multiples of 32) */
int flope_yolo_input_size(flope_yolo_handle h, int* in_h, int* in_w);
/* the ultralytics model's state_dict (`model.<i>. ...` names, host fp32): builds the graph from the key set and the
 * tensor shapes, folds BatchNorm(eps 1e-3), packs for MFMA, allocates every intermediate map.  Once per handle. */
int flope_yolo_load_weights(flope_yolo_handle h, int n, const char* const* names,
                            const float* const* host_ptrs, const int* ndims, const int64_t* const* shapes);
/* `results = self.yolo(image)` + get_bbox_mask's post-processing.  frame_dev: uint8 BGR [H,W,3] (a cv2 image).
 * conf / iou / max_det: ultralytics predict defaults are 0.25 / 0.7 / 300 (max_det <= 300).  NMS considers the 4,096 most
 * confident anchors above `conf` (ultralytics: 30,000) -- identical unless more than 4,096 anchors pass the threshold.
 * det_dev float32 [max_det,8]: rows = xyxy in frame pixels (ops.scale_boxes, clipped; the reference casts them to
 * int16), confidence, class, anchor index, 0 -- in NMS order; count_dev int32 [1]; mask_dev uint8 [H,W] = the summed /
 * clipped / x255 instance masks resized to the frame with cv2's 8-bit INTER_LINEAR (fast_pose_predictor.py:50-54). */
int flope_yolo_detect(flope_yolo_handle h, const uint8_t* frame_dev, float conf, float iou, int max_det,
                      float* det_dev, int32_t* count_dev, uint8_t* mask_dev, void* stream);
/* network only (parity tests): letterbox + every layer, no post-processing */
int flope_yolo_forward(flope_yolo_handle h, const uint8_t* frame_dev, void* stream);
/* copy one map of the LAST forward to float32 [C,H,W]: "input", graph outputs "0".."22" (yaml indices of Conv / C3k2 /
 * SPPF / C2PSA modules), "box0..2" / "cls0..2" / "coef0..2" (Segment head rows per level), "proto", "proto_up",
 * "mask_lb" (merged mask at the letterboxed size), "cand_box" [4,1,A] / "cand_conf" / "cand_cls" [1,1,A] (decoded box, best
 * confidence and class of every anchor) -- the last four after flope_yolo_detect.  dims_out[3] = {C,H,W}; dst_dev NULL = size
 * query only. */
int flope_yolo_read_tensor(flope_yolo_handle h, const char* name, float* dst_dev, int64_t* dims_out, void* stream);
/* options of one handle (each call returns the previous value or <0; an unknown name is FLOPE_EINVAL):
 *   "graph" (default 0): flope_yolo_detect captures its launch sequence into a hipGraph the first time it sees a
 *       (frame_dev, thresholds, output buffers) tuple and replays it afterwards -- keep those pointers stable across frames
 *       (measured as no gain on MI355X: the GPU-side chain of short kernels is the bound, not the host).
 * The others force the reference path that tests compare a shipped kernel against; the defaults are the shipped paths:
 *   "batch" (default 1): the independent launches of one dependency level of the graph (the Segment head's box / class /
 *       coefficient branches of a level, the Proto block beside them, parallel 1x1 convs inside C3k) share one grid; 0: one
 *       launch per op in the program order of the ultralytics yaml;
 *   "bneck" (default 1): Bottleneck pairs (3x3 -> 3x3, <= 64 channels) as one fused launch with the intermediate map in LDS;
 *       0: two conv launches;
 *   "generic_attn" (default 0): 1 runs C2PSA attention on the generic fp32 kernel instead of the MFMA one;
 *   "f32mfma" (default 1): FLOPE_DT_F32 convolutions and attention on the exact-fp32 MFMA kernels; 0: the plain
 *       fused-multiply-add kernels, one launch per op;
 *   "tile" (default 1): large-map convs stage an 8 x 16 tile's input patch in LDS; 0: fragments straight from global memory;
 *   "pool_lds" (default 1): SPPF's cascaded max-pools in LDS where the map fits; 0: the 13 x 13 ring kernel.
 * "bneck", "tile" and "pool_lds" rebuild this handle's schedules and drop its captured graphs when they change. */
int flope_yolo_set_option(flope_yolo_handle h, const char* name, int value);
/* Test hooks (per-op element-wise checks); nothing flope_yolo_forward / flope_yolo_detect launch depends on them.
 * flope_yolo_op_count: ops of the program-order list.  flope_yolo_op_info: one line of `key=value` words for op i -- kind (conv,
 * bneck, dw, pool, up, attn), state_dict name, geometry (a fused Bottleneck: cv1's words, " | ", cv2's), and `path=`: the kernel
 * form the launcher takes under the handle's current options, as reported by the launchers' own geometry functions.
 * Op i's views are tensors of flope_yolo_read_tensor: "op<i>.in", "op<i>.res" (conv residual), "op<i>.add" (depthwise addend),
 * "op<i>.mid" (a Bottleneck's cv1 output, written with bneck = 0 only), "op<i>.out" (out_mode 1: its float32 columns of the
 * prediction rows; pool: all n * C channels; attention: [C, 1, N]).
 * flope_yolo_forward_ops: the letterbox and the first n ops in program order, one launch per op (C2PSA updates a map in place,
 * so an op's inputs are only intact before it ran). */
int flope_yolo_op_count(flope_yolo_handle h);
int flope_yolo_op_info(flope_yolo_handle h, int i, char* text, int cap);
int flope_yolo_forward_ops(flope_yolo_handle h, const uint8_t* frame_dev, int n, void* stream);
/* Test hook: the post-processing tail of flope_yolo_detect (decode, NMS with box scaling, masks, resize: the same launch
 * sequence, one function) on GIVEN head rows instead of the network's.  rows_dev: float32 [A][no], a row = 64 DFL logits, nc
 * class logits, 32 mask coefficients (A = W of "cand_conf", no = 64 + nc + 32); proto_dev: [mh][mw][32] in the handle's own map
 * type (16-bit or float32; mh, mw = H, W of "proto").  Both are copied device to device into the handle's own buffers, so
 * flope_yolo_read_tensor serves "cand_*", "mask_lb", "box*" / "cls*" / "coef*" and "proto" afterwards as after flope_yolo_detect.
 * Runs eagerly whatever the "graph" option says; thresholds and outputs as flope_yolo_detect. */
int flope_yolo_postprocess(flope_yolo_handle h, const float* rows_dev, const void* proto_dev, float conf, float iou, int max_det,
                           float* det_dev, int32_t* count_dev, uint8_t* mask_dev, void* stream);
/* developer aid: `iters` forwards with a HIP event pair around every launch of the graph; writes a text table (mean
 * microseconds per launch, kind, geometry, state_dict name) into text_out[cap] */
int flope_yolo_profile(flope_yolo_handle h, const uint8_t* frame_dev, int iters, char* text_out, int cap, void* stream);
double flope_yolo_flops(flope_yolo_handle h);      /* 2*MAC of one forward (convs + attention) */
int flope_yolo_launches(flope_yolo_handle h);      /* kernel launches per flope_yolo_detect */
int flope_yolo_graph_cache_size(flope_yolo_handle h);  /* captured launch sequences currently held ("graph" option; <= 8) */

#ifdef __cplusplus
}
#endif
#endif /* FLOPE_AMD_H */
