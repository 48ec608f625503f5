// flope_frame_*: everything FastPosePredictor.get_flower_poses does BEHIND the detector
// (reference sunflower/predictor/fast_pose_predictor.py:55-56, 60-156) as three C calls per frame -- r05, VERDICT r4 item 3.
//
//   flope_frame_select   detector rows -> int16 boxes (:55-56) -> squarify_bb (mvg.py:324-343) -> bb_in_frame (mvg.py:345-351), in
//                        detection order, ON THE DEVICE (one wave, ballots for the ranks: no atomics, deterministic order); the number
//                        of surviving boxes travels to pinned host memory behind it.  Asynchronous.
//   flope_frame_enqueue  waits for that ONE integer (HIP grids are sized on the host: a fixed-capacity batch would run the network on
//                        up to max_det crops -- B = 32 @ 512^2 costs 0.83 ms where B = 4 costs 0.39 -- against ~20 us for the 4-byte
//                        read-back), then enqueues depth lift (:88-96, image_manipulation.py:39-96, mvg.py:387-408), Lanczos crops x
//                        mask (:108-123), PoseResNet -> Procrustes -> yaw-null -> Rt (:125-144) and the copy of the pose rows +
//                        depth-reliable flags to pinned host memory.  Asynchronous behind the wait.
//   flope_frame_finish   waits for those copies, drops the flowers without reliable depth (:97-102) -> float64 [n][4][4]; 0 rows is the
//                        reference's `None` (:86-87, :101-102).
//   flope_frame_to_poses = the three in sequence (the sequential live loop, scripts/live_pose.py:31-41).
// The host does no per-box work and issues no PyTorch operation: the Python predictor makes one ctypes call per stage.  Every
// unreliable-depth box still goes through the network and is dropped at the end (as the r01 host path did: crops are independent, one
// round trip less); the surviving rows are the rows the reference computes.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include "../../include/flope_amd.h"
#include "frame_plan.h"
#include "guard.h"

namespace {
thread_local std::string g_frame_error;

struct Slot {
  int32_t* boxes = nullptr;      // device [2 * cap][4]: in-frame boxes as detected, then their squared versions
  int* nsel = nullptr;           // device [2]: boxes kept (<= cap), boxes in frame
  uint8_t* depth_scratch = nullptr;
  float *dv = nullptr, *xyz = nullptr, *Rt = nullptr;
  int32_t* rel = nullptr;
  void* crops = nullptr;
  int* nsel_host = nullptr;      // pinned [2]
  float* Rt_host = nullptr;      // pinned [cap][16]
  int32_t* rel_host = nullptr;   // pinned [cap]
  hipEvent_t ev_sel = nullptr, ev_done = nullptr;
  int state = 0;                 // 0 idle, 1 selected, 2 enqueued
  int n = 0;                     // boxes enqueued
  // guarded handles only (flope_frame_create_guarded)
  float* gap = nullptr;          // device [cap]: the guard's conditioning figure of every crop
  void* stream = nullptr;        // the stream flope_frame_enqueue ran on: flope_frame_finish repairs on it
  int gap_n = -1;                // crops of the last finished frame (flope_frame_read_gaps); -1: none yet
};
}  // namespace

struct flope_frame {
  flope_handle eng = nullptr;
  flope_guard_handle guard = nullptr;   // guarded mode: eng is the guard's f16 engine and slot i uses slot i of the guard
  int device = 0, H = 0, W = 0, crop = 0, cap = 0, nslots = 0, eng_maxB = 0, fmt = 0;
  size_t crop_bytes = 0;
  Slot* slots = nullptr;
  std::string err;
};

namespace {
int ffail(flope_frame* f, int code, const std::string& msg) {
  if (f) f->err = msg;
  g_frame_error = msg;
  return code;
}

// (:55-56) float32 xyxy -> int16 like numpy's astype, then squarify_bb / bb_in_frame in integer arithmetic exactly as
// sunflower/utils/mvg.py states them: frame_plan.h's frame_count and frame_box (one definition, shared with the CPU tests); here
// only the order: 64 rows per pass, a ballot for the ranks, the kept boxes of earlier passes carried in `base`
__global__ __launch_bounds__(64) void frame_select_kernel(const float* __restrict__ det, const int* __restrict__ count, int max_det,
                                                          int H, int W, int cap, int32_t* __restrict__ boxes, int* __restrict__ nsel) {
  const int lane = threadIdx.x;
  const int n = frame_count(*count, max_det);
  int base = 0;
  for (int i0 = 0; i0 < n; i0 += 64) {
    const int i = i0 + lane;
    bool keep = false;
    int good[4] = {0, 0, 0, 0}, sq[4] = {0, 0, 0, 0};
    if (i < n) keep = frame_box(det + (size_t)i * kFrameDetRow, W, H, good, sq);
    const unsigned long long m = __ballot(keep);
    const int rank = base + __popcll(m & ((1ull << lane) - 1ull));
    if (keep && rank < cap) {
      int32_t *g = boxes + rank * 4, *s = boxes + (size_t)cap * 4 + rank * 4;
      g[0] = good[0]; g[1] = good[1]; g[2] = good[2]; g[3] = good[3];
      s[0] = sq[0]; s[1] = sq[1]; s[2] = sq[2]; s[3] = sq[3];
    }
    base += __popcll(m);
  }
  if (lane == 0) { nsel[0] = base < cap ? base : cap; nsel[1] = base; }
}

void free_slot(Slot& s) {
  if (s.ev_done) { hipEventSynchronize(s.ev_done); }
  void* dev[] = {s.boxes, s.nsel, s.depth_scratch, s.dv, s.xyz, s.Rt, s.rel, s.crops, s.gap};
  for (void* p : dev) if (p) hipFree(p);
  void* host[] = {s.nsel_host, s.Rt_host, s.rel_host};
  for (void* p : host) if (p) hipHostFree(p);
  if (s.ev_sel) hipEventDestroy(s.ev_sel);
  if (s.ev_done) hipEventDestroy(s.ev_done);
  s = Slot();
}
}  // namespace

extern "C" const char* flope_frame_last_error(flope_frame_handle f) { return f ? f->err.c_str() : g_frame_error.c_str(); }

namespace {
int frame_create(flope_handle pose_engine, flope_guard_handle guard, int frame_h, int frame_w, int max_boxes, int slots, flope_frame_handle* out) {
  int maxB = 0, dtype = 0, eh = 0, ew = 0, dev = 0;
  if (!pose_engine || flope_engine_geometry(pose_engine, &maxB, &dtype, &eh, &ew, &dev) != FLOPE_OK)
    return ffail(nullptr, FLOPE_EINVAL, "flope_frame_create: bad PoseResNet engine handle");
  if (frame_h < 1 || frame_w < 1 || frame_h > 32767 || frame_w > 32767 || max_boxes < 1 || max_boxes > 4096 || slots < 1 || slots > 16 || eh != ew)
    return ffail(nullptr, FLOPE_EINVAL, "flope_frame_create: frame up to 32767 x 32767 (int16 boxes), 1..4096 boxes, 1..16 slots, a square crop engine");
  if (hipSetDevice(dev) != hipSuccess) return ffail(nullptr, FLOPE_EHIP, "flope_frame_create: hipSetDevice failed");
  flope_frame* f = new flope_frame();
  f->eng = pose_engine; f->guard = guard; f->device = dev; f->H = frame_h; f->W = frame_w; f->crop = eh; f->cap = max_boxes; f->nslots = slots; f->eng_maxB = maxB;
  // crops in the trunk's own 16-bit NHWC layout where there is one (bit-identical to float32 crops: the stem rounds to that type)
  // a guarded handle keeps float32 crops: the f16 stem rounds them on load exactly as it rounds the 16-bit ones, and the float32 repair
  // sees them unrounded
  f->fmt = guard ? FLOPE_IN_F32_NCHW : dtype == FLOPE_DT_F16 ? FLOPE_IN_F16_NHWC : (dtype == FLOPE_DT_BF16 ? FLOPE_IN_BF16_NHWC : FLOPE_IN_F32_NCHW);
  f->crop_bytes = (size_t)f->crop * f->crop * 3 * (f->fmt == FLOPE_IN_F32_NCHW ? 4 : 2);
  f->slots = new Slot[slots];
  const size_t cap = (size_t)max_boxes, npix = (size_t)frame_h * frame_w;
  bool ok = true;
  for (int i = 0; i < slots && ok; ++i) {
    Slot& s = f->slots[i];
    ok = hipMalloc((void**)&s.boxes, cap * 8 * sizeof(int32_t)) == hipSuccess && hipMalloc((void**)&s.nsel, 2 * sizeof(int)) == hipSuccess &&
         hipMalloc((void**)&s.depth_scratch, ((npix + 15) & ~(size_t)15) + 16 + 512 * cap) == hipSuccess &&
         hipMalloc((void**)&s.dv, cap * sizeof(float)) == hipSuccess && hipMalloc((void**)&s.xyz, cap * 3 * sizeof(float)) == hipSuccess &&
         hipMalloc((void**)&s.Rt, cap * 16 * sizeof(float)) == hipSuccess && hipMalloc((void**)&s.rel, cap * sizeof(int32_t)) == hipSuccess &&
         hipMalloc(&s.crops, cap * f->crop_bytes) == hipSuccess && (!guard || hipMalloc((void**)&s.gap, cap * sizeof(float)) == hipSuccess) &&
         hipHostMalloc((void**)&s.nsel_host, 2 * sizeof(int), hipHostMallocDefault) == hipSuccess &&
         hipHostMalloc((void**)&s.Rt_host, cap * 16 * sizeof(float), hipHostMallocDefault) == hipSuccess &&
         hipHostMalloc((void**)&s.rel_host, cap * sizeof(int32_t), hipHostMallocDefault) == hipSuccess &&
         hipEventCreateWithFlags(&s.ev_sel, hipEventDisableTiming) == hipSuccess && hipEventCreateWithFlags(&s.ev_done, hipEventDisableTiming) == hipSuccess;
  }
  if (!ok) {
    for (int i = 0; i < slots; ++i) free_slot(f->slots[i]);
    delete[] f->slots; delete f;
    return ffail(nullptr, FLOPE_EHIP, "flope_frame_create: allocation failed");
  }
  *out = f;
  return FLOPE_OK;
}
}  // namespace

extern "C" int flope_frame_create(flope_handle pose_engine, int frame_h, int frame_w, int max_boxes, int slots, flope_frame_handle* out) {
  if (!out) return ffail(nullptr, FLOPE_EINVAL, "flope_frame_create: out is NULL");
  *out = nullptr;
  return frame_create(pose_engine, nullptr, frame_h, frame_w, max_boxes, slots, out);
}

extern "C" int flope_frame_create_guarded(flope_guard_handle guard, int frame_h, int frame_w, int max_boxes, int slots, flope_frame_handle* out) {
  if (!out) return ffail(nullptr, FLOPE_EINVAL, "flope_frame_create_guarded: out is NULL");
  *out = nullptr;
  int gslots = 0;
  flope_handle fast = flope_guard_fast_engine(guard, &gslots);
  if (!fast) return ffail(nullptr, FLOPE_EINVAL, "flope_frame_create_guarded: NULL guard handle");
  if (slots > gslots) return ffail(nullptr, FLOPE_EINVAL, "flope_frame_create_guarded: more slots than the guard has (" + std::to_string(gslots) + ")");
  return frame_create(fast, guard, frame_h, frame_w, max_boxes, slots, out);
}

extern "C" int flope_frame_destroy(flope_frame_handle f) {
  if (!f) return FLOPE_OK;
  hipSetDevice(f->device);
  for (int i = 0; i < f->nslots; ++i) free_slot(f->slots[i]);
  delete[] f->slots;
  delete f;
  return FLOPE_OK;
}

extern "C" int flope_frame_select(flope_frame_handle f, int slot, const float* det_dev, const int32_t* count_dev, int max_det, void* stream) {
  if (!f) return ffail(nullptr, FLOPE_EINVAL, "flope_frame_select: NULL handle");
  if (slot < 0 || slot >= f->nslots || !det_dev || !count_dev || max_det < 1) return ffail(f, FLOPE_EINVAL, "flope_frame_select: bad slot / NULL detector outputs");
  Slot& s = f->slots[slot];
  if (s.state == 2) return ffail(f, FLOPE_ESTATE, "flope_frame_select: the slot still holds an unfinished frame (call flope_frame_finish)");
  if (hipSetDevice(f->device) != hipSuccess) return ffail(f, FLOPE_EHIP, "hipSetDevice failed");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(frame_select_kernel, dim3(1), dim3(64), 0, st, det_dev, (const int*)count_dev, max_det, f->H, f->W, f->cap, s.boxes, s.nsel);
  if (hipGetLastError() != hipSuccess || hipMemcpyAsync(s.nsel_host, s.nsel, 2 * sizeof(int), hipMemcpyDeviceToHost, st) != hipSuccess ||
      hipEventRecord(s.ev_sel, st) != hipSuccess)
    return ffail(f, FLOPE_EHIP, "flope_frame_select: launch / copy failed");
  s.state = 1;
  return FLOPE_OK;
}

extern "C" int flope_frame_enqueue(flope_frame_handle f, int slot, const uint8_t* frame_dev, const uint8_t* mask_dev, const void* depth_dev,
                                   int depth_format, float depth_div, const float* K4_host, float near_plane, float far_plane, void* stream) {
  if (!f) return ffail(nullptr, FLOPE_EINVAL, "flope_frame_enqueue: NULL handle");
  if (slot < 0 || slot >= f->nslots || !frame_dev || !mask_dev || !depth_dev || !K4_host) return ffail(f, FLOPE_EINVAL, "flope_frame_enqueue: bad slot / NULL input");
  Slot& s = f->slots[slot];
  if (s.state != 1) return ffail(f, FLOPE_ESTATE, "flope_frame_enqueue: call flope_frame_select for this slot first");
  // Every negative return from here on leaves the slot idle (state 0) and, on a guarded handle, the guard slot un-armed: a slot left
  // in state 2 by a failed call would let flope_frame_finish wait on an event of an earlier frame and return that frame's rows.
  if (hipSetDevice(f->device) != hipSuccess) { s.state = 0; return ffail(f, FLOPE_EHIP, "hipSetDevice failed"); }
  if (hipEventSynchronize(s.ev_sel) != hipSuccess) { s.state = 0; return ffail(f, FLOPE_EHIP, "flope_frame_enqueue: waiting for the box count failed"); }
  const int n = s.nsel_host[0];
  if (s.nsel_host[1] > f->cap) { s.state = 0; return ffail(f, FLOPE_EINVAL, "flope_frame_enqueue: more in-frame boxes than max_boxes (" + std::to_string(s.nsel_host[1]) + ")"); }
  // What flope_depth_lift refuses before it launches anything is refused here first, whatever the number of boxes.
  if (!(depth_div > 0.f) || depth_format < 0 || depth_format > 1) {
    s.state = 0;
    return ffail(f, FLOPE_EINVAL, "flope_frame_enqueue: depth_div must be > 0 and depth_format 0 (uint16) or 1 (float32)");
  }
  s.n = n; s.state = 2;
  hipStream_t st = (hipStream_t)stream;
  if (n == 0) {
    if (hipEventRecord(s.ev_done, st) == hipSuccess) return 0;
    s.state = 0;
    return ffail(f, FLOPE_EHIP, "hipEventRecord failed");
  }
  if (flope_depth_lift(depth_dev, depth_format, mask_dev, f->H, f->W, depth_div, near_plane, far_plane, s.boxes, n, K4_host, s.depth_scratch, s.dv,
                       s.rel, s.xyz, stream) != 0) {
    s.state = 0;
    return ffail(f, FLOPE_EHIP, "flope_frame_enqueue: depth lift failed");
  }
  if (flope_crop_resize_mask(frame_dev, mask_dev, f->H, f->W, s.boxes + (size_t)f->cap * 4, n, f->crop, f->fmt, s.crops, stream) != 0) {
    s.state = 0;
    return ffail(f, FLOPE_EHIP, "flope_frame_enqueue: crop kernel failed");
  }
  s.stream = stream;
  for (int off = 0; f->guard && off < n; off += f->eng_maxB) {
    // guarded: the f16 forward and the guard's selection per chunk; every chunk but the last is repaired here (one guard slot holds
    // one forward), the last one in flope_frame_finish.  A failure leaves frame slot and guard slot idle.
    const int m = n - off < f->eng_maxB ? n - off : f->eng_maxB;
    int rc = flope_guard_forward(f->guard, slot, (const char*)s.crops + (size_t)off * f->crop_bytes, f->fmt, m, s.xyz + (size_t)off * 3, 1, nullptr, nullptr,
                                 s.Rt + (size_t)off * 16, s.gap + off, stream);
    if (rc == FLOPE_OK && off + m < n) rc = flope_guard_repair(f->guard, slot, stream);
    if (rc < 0) { s.state = 0; return ffail(f, rc, std::string("flope_frame_enqueue: ") + flope_guard_last_error(f->guard)); }
  }
  for (int off = 0; !f->guard && off < n; off += f->eng_maxB) {           // (more boxes than the engine's batch: several forwards)
    const int m = n - off < f->eng_maxB ? n - off : f->eng_maxB;
    const int rc = flope_forward_poses(f->eng, (const char*)s.crops + (size_t)off * f->crop_bytes, f->fmt, m, s.xyz + (size_t)off * 3, 1, nullptr, nullptr,
                                       s.Rt + (size_t)off * 16, stream);
    if (rc != FLOPE_OK) { s.state = 0; return ffail(f, rc, std::string("flope_frame_enqueue: ") + flope_last_error(f->eng)); }
  }
  if (hipMemcpyAsync(s.Rt_host, s.Rt, (size_t)n * 16 * sizeof(float), hipMemcpyDeviceToHost, st) != hipSuccess ||
      hipMemcpyAsync(s.rel_host, s.rel, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, st) != hipSuccess || hipEventRecord(s.ev_done, st) != hipSuccess) {
    if (f->guard) flope_guard_cancel(f->guard, slot);
    s.state = 0;
    return ffail(f, FLOPE_EHIP, "flope_frame_enqueue: result copy failed");
  }
  return n;
}

extern "C" int flope_frame_finish(flope_frame_handle f, int slot, double* poses_out, int cap) {
  if (!f) return ffail(nullptr, FLOPE_EINVAL, "flope_frame_finish: NULL handle");
  if (slot < 0 || slot >= f->nslots) return ffail(f, FLOPE_EINVAL, "flope_frame_finish: bad slot");
  Slot& s = f->slots[slot];
  if (s.state != 2) return ffail(f, FLOPE_ESTATE, "flope_frame_finish: nothing enqueued in this slot");
  if (f->guard && s.n > 0) {
    // the guard's one host wait (the number of flagged crops) sits here, where the host waits anyway; repaired rows travel again
    const int fixed = flope_guard_repair(f->guard, slot, s.stream);
    if (fixed < 0) { s.state = 0; return ffail(f, fixed, std::string("flope_frame_finish: ") + flope_guard_last_error(f->guard)); }
    if (fixed > 0 && (hipMemcpyAsync(s.Rt_host, s.Rt, (size_t)s.n * 16 * sizeof(float), hipMemcpyDeviceToHost, (hipStream_t)s.stream) != hipSuccess ||
                      hipEventRecord(s.ev_done, (hipStream_t)s.stream) != hipSuccess)) {
      s.state = 0;
      return ffail(f, FLOPE_EHIP, "flope_frame_finish: copy of the repaired poses failed");
    }
  }
  s.state = 0;                                                     // whatever happens below, the slot is idle afterwards
  if (hipSetDevice(f->device) != hipSuccess || hipEventSynchronize(s.ev_done) != hipSuccess) return ffail(f, FLOPE_EHIP, "flope_frame_finish: waiting for the poses failed");
  s.gap_n = s.n;
  int k = 0;
  for (int i = 0; i < s.n; ++i) {
    if (!s.rel_host[i]) continue;
    if (k >= cap || !poses_out) return ffail(f, FLOPE_EINVAL, "flope_frame_finish: poses_out too small");
    for (int j = 0; j < 16; ++j) poses_out[(size_t)k * 16 + j] = (double)s.Rt_host[(size_t)i * 16 + j];
    ++k;
  }
  return k;
}

// the slot's pose rows and reliability flags into a device tracker (track.hip), behind the slot's pose kernels on the stream
// flope_frame_enqueue ran on: the rows flope_frame_finish would return (it drops rel == 0 and widens float32 exactly; so does the
// tracker), without the host seeing a pose
extern "C" int flope_frame_track(flope_frame_handle f, int slot, flope_track_handle t, const double* cam16_host) {
  if (!f) return ffail(nullptr, FLOPE_EINVAL, "flope_frame_track: NULL handle");
  if (slot < 0 || slot >= f->nslots || !t || !cam16_host) return ffail(f, FLOPE_EINVAL, "flope_frame_track: bad slot / NULL tracker or camera pose");
  if (f->guard) return ffail(f, FLOPE_EINVAL, "flope_frame_track: a guarded frame handle repairs its poses in flope_frame_finish; track the rows it returns");
  Slot& s = f->slots[slot];
  if (s.state != 2) return ffail(f, FLOPE_ESTATE, "flope_frame_track: nothing enqueued in this slot");
  if (s.n == 0) return 0;
  const int rc = flope_track_update(t, s.Rt, 0, s.rel, s.n, cam16_host, s.stream);
  if (rc < 0) return ffail(f, rc, std::string("flope_frame_track: ") + flope_track_last_error(t));
  return 0;
}

extern "C" int flope_frame_to_poses(flope_frame_handle f, const float* det_dev, const int32_t* count_dev, int max_det, const uint8_t* frame_dev,
                                    const uint8_t* mask_dev, const void* depth_dev, int depth_format, float depth_div, const float* K4_host,
                                    float near_plane, float far_plane, double* poses_out, int cap, void* stream) {
  int rc = flope_frame_select(f, 0, det_dev, count_dev, max_det, stream);
  if (rc < 0) return rc;
  rc = flope_frame_enqueue(f, 0, frame_dev, mask_dev, depth_dev, depth_format, depth_div, K4_host, near_plane, far_plane, stream);
  if (rc < 0) return rc;
  return flope_frame_finish(f, 0, poses_out, cap);
}

// test hook: the boxes flope_frame_select kept (as detected / squared), int32 [n][4] each, after the count has arrived
extern "C" int flope_frame_read_boxes(flope_frame_handle f, int slot, int32_t* good_host, int32_t* sq_host, int cap) {
  if (!f || slot < 0 || slot >= f->nslots) return ffail(f, FLOPE_EINVAL, "flope_frame_read_boxes: bad handle / slot");
  Slot& s = f->slots[slot];
  if (s.state < 1) return ffail(f, FLOPE_ESTATE, "flope_frame_read_boxes: nothing selected in this slot");
  if (hipSetDevice(f->device) != hipSuccess || hipEventSynchronize(s.ev_sel) != hipSuccess) return ffail(f, FLOPE_EHIP, "flope_frame_read_boxes: wait failed");
  const int n = s.nsel_host[0];
  if (n > cap) return ffail(f, FLOPE_EINVAL, "flope_frame_read_boxes: buffers too small");
  if (n > 0 && (hipMemcpy(good_host, s.boxes, (size_t)n * 16, hipMemcpyDeviceToHost) != hipSuccess ||
                hipMemcpy(sq_host, s.boxes + (size_t)f->cap * 4, (size_t)n * 16, hipMemcpyDeviceToHost) != hipSuccess))
    return ffail(f, FLOPE_EHIP, "flope_frame_read_boxes: copy failed");
  return n;
}

// test hook (guarded handles): the guard's conditioning figure of every crop of the slot's last finished frame, float32 [n]; returns n
extern "C" int flope_frame_read_gaps(flope_frame_handle f, int slot, float* gap_host, int cap) {
  if (!f || slot < 0 || slot >= f->nslots) return ffail(f, FLOPE_EINVAL, "flope_frame_read_gaps: bad handle / slot");
  Slot& s = f->slots[slot];
  if (!f->guard || s.state == 2 || s.gap_n < 0) return ffail(f, FLOPE_ESTATE, "flope_frame_read_gaps: no finished frame of a guarded handle in this slot");
  if (s.gap_n > cap || (s.gap_n > 0 && !gap_host)) return ffail(f, FLOPE_EINVAL, "flope_frame_read_gaps: gap_host too small");
  if (s.gap_n > 0 && (hipSetDevice(f->device) != hipSuccess || hipMemcpy(gap_host, s.gap, (size_t)s.gap_n * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess))
    return ffail(f, FLOPE_EHIP, "flope_frame_read_gaps: copy failed");
  return s.gap_n;
}
