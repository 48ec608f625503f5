// flope_track_*: FlowerModel.assign_meas_to_state (reference sunflower/predictor/flower_model.py:146-213) on the device, behind the
// frame handle -- DESIGN.md 45.  The state (anchors, filter means, p, hit counts, the track count, a sticky overflow flag, the last
// association) lives in device memory; one update is two launches and no host wait:
//
//   track_assoc_kernel   one wave per measurement, grid-strided.  Every lane builds the measurement (track_math.h: the same
//                        bits in all 64 lanes), the lanes stride over the anchors AS THEY STOOD AT THE START OF THE FRAME, and the
//                        argmin is reduced on (distance, index) pairs, so that equal distances go to the lower index whatever
//                        lane met them.  Writes the measurement and its candidate: a track, "unmatched" or "skipped".
//   track_apply_kernel   one workgroup.  Counts the unmatched measurements; more new tracks than fit set the flag and nothing of
//                        the frame is applied.  Otherwise an exclusive prefix count over the unmatched measurements (ballots and
//                        per-wave totals in LDS) hands out the new indices in measurement order, and the FIRST measurement matched
//                        to a track walks the later ones and applies that track's updates in measurement order on its own thread.
//
// Per-track arithmetic is one thread's, in the order of track_math.h; nothing depends on the grid or block size.  Updates of one
// handle are ordered by an event of the handle, whatever streams they were issued on.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string>
#include "../../include/flope_amd.h"
#include "track_math.h"

namespace {
thread_local std::string g_track_error;
constexpr int kGuardWords = 8;                  // sentinel words behind every state array (flope_track_debug_sentinels)
constexpr uint32_t kGuardWord = 0x7ac4e55du;
constexpr int kAssocBlock = 256, kApplyBlock = 256;

struct Cam { double m[16]; };
}  // namespace

struct flope_track {
  int device = 0, max_tracks = 0, max_meas = 0;
  double th = 0, q = 0, r = 0, p0 = 0;
  double *anchors = nullptr, *means = nullptr, *p = nullptr, *meas = nullptr;
  int32_t *hits = nullptr, *count = nullptr, *assoc = nullptr, *cand = nullptr;     // count[0] tracks, count[1] overflow flag
  hipEvent_t ev = nullptr;
  int last_n = -1;                               // measurements of the last update; -1: none since create / reset
  unsigned long long serial = 0;                 // updates that enqueued anything, never reset (flope_track_device_view)
  std::string err;
};

namespace {
int tfail(flope_track* t, int code, const std::string& msg) {
  if (t) t->err = msg;
  g_track_error = msg;
  return code;
}

template <typename Pose>
__global__ __launch_bounds__(kAssocBlock) void track_assoc_kernel(const Pose* __restrict__ Rt, const int32_t* __restrict__ rel, int n, Cam cam,
                                                                  const double* __restrict__ anchors, const int32_t* __restrict__ count,
                                                                  double th, double* __restrict__ meas, int32_t* __restrict__ cand) {
  const int lane = threadIdx.x & 63;
  const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, waves = (gridDim.x * blockDim.x) >> 6;
  const int T = count[0];
  for (int m = wave; m < n; m += waves) {
    if (rel && rel[m] == 0) {
      if (lane == 0) cand[m] = kTrackSkipped;
      continue;
    }
    double P[16], z[kTrackDim];
    for (int e = 0; e < 16; ++e) P[e] = (double)Rt[(size_t)m * 16 + e];       // float32 widens exactly
    track_measure(P, cam.m, z);
    double bd = INFINITY;
    int bi = -1;
    for (int t = lane; t < T; t += 64) {
      const double d = track_dist(z, anchors + (size_t)t * kTrackDim);
      if (track_better(d, t, bd, bi)) { bd = d; bi = t; }
    }
    for (int off = 32; off > 0; off >>= 1) {
      const double od = __shfl_xor(bd, off, 64);
      const int oi = __shfl_xor(bi, off, 64);
      if (track_better(od, oi, bd, bi)) { bd = od; bi = oi; }
    }
    if (lane == 0) {
      for (int c = 0; c < kTrackDim; ++c) meas[(size_t)m * kTrackDim + c] = z[c];
      cand[m] = track_match(bd, bi, th) ? bi : kTrackUnmatched;
    }
  }
}

__global__ __launch_bounds__(kApplyBlock) void track_apply_kernel(int n, int max_tracks, double q, double r, double p0, const double* __restrict__ meas,
                                                                  const int32_t* __restrict__ cand, double* __restrict__ anchors,
                                                                  double* __restrict__ means, double* __restrict__ p, int32_t* __restrict__ hits,
                                                                  int32_t* __restrict__ count, int32_t* __restrict__ assoc) {
  __shared__ int s_wave[kApplyBlock / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nwaves = blockDim.x >> 6;
  const int T0 = count[0];
  if (count[1] != 0) return;                     // an earlier update overflowed: nothing is applied until flope_track_reset
  int fresh = 0;                                 // measurements that open a track
  for (int base = 0; base < n; base += blockDim.x) {
    const int m = base + tid;
    fresh += __syncthreads_count(m < n && cand[m] == kTrackUnmatched);
  }
  if (fresh > max_tracks - T0) {                 // (every thread has read count[] before the barriers above)
    if (tid == 0) count[1] = 1;
    return;
  }
  int opened = 0;                                // tracks opened by the measurements before this pass
  for (int base = 0; base < n; base += blockDim.x) {
    const int m = base + tid;
    const int c = m < n ? cand[m] : kTrackSkipped;
    const unsigned long long bal = __ballot(c == kTrackUnmatched);
    if (lane == 0) s_wave[wave] = __popcll(bal);
    __syncthreads();
    int before = opened, pass = 0;
    for (int w = 0; w < nwaves; ++w) { if (w < wave) before += s_wave[w]; pass += s_wave[w]; }
    __syncthreads();
    opened += pass;
    if (m >= n) {
      // (a thread behind the last measurement only took part in the count)
    } else if (c == kTrackSkipped) {
      assoc[m] = kTrackSkipped;
    } else if (c == kTrackUnmatched) {
      const int t = T0 + before + __popcll(bal & ((1ull << lane) - 1ull));
      if (t < max_tracks) {                      // (always: fresh fits)
        for (int e = 0; e < kTrackDim; ++e) {
          const double v = meas[(size_t)m * kTrackDim + e];
          anchors[(size_t)t * kTrackDim + e] = v;
          means[(size_t)t * kTrackDim + e] = v;
        }
        p[t] = p0;
        hits[t] = 1;
        assoc[m] = -1 - t;
      }
    } else if (c >= 0 && c < T0) {
      assoc[m] = c;
      bool first = true;
      for (int e = 0; e < m && first; ++e) first = cand[e] != c;
      if (first) {                               // this thread alone touches track c in this frame
        double x[kTrackDim], z[kTrackDim], pc = p[c];
        int h = hits[c];
        for (int e = 0; e < kTrackDim; ++e) x[e] = means[(size_t)c * kTrackDim + e];
        for (int mm = m; mm < n; ++mm) {
          if (cand[mm] != c) continue;
          for (int e = 0; e < kTrackDim; ++e) z[e] = meas[(size_t)mm * kTrackDim + e];
          track_filter_update(x, &pc, z, q, r);
          ++h;
        }
        for (int e = 0; e < kTrackDim; ++e) means[(size_t)c * kTrackDim + e] = x[e];
        p[c] = pc;
        hits[c] = h;
      }
    }
  }
  if (tid == 0) count[0] = T0 + fresh;
}

template <typename T>
bool alloc_guarded(T** out, size_t elems) {
  // every state array ends in kGuardWords sentinel words, 8-byte aligned behind the payload
  const size_t bytes = (elems * sizeof(T) + 7) & ~(size_t)7;
  char* base = nullptr;
  if (hipMalloc((void**)&base, bytes + kGuardWords * sizeof(uint32_t)) != hipSuccess) return false;
  uint32_t g[kGuardWords];
  for (int i = 0; i < kGuardWords; ++i) g[i] = kGuardWord;
  *out = (T*)base;
  return hipMemset(base, 0, bytes) == hipSuccess && hipMemcpy(base + bytes, g, sizeof(g), hipMemcpyHostToDevice) == hipSuccess;
}

template <typename T>
int bad_guards(const T* arr, size_t elems) {
  if (!arr) return 0;
  const size_t bytes = (elems * sizeof(T) + 7) & ~(size_t)7;
  uint32_t g[kGuardWords];
  if (hipMemcpy(g, (const char*)arr + bytes, sizeof(g), hipMemcpyDeviceToHost) != hipSuccess) return kGuardWords;
  int bad = 0;
  for (int i = 0; i < kGuardWords; ++i) bad += g[i] != kGuardWord;
  return bad;
}

void free_track(flope_track* t) {
  if (t->ev) { hipEventSynchronize(t->ev); hipEventDestroy(t->ev); }
  void* dev[] = {t->anchors, t->means, t->p, t->meas, t->hits, t->count, t->assoc, t->cand};
  for (void* d : dev) if (d) hipFree(d);
  delete t;
}

// waits for the handle's last update; FLOPE_ESTATE once an update overflowed.  -> tracks
int settled_count(flope_track* t, const char* who) {
  if (hipSetDevice(t->device) != hipSuccess || hipEventSynchronize(t->ev) != hipSuccess) return tfail(t, FLOPE_EHIP, std::string(who) + ": waiting for the last update failed");
  int32_t c[2] = {0, 0};
  if (hipMemcpy(c, t->count, sizeof(c), hipMemcpyDeviceToHost) != hipSuccess) return tfail(t, FLOPE_EHIP, std::string(who) + ": copy failed");
  if (c[1] != 0) return tfail(t, FLOPE_ESTATE, std::string(who) + ": an update needed more than max_tracks (" + std::to_string(t->max_tracks) + ") tracks and was not applied; call flope_track_reset");
  return c[0];
}
}  // namespace

extern "C" const char* flope_track_last_error(flope_track_handle t) { return t ? t->err.c_str() : g_track_error.c_str(); }

extern "C" int flope_track_create(int device_id, int max_tracks, int max_meas, double dist_th_m, double q, double r, double p0, flope_track_handle* out) {
  if (!out) return tfail(nullptr, FLOPE_EINVAL, "flope_track_create: out is NULL");
  *out = nullptr;
  if (max_tracks < 1 || max_meas < 1) return tfail(nullptr, FLOPE_EINVAL, "flope_track_create: max_tracks and max_meas must be at least 1");
  const double par[4] = {dist_th_m, q, r, p0};
  const char* name[4] = {"dist_th_m", "q", "r", "p0"};
  for (int i = 0; i < 4; ++i)
    if (!(isfinite(par[i]) && par[i] > 0)) return tfail(nullptr, FLOPE_EINVAL, std::string("flope_track_create: ") + name[i] + " must be finite and positive");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return tfail(nullptr, FLOPE_EHIP, "flope_track_create: no HIP device");
  if (device_id < 0 || device_id >= ndev) return tfail(nullptr, FLOPE_EINVAL, "flope_track_create: no such device");
  if (hipSetDevice(device_id) != hipSuccess) return tfail(nullptr, FLOPE_EHIP, "flope_track_create: hipSetDevice failed");
  flope_track* t = nullptr;
  try {
    t = new flope_track();
  } catch (...) {
    return tfail(nullptr, FLOPE_EHIP, "flope_track_create: out of host memory");
  }
  t->device = device_id; t->max_tracks = max_tracks; t->max_meas = max_meas;
  t->th = dist_th_m; t->q = q; t->r = r; t->p0 = p0;
  const size_t T = (size_t)max_tracks, M = (size_t)max_meas;
  const bool ok = alloc_guarded(&t->anchors, T * kTrackDim) && alloc_guarded(&t->means, T * kTrackDim) && alloc_guarded(&t->p, T) &&
                  alloc_guarded(&t->hits, T) && alloc_guarded(&t->count, 2) && alloc_guarded(&t->assoc, M) && alloc_guarded(&t->cand, M) &&
                  alloc_guarded(&t->meas, M * kTrackDim) && hipEventCreateWithFlags(&t->ev, hipEventDisableTiming) == hipSuccess;
  if (!ok) {
    free_track(t);
    return tfail(nullptr, FLOPE_EHIP, "flope_track_create: allocation failed");
  }
  *out = t;
  return FLOPE_OK;
}

extern "C" int flope_track_destroy(flope_track_handle t) {
  if (!t) return FLOPE_OK;
  hipSetDevice(t->device);
  free_track(t);
  return FLOPE_OK;
}

extern "C" int flope_track_reset(flope_track_handle t) {
  if (!t) return tfail(nullptr, FLOPE_EINVAL, "flope_track_reset: NULL handle");
  // waits for the last update, then clears count and flag with a blocking copy: every later update is behind it
  const int32_t zero[2] = {0, 0};
  if (hipSetDevice(t->device) != hipSuccess || hipEventSynchronize(t->ev) != hipSuccess ||
      hipMemcpy(t->count, zero, sizeof(zero), hipMemcpyHostToDevice) != hipSuccess)
    return tfail(t, FLOPE_EHIP, "flope_track_reset: wait / copy failed");
  t->last_n = -1;
  return FLOPE_OK;
}

extern "C" int flope_track_update(flope_track_handle t, const void* Rt_dev, int rt_f64, const int32_t* rel_dev, int n, const double* cam16_host, void* stream) {
  if (!t) return tfail(nullptr, FLOPE_EINVAL, "flope_track_update: NULL handle");
  if (n < 0 || n > t->max_meas) return tfail(t, FLOPE_EINVAL, "flope_track_update: n = " + std::to_string(n) + " outside 0 .. max_meas (" + std::to_string(t->max_meas) + ")");
  if (n == 0) return FLOPE_OK;
  if (!Rt_dev || !cam16_host || (rt_f64 != 0 && rt_f64 != 1)) return tfail(t, FLOPE_EINVAL, "flope_track_update: NULL poses / camera pose, or rt_f64 not 0 or 1");
  if (hipSetDevice(t->device) != hipSuccess) return tfail(t, FLOPE_EHIP, "flope_track_update: hipSetDevice failed");
  hipStream_t st = (hipStream_t)stream;
  Cam cam;
  for (int i = 0; i < 16; ++i) cam.m[i] = cam16_host[i];
  if (hipStreamWaitEvent(st, t->ev, 0) != hipSuccess) return tfail(t, FLOPE_EHIP, "flope_track_update: hipStreamWaitEvent failed");
  const int waves_per_block = kAssocBlock / 64;
  const int grid = (n + waves_per_block - 1) / waves_per_block;
  if (rt_f64)
    hipLaunchKernelGGL(track_assoc_kernel<double>, dim3(grid), dim3(kAssocBlock), 0, st, (const double*)Rt_dev, rel_dev, n, cam, t->anchors, t->count, t->th, t->meas, t->cand);
  else
    hipLaunchKernelGGL(track_assoc_kernel<float>, dim3(grid), dim3(kAssocBlock), 0, st, (const float*)Rt_dev, rel_dev, n, cam, t->anchors, t->count, t->th, t->meas, t->cand);
  hipLaunchKernelGGL(track_apply_kernel, dim3(1), dim3(kApplyBlock), 0, st, n, t->max_tracks, t->q, t->r, t->p0, t->meas, t->cand, t->anchors, t->means, t->p,
                     t->hits, t->count, t->assoc);
  if (hipGetLastError() != hipSuccess || hipEventRecord(t->ev, st) != hipSuccess) return tfail(t, FLOPE_EHIP, "flope_track_update: launch failed");
  t->last_n = n;
  ++t->serial;
  return FLOPE_OK;
}

extern "C" int flope_track_device_view(flope_track_handle t, flope_track_view* out) {
  if (!t || !out) return tfail(t, FLOPE_EINVAL, "flope_track_device_view: NULL handle or view");
  out->assoc = t->assoc; out->meas = t->meas; out->means = t->means; out->count = t->count;
  out->event = (void*)t->ev;
  out->device = t->device; out->max_tracks = t->max_tracks; out->max_meas = t->max_meas; out->n = t->last_n;
  out->serial = t->serial;
  return FLOPE_OK;
}

extern "C" int flope_track_count(flope_track_handle t) {
  if (!t) return tfail(nullptr, FLOPE_EINVAL, "flope_track_count: NULL handle");
  return settled_count(t, "flope_track_count");
}

extern "C" int flope_track_read(flope_track_handle t, double* anchors, double* means, double* p, int32_t* hits, int cap) {
  if (!t) return tfail(nullptr, FLOPE_EINVAL, "flope_track_read: NULL handle");
  const int T = settled_count(t, "flope_track_read");
  if (T <= 0) return T;
  if (T > cap) return tfail(t, FLOPE_EINVAL, "flope_track_read: " + std::to_string(T) + " tracks, room for " + std::to_string(cap));
  const size_t row = kTrackDim * sizeof(double);
  if ((anchors && hipMemcpy(anchors, t->anchors, T * row, hipMemcpyDeviceToHost) != hipSuccess) ||
      (means && hipMemcpy(means, t->means, T * row, hipMemcpyDeviceToHost) != hipSuccess) ||
      (p && hipMemcpy(p, t->p, T * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) ||
      (hits && hipMemcpy(hits, t->hits, T * sizeof(int32_t), hipMemcpyDeviceToHost) != hipSuccess))
    return tfail(t, FLOPE_EHIP, "flope_track_read: copy failed");
  return T;
}

extern "C" int flope_track_read_assoc(flope_track_handle t, int32_t* assoc_host, int cap) {
  if (!t) return tfail(nullptr, FLOPE_EINVAL, "flope_track_read_assoc: NULL handle");
  const int T = settled_count(t, "flope_track_read_assoc");
  if (T < 0) return T;
  if (t->last_n < 0) return tfail(t, FLOPE_ESTATE, "flope_track_read_assoc: no update since create / reset");
  if (t->last_n > cap || !assoc_host) return tfail(t, FLOPE_EINVAL, "flope_track_read_assoc: assoc_host too small");
  if (hipMemcpy(assoc_host, t->assoc, (size_t)t->last_n * sizeof(int32_t), hipMemcpyDeviceToHost) != hipSuccess)
    return tfail(t, FLOPE_EHIP, "flope_track_read_assoc: copy failed");
  return t->last_n;
}

extern "C" int flope_track_debug_read(flope_track_handle t, double* anchors, double* means, double* p, int32_t* hits, int32_t* count2, int rows) {
  if (!t) return tfail(nullptr, FLOPE_EINVAL, "flope_track_debug_read: NULL handle");
  if (rows < 0 || rows > t->max_tracks || !anchors || !means || !p || !hits || !count2) return tfail(t, FLOPE_EINVAL, "flope_track_debug_read: NULL buffer or rows outside 0 .. max_tracks");
  const size_t row = kTrackDim * sizeof(double);
  if (hipSetDevice(t->device) != hipSuccess || hipEventSynchronize(t->ev) != hipSuccess ||
      hipMemcpy(count2, t->count, 2 * sizeof(int32_t), hipMemcpyDeviceToHost) != hipSuccess ||
      (rows > 0 && (hipMemcpy(anchors, t->anchors, rows * row, hipMemcpyDeviceToHost) != hipSuccess ||
                    hipMemcpy(means, t->means, rows * row, hipMemcpyDeviceToHost) != hipSuccess ||
                    hipMemcpy(p, t->p, rows * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess ||
                    hipMemcpy(hits, t->hits, rows * sizeof(int32_t), hipMemcpyDeviceToHost) != hipSuccess)))
    return tfail(t, FLOPE_EHIP, "flope_track_debug_read: wait / copy failed");
  return rows;
}

extern "C" int flope_track_debug_sentinels(flope_track_handle t) {
  if (!t) return tfail(nullptr, FLOPE_EINVAL, "flope_track_debug_sentinels: NULL handle");
  if (hipSetDevice(t->device) != hipSuccess || hipEventSynchronize(t->ev) != hipSuccess) return tfail(t, FLOPE_EHIP, "flope_track_debug_sentinels: wait failed");
  const size_t T = (size_t)t->max_tracks, M = (size_t)t->max_meas;
  return bad_guards(t->anchors, T * kTrackDim) + bad_guards(t->means, T * kTrackDim) + bad_guards(t->p, T) + bad_guards(t->hits, T) +
         bad_guards(t->count, 2) + bad_guards(t->assoc, M) + bad_guards(t->cand, M) + bad_guards(t->meas, M * kTrackDim);
}
