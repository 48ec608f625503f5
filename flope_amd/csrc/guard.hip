// flope_guard_*: the guarded mode.  The whole batch runs on the 16-bit trunk; the device measures the
// conditioning of every crop's own head output M (pose_math.h: gap(M) = s2 + sign(det M) s3, the quantity that amplifies the
// trunk's error dM into the rotation, |dR| gap <= 3 |dM|); the crops below a threshold -- and only those -- run again on the float32
// trunk and overwrite their rows.
//
//   flope_guard_forward   asynchronous: f16 forward into the caller's outputs; behind it, on the guard's own stream (forked from the
//                         caller's, joined by nobody but the host wait below), guard_select_kernel (gap per crop, the flagged crops'
//                         indices in ascending order, their number -- stored to mapped pinned host memory by the kernel itself), an event.
//   flope_guard_repair    waits on the host for that ONE integer (HIP grids are sized on the host; flope_frame_enqueue is the
//                         precedent).  0: nothing is launched.  Otherwise, in chunks of max_repair: guard_gather_kernel (flagged
//                         crops + their xyz rows -> a compact staging batch), flope_forward_poses on the float32 engine,
//                         guard_scatter_kernel (compact r9 / R / Rt rows -> rows idx[i] of the caller's outputs).
// A crop's float32 result does not depend on its position or its neighbours, so a repaired row is bit for bit
// the row a float32 forward of the whole batch would have written, and an unflagged row is the f16 engine's, untouched.
// The handle borrows both engines and owns small state only: per slot the index list, the count, its event and an r9 buffer for
// callers that pass none; the staging batch and the compact outputs exist once, because the float32 engine they feed exists once
// (two repairs can no more overlap than two forwards of one engine can).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include "guard.h"
#include "pose_math.h"

namespace {
thread_local std::string g_guard_error;

struct GSlot {
  int32_t* sel = nullptr;        // device [1 + maxB]: the number of flagged crops, then their indices (ascending)
  int* count_host = nullptr;     // pinned, mapped [1]: the select kernel stores the number here itself
  int* count_host_dev = nullptr; // the device's address of it
  float* r9_own = nullptr;       // device [maxB][9]: M of the f16 forward when the caller passes no r9 buffer
  hipEvent_t ev_fwd = nullptr, ev = nullptr;   // the f16 forward is done (caller's stream); the selection is done (the guard's stream)
  int state = 0;                 // 0 idle, 1 forward enqueued (awaits repair)
  int last_count = -1;           // flagged crops of the last repair (flope_guard_read_selection); -1: none yet
  // the armed call's arguments (the caller keeps the buffers alive and unchanged until repair returns)
  const void* x = nullptr; const float* xyz = nullptr; float *r9 = nullptr, *R = nullptr, *Rt = nullptr;
  int fmt = 0, batch = 0, nullify = 0;
};
}  // namespace

struct flope_guard {
  flope_handle fast = nullptr, exact = nullptr;
  int device = 0, H = 0, W = 0, maxB = 0, max_repair = 0, nslots = 0;
  float gap_min = 0.5f;
  GSlot* slots = nullptr;
  hipStream_t side = nullptr;    // the selection kernels run here, off the caller's stream (the next forward does not wait for them)
  void* stage_x = nullptr;       // [max_repair] crops, sized for float32
  float *stage_xyz = nullptr, *c_r9 = nullptr, *c_R = nullptr, *c_Rt = nullptr;   // [max_repair][3 / 9 / 9 / 16]
  std::string err;
};

namespace {
int gfail(flope_guard* g, int code, const std::string& msg) {
  if (g) g->err = msg;
  g_guard_error = msg;
  return code;
}

size_t crop_bytes(int H, int W, int fmt) { return (size_t)H * W * 3 * (fmt == FLOPE_IN_F32_NCHW ? 4 : (fmt == FLOPE_IN_U8_NHWC ? 1 : 2)); }

// One workgroup, four waves.  Per pass of 256 crops: a lane per crop, a ballot per wave, the waves' totals through LDS -- the rank of
// a flagged crop is the number of flagged crops in front of it, so the list is ascending and the same on every run (no atomics).
__global__ __launch_bounds__(256) void guard_select_kernel(const float* __restrict__ r9, int B, float gap_min, float* __restrict__ gap_out,
                                                           int32_t* __restrict__ sel, int* __restrict__ count_host) {
  __shared__ int wave_total[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int base = 0;
  for (int i0 = 0; i0 < B; i0 += 256) {
    const int i = i0 + (int)threadIdx.x;
    bool flag = false;
    if (i < B) {
      float M[9];
#pragma unroll
      for (int j = 0; j < 9; ++j) M[j] = r9[(size_t)i * 9 + j];
      const float gap = procrustes_gap3x3(M);
      if (gap_out) gap_out[i] = gap;
      flag = procrustes_gap_flagged(gap, gap_min);
    }
    const unsigned long long m = __ballot(flag);
    if (lane == 0) wave_total[wave] = __popcll(m);
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const int t = wave_total[w];
      before += w < wave ? t : 0;
      total += t;
    }
    if (flag) sel[1 + base + before + __popcll(m & ((1ull << lane) - 1ull))] = i;     // < 1 + B: at most one entry per crop
    base += total;
    __syncthreads();
  }
  // the number goes to the host as a plain store into mapped pinned memory: the event recorded behind this kernel releases it to the
  // system, and the copy engine's 4-byte transfer that would do the same costs more than this whole kernel
  if (threadIdx.x == 0) { sel[0] = base; *count_host = base; }
}

// Flagged crop idx[blockIdx.y] -> compact crop blockIdx.y, in words of T (the widest type that divides the crop's byte count and
// both base addresses: a crop is one contiguous byte range in every FLOPE_IN_* layout); block (0, i) also moves the xyz row.
template <typename T>
__global__ __launch_bounds__(256) void guard_gather_kernel(const T* __restrict__ x, const int32_t* __restrict__ idx, size_t words,
                                                           T* __restrict__ stage, const float* __restrict__ xyz, float* __restrict__ stage_xyz) {
  const int i = blockIdx.y;
  const size_t src = (size_t)idx[i] * words, dst = (size_t)i * words;
  for (size_t k = (size_t)blockIdx.x * 256 + threadIdx.x; k < words; k += (size_t)gridDim.x * 256) stage[dst + k] = x[src + k];
  if (xyz && blockIdx.x == 0 && threadIdx.x < 3) stage_xyz[i * 3 + threadIdx.x] = xyz[(size_t)idx[i] * 3 + threadIdx.x];
}

// compact rows of the float32 forward -> rows idx[i] of the caller's outputs (34 floats per crop: r9, R, Rt; any may be absent)
__global__ __launch_bounds__(256) void guard_scatter_kernel(const int32_t* __restrict__ idx, int n, const float* __restrict__ c_r9,
                                                            const float* __restrict__ c_R, const float* __restrict__ c_Rt,
                                                            float* __restrict__ r9, float* __restrict__ R, float* __restrict__ Rt) {
  for (int t = blockIdx.x * 256 + threadIdx.x; t < n * 34; t += gridDim.x * 256) {
    const int i = t / 34, j = t - i * 34;
    const size_t row = (size_t)idx[i];
    if (j < 9) { if (r9) r9[row * 9 + j] = c_r9[i * 9 + j]; }
    else if (j < 18) { if (R) R[row * 9 + j - 9] = c_R[i * 9 + j - 9]; }
    else if (Rt) Rt[row * 16 + j - 18] = c_Rt[i * 16 + j - 18];
  }
}

template <typename T>
hipError_t launch_gather(const void* x, const int32_t* idx, size_t bytes, int n, void* stage, const float* xyz, float* stage_xyz, hipStream_t st) {
  const size_t words = bytes / sizeof(T);
  size_t bx = (words + 256 * 8 - 1) / (256 * 8);                   // ~8 words per thread, at most 128 blocks per crop
  bx = bx < 1 ? 1 : (bx > 128 ? 128 : bx);
  hipLaunchKernelGGL(guard_gather_kernel<T>, dim3((unsigned)bx, (unsigned)n), dim3(256), 0, st, (const T*)x, idx, words, (T*)stage, xyz, stage_xyz);
  return hipGetLastError();
}

void free_guard(flope_guard* g) {
  for (int i = 0; i < g->nslots && g->slots; ++i) {
    GSlot& s = g->slots[i];
    if (s.ev) { if (s.state == 1) hipEventSynchronize(s.ev); hipEventDestroy(s.ev); }
    if (s.ev_fwd) hipEventDestroy(s.ev_fwd);
    if (s.sel) hipFree(s.sel);
    if (s.r9_own) hipFree(s.r9_own);
    if (s.count_host) hipHostFree(s.count_host);
  }
  delete[] g->slots;
  if (g->side) { hipStreamSynchronize(g->side); hipStreamDestroy(g->side); }
  void* dev[] = {g->stage_x, g->stage_xyz, g->c_r9, g->c_R, g->c_Rt};
  for (void* p : dev) if (p) hipFree(p);
  delete g;
}
}  // namespace

extern "C" const char* flope_guard_last_error(flope_guard_handle g) { return g ? g->err.c_str() : g_guard_error.c_str(); }

extern "C" flope_handle flope_guard_fast_engine(flope_guard_handle g, int* slots) {
  if (!g) return nullptr;
  if (slots) *slots = g->nslots;
  return g->fast;
}

extern "C" int flope_guard_create(flope_handle fast, flope_handle exact, int max_repair, int slots, flope_guard_handle* out) {
  if (!out) return gfail(nullptr, FLOPE_EINVAL, "flope_guard_create: out is NULL");
  *out = nullptr;
  int fB = 0, fdt = 0, fh = 0, fw = 0, fdev = 0, eB = 0, edt = 0, eh = 0, ew = 0, edev = 0;
  if (!fast || !exact || fast == exact || flope_engine_geometry(fast, &fB, &fdt, &fh, &fw, &fdev) != FLOPE_OK ||
      flope_engine_geometry(exact, &eB, &edt, &eh, &ew, &edev) != FLOPE_OK)
    return gfail(nullptr, FLOPE_EINVAL, "flope_guard_create: two distinct PoseResNet engine handles are needed");
  if (fdt == FLOPE_DT_BF16)
    return gfail(nullptr, FLOPE_EINVAL, "flope_guard_create: a bf16 fast engine is refused: its error of M (2.3e-3) would need gap_min = 6.9, more than "
                                        "a rotation-like M has, so every crop would be repaired; use FLOPE_DT_F16");
  if (fdt != FLOPE_DT_F16) return gfail(nullptr, FLOPE_EINVAL, "flope_guard_create: the fast engine must be FLOPE_DT_F16");
  if (edt != FLOPE_DT_F32) return gfail(nullptr, FLOPE_EINVAL, "flope_guard_create: the exact engine must be FLOPE_DT_F32");
  if (fdev != edev || fh != eh || fw != ew || flope_engine_bod(fast) != flope_engine_bod(exact))
    return gfail(nullptr, FLOPE_EINVAL, "flope_guard_create: the two engines must share device, crop size and backbone_out_dim");
  if (max_repair < 1 || max_repair > eB)
    return gfail(nullptr, FLOPE_EINVAL, "flope_guard_create: max_repair must be within 1..max_batch of the exact engine (" + std::to_string(eB) + ")");
  if (slots < 1 || slots > 16) return gfail(nullptr, FLOPE_EINVAL, "flope_guard_create: 1..16 slots");
  if (hipSetDevice(fdev) != hipSuccess) return gfail(nullptr, FLOPE_EHIP, "flope_guard_create: hipSetDevice failed");
  flope_guard* g = new flope_guard();
  g->fast = fast; g->exact = exact; g->device = fdev; g->H = fh; g->W = fw; g->maxB = fB; g->max_repair = max_repair; g->nslots = slots;
  g->slots = new GSlot[slots];
  const size_t mr = (size_t)max_repair;
  bool ok = hipStreamCreateWithFlags(&g->side, hipStreamNonBlocking) == hipSuccess && hipMalloc(&g->stage_x, mr * crop_bytes(fh, fw, FLOPE_IN_F32_NCHW)) == hipSuccess &&
            hipMalloc((void**)&g->stage_xyz, mr * 3 * sizeof(float)) == hipSuccess && hipMalloc((void**)&g->c_r9, mr * 9 * sizeof(float)) == hipSuccess &&
            hipMalloc((void**)&g->c_R, mr * 9 * sizeof(float)) == hipSuccess && hipMalloc((void**)&g->c_Rt, mr * 16 * sizeof(float)) == hipSuccess;
  for (int i = 0; i < slots && ok; ++i) {
    GSlot& s = g->slots[i];
    ok = hipMalloc((void**)&s.sel, ((size_t)fB + 1) * sizeof(int32_t)) == hipSuccess && hipMalloc((void**)&s.r9_own, (size_t)fB * 9 * sizeof(float)) == hipSuccess &&
         hipHostMalloc((void**)&s.count_host, sizeof(int), hipHostMallocMapped | hipHostMallocCoherent) == hipSuccess &&
         hipHostGetDevicePointer((void**)&s.count_host_dev, s.count_host, 0) == hipSuccess &&
         hipEventCreateWithFlags(&s.ev, hipEventDisableTiming) == hipSuccess && hipEventCreateWithFlags(&s.ev_fwd, hipEventDisableTiming | hipEventDisableSystemFence) == hipSuccess;   // (orders two device streams only)
  }
  if (!ok) {
    free_guard(g);
    return gfail(nullptr, FLOPE_EHIP, "flope_guard_create: allocation failed");
  }
  *out = g;
  return FLOPE_OK;
}

extern "C" int flope_guard_destroy(flope_guard_handle g) {
  if (!g) return FLOPE_OK;
  hipSetDevice(g->device);
  free_guard(g);
  return FLOPE_OK;
}

extern "C" float flope_guard_set_gap_min(flope_guard_handle g, float gap_min) {
  if (!g) return -1.f;
  const float prev = g->gap_min;
  g->gap_min = gap_min;
  return prev;
}

extern "C" int flope_guard_forward(flope_guard_handle g, int slot, const void* x_dev, int in_format, int batch, const float* xyz_dev, int nullify_yaw,
                                   float* r9_dev, float* R_dev, float* Rt_dev, float* gap_dev, void* stream) {
  if (!g) return gfail(nullptr, FLOPE_EINVAL, "flope_guard_forward: NULL handle");
  if (slot < 0 || slot >= g->nslots) return gfail(g, FLOPE_EINVAL, "flope_guard_forward: bad slot");
  GSlot& s = g->slots[slot];
  if (s.state != 0) return gfail(g, FLOPE_ESTATE, "flope_guard_forward: the slot awaits flope_guard_repair");
  if (!R_dev && !Rt_dev && !r9_dev) return gfail(g, FLOPE_EINVAL, "flope_guard_forward: no output buffer");
  // (x_dev, in_format and batch are judged by the engine; a refused forward leaves the slot idle)
  float* r9 = r9_dev ? r9_dev : s.r9_own;
  const int rc = Rt_dev ? flope_forward_poses(g->fast, x_dev, in_format, batch, xyz_dev, nullify_yaw, r9, R_dev, Rt_dev, stream)
                        : flope_forward(g->fast, x_dev, in_format, batch, r9, R_dev, stream);
  if (rc != FLOPE_OK) return gfail(g, rc, std::string("flope_guard_forward: ") + flope_last_error(g->fast));
  // the selection forks off the caller's stream and is never joined to it: only flope_guard_repair (host) waits for it, so it
  // overlaps whatever the caller enqueues next (r9 / gap are the caller's to leave alone until repair returns)
  if (hipEventRecord(s.ev_fwd, (hipStream_t)stream) != hipSuccess || hipStreamWaitEvent(g->side, s.ev_fwd, 0) != hipSuccess)
    return gfail(g, FLOPE_EHIP, "flope_guard_forward: forking the selection failed");
  hipLaunchKernelGGL(guard_select_kernel, dim3(1), dim3(256), 0, g->side, (const float*)r9, batch, g->gap_min, gap_dev, s.sel, s.count_host_dev);
  if (hipGetLastError() != hipSuccess || hipEventRecord(s.ev, g->side) != hipSuccess) {
    hipStreamSynchronize(g->side);                    // nothing of a refused call may still be running when the caller reuses its buffers
    return gfail(g, FLOPE_EHIP, "flope_guard_forward: select launch / event failed");
  }
  s.x = x_dev; s.xyz = xyz_dev; s.r9 = r9; s.R = R_dev; s.Rt = Rt_dev; s.fmt = in_format; s.batch = batch; s.nullify = nullify_yaw;
  s.state = 1;
  return FLOPE_OK;
}

extern "C" int flope_guard_repair(flope_guard_handle g, int slot, void* stream) {
  if (!g) return gfail(nullptr, FLOPE_EINVAL, "flope_guard_repair: NULL handle");
  if (slot < 0 || slot >= g->nslots) return gfail(g, FLOPE_EINVAL, "flope_guard_repair: bad slot");
  GSlot& s = g->slots[slot];
  if (s.state != 1) return gfail(g, FLOPE_ESTATE, "flope_guard_repair: call flope_guard_forward for this slot first");
  s.state = 0;                                        // whatever happens below, the slot is idle afterwards
  s.last_count = -1;
  if (hipSetDevice(g->device) != hipSuccess || hipEventSynchronize(s.ev) != hipSuccess)
    return gfail(g, FLOPE_EHIP, "flope_guard_repair: waiting for the number of flagged crops failed");
  const int n = *s.count_host;
  if (n < 0 || n > s.batch) return gfail(g, FLOPE_EHIP, "flope_guard_repair: the device reported " + std::to_string(n) + " flagged crops of " + std::to_string(s.batch));
  s.last_count = n;
  if (n == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  const size_t cb = crop_bytes(g->H, g->W, s.fmt);
  const uintptr_t align = (uintptr_t)cb | (uintptr_t)s.x | (uintptr_t)g->stage_x;
  for (int off = 0; off < n; off += g->max_repair) {
    const int m = n - off < g->max_repair ? n - off : g->max_repair;
    const int32_t* idx = s.sel + 1 + off;
    float* sxyz = s.xyz ? g->stage_xyz : nullptr;
    hipError_t e;
    if (align % 16 == 0) e = launch_gather<uint4>(s.x, idx, cb, m, g->stage_x, s.xyz, sxyz, st);
    else if (align % 4 == 0) e = launch_gather<uint32_t>(s.x, idx, cb, m, g->stage_x, s.xyz, sxyz, st);
    else if (align % 2 == 0) e = launch_gather<uint16_t>(s.x, idx, cb, m, g->stage_x, s.xyz, sxyz, st);
    else e = launch_gather<uint8_t>(s.x, idx, cb, m, g->stage_x, s.xyz, sxyz, st);
    if (e != hipSuccess) return gfail(g, FLOPE_EHIP, "flope_guard_repair: gather launch failed");
    const int rc = flope_forward_poses(g->exact, g->stage_x, s.fmt, m, sxyz, s.nullify, g->c_r9, g->c_R, g->c_Rt, stream);
    if (rc != FLOPE_OK) return gfail(g, rc, std::string("flope_guard_repair: ") + flope_last_error(g->exact));
    hipLaunchKernelGGL(guard_scatter_kernel, dim3((unsigned)((m * 34 + 255) / 256)), dim3(256), 0, st, idx, m, (const float*)g->c_r9, (const float*)g->c_R,
                       (const float*)g->c_Rt, s.r9, s.R, s.Rt);
    if (hipGetLastError() != hipSuccess) return gfail(g, FLOPE_EHIP, "flope_guard_repair: scatter launch failed");
  }
  return n;
}

extern "C" int flope_guard_cancel(flope_guard_handle g, int slot) {
  if (!g || slot < 0 || slot >= g->nslots) return FLOPE_EINVAL;
  GSlot& s = g->slots[slot];
  if (s.state == 1) { hipSetDevice(g->device); hipEventSynchronize(s.ev); }
  s.state = 0;
  return FLOPE_OK;
}

extern "C" int flope_guard_forward_repaired(flope_guard_handle g, const void* x_dev, int in_format, int batch, const float* xyz_dev, int nullify_yaw,
                                            float* r9_dev, float* R_dev, float* Rt_dev, float* gap_dev, void* stream) {
  const int rc = flope_guard_forward(g, 0, x_dev, in_format, batch, xyz_dev, nullify_yaw, r9_dev, R_dev, Rt_dev, gap_dev, stream);
  if (rc < 0) return rc;
  return flope_guard_repair(g, 0, stream);
}

// test hook: the selection kernel with flope_guard_forward's launch shape and its mapped-host count, on a caller's M [n, 9]
extern "C" int flope_guard_select_rows(const float* M_dev, int n, float gap_min, float* gap_dev, int32_t* sel_dev, void* stream) {
  if (!M_dev || !sel_dev || n < 1) return gfail(nullptr, FLOPE_EINVAL, "flope_guard_select_rows: M_dev, sel_dev and n >= 1 are needed");
  int *count_host = nullptr, *count_dev = nullptr;
  if (hipHostMalloc((void**)&count_host, sizeof(int), hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess)
    return gfail(nullptr, FLOPE_EHIP, "flope_guard_select_rows: allocation failed");
  *count_host = -1;
  int rc = FLOPE_EHIP;
  if (hipHostGetDevicePointer((void**)&count_dev, count_host, 0) == hipSuccess) {
    hipLaunchKernelGGL(guard_select_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, M_dev, n, gap_min, gap_dev, sel_dev, count_dev);
    if (hipGetLastError() == hipSuccess && hipStreamSynchronize((hipStream_t)stream) == hipSuccess) rc = *count_host;
  }
  hipHostFree(count_host);
  if (rc < 0 || rc > n) return gfail(nullptr, FLOPE_EHIP, "flope_guard_select_rows: launch, wait or count failed");
  return rc;
}

// test hook: the flagged crops of the slot's last repair, ascending; returns their number
extern "C" int flope_guard_read_selection(flope_guard_handle g, int slot, int32_t* idx_host, int cap) {
  if (!g || slot < 0 || slot >= g->nslots) return gfail(g, FLOPE_EINVAL, "flope_guard_read_selection: bad handle / slot");
  GSlot& s = g->slots[slot];
  if (s.state != 0 || s.last_count < 0) return gfail(g, FLOPE_ESTATE, "flope_guard_read_selection: no finished repair in this slot");
  const int n = s.last_count;
  if (n > cap || (n > 0 && !idx_host)) return gfail(g, FLOPE_EINVAL, "flope_guard_read_selection: idx_host too small");
  if (n > 0 && (hipSetDevice(g->device) != hipSuccess || hipMemcpy(idx_host, s.sel + 1, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost) != hipSuccess))
    return gfail(g, FLOPE_EHIP, "flope_guard_read_selection: copy failed");
  return n;
}
