// C-ABI of the MI355X flower-pose hot path (include/flope_amd.h): engine handle,
// BatchNorm folding + MFMA weight packing, and the forward pass
//   crop batch -> PoseResNet trunk -> fp32 head -> special Procrustes.
// What every conv launches is decided in plan.h (host code without HIP); this file owns the device state and launches it.
// Reference behaviour restated: sunflower/models/posenet.py:5-34 (network),
// sunflower/utils/conversion.py:54-58 (Procrustes), eval-mode semantics throughout
// (BatchNorm running statistics, dropout = identity).
#include "../../include/flope_amd.h"
#include "common.h"
#include "host_pack.h"
#include "plan.h"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <string>
#include <vector>

// kernels (other translation units)
extern "C" int flope_conv_mfma_init();
extern "C" int flope_conv_mfma_launch(const ConvP* p, int dtype, int cfg, int patch, int nbuf, size_t lds, void* stream);
extern "C" int flope_stem_init();
extern "C" int flope_stem_launch(const StemP* p, int dtype, size_t lds, void* stream);
extern "C" int flope_maxpool_launch(const PoolP* p, int dtype, void* stream);
extern "C" int flope_avgpool_launch(const void* in, float* out, int B, int h, int w, int C, int dtype, void* stream);
extern "C" int flope_fc1_launch(const float* feat, const float* W1, const float* W1p, const float* b1, float* hidden, int B, int K, int N, void* stream);
extern "C" int flope_fc2_procrustes_launch(const float* hidden, const float* W2, const float* b2, float* r9, float* R, int B, int K, const float* xyz, int nullify, float* Rt, void* stream);
extern "C" int flope_fc2_procrustes_k4_launch(const float* hidden, const float* W2, const float* b2, float* r9, float* R, int B, int K, const float* xyz, int nullify, float* Rt, void* stream);
extern "C" int flope_prep_input_launch(const void* x, int in_format, int B, int H, int W, void* out, int Hip, int Wip, int dtype, void* stream);
extern "C" int flope_read_stage_launch(const void* in, float* out, int B, int C, int h, int w, int dtype, void* stream);
extern "C" int flope_naive_conv_launch(const NaiveConvP* p, void* stream);
extern "C" int flope_conv_f32m_init();
extern "C" int flope_conv_f32m_launch(const F32mConvP* p, int mp, int stem, int grid, size_t lds, size_t ws_bytes, void* stream);
extern "C" int flope_conv_stag_init();
extern "C" int flope_conv_gstag_init();
extern "C" int flope_conv_w4_init();
extern "C" int flope_conv_r4_init();
extern "C" int flope_conv_r4_launch(const ConvP* p, int dtype, int grid_blocks, void* stream);
extern "C" int flope_conv_s1r_init();
extern "C" int flope_conv_s1r_launch(const ConvP* p, const void* w, int dtype, int grid, int yw, void* stream);
extern "C" int flope_conv_s2r_init();
extern "C" int flope_conv_s2r_launch(const ConvP* p, const void* w, int dtype, int grid, void* stream);
extern "C" int flope_conv_w4_launch(const ConvP* p, int dtype, int grid_blocks, int mt, void* stream);
extern "C" int flope_conv_gstag_launch(const ConvP* p, int dtype, void* stream);
extern "C" int flope_conv_stag_launch(const ConvP* p, int dtype, int grid_blocks, size_t lds, void* stream);
extern "C" int flope_conv_split_finalize_launch(const ConvP* p, int dtype, void* stream);
extern "C" int flope_stem_pool_init();
extern "C" int flope_stem_pool_r_blocks_per_cu();
#ifdef FLOPE_STAG_DBG
extern "C" void flope_stem_pool_set_dbg(void* ptr);
#endif
extern "C" int flope_stem_pool_launch(const void* x, int in_format, int B, int H, int W, int Hs, int Ws_, int Hq, int Wq,
                                      const void* w, const void* w2, int* queues, const float* bias, void* out, int dtype, int persist_blocks, void* stream);

using namespace flope_host;
using namespace flope_plan;

namespace {

thread_local std::string g_last_error;

constexpr double kBnEps = 1e-5;
constexpr size_t kDbgRegion = 1 << 20;        // diagnostic builds: bytes of the split-K workspace per conv launch (clock stamps)
constexpr size_t kBufSlack = 1 << 20;         // conv_stag's fixed-size patch DMA may read this far past the last pixel (zeros)

// device images of a conv's folded weights (which of them exist: plan.h has_*_image)
enum Image {
  kWPacked,     // MFMA image (16-bit)
  kWStag,       // conv_stag image (16-bit), 3x3 Cin % 64 == 0
  kWS2r,        // conv_s2r fragment image (16-bit), the 3x3 stride-2 64 -> 128 conv only
  kWS1r,        // conv_s1r fragment image (16-bit), the 3x3 stride-1 128 -> 128 convs
  kWNaive,      // float [ky][kx][ci][cout], strict mode
  kWF32m,       // float A-fragment image of conv_f32m (float32 engines: uploaded beside kWNaive, option f32mfma picks per forward)
  kBias,        // float [cout]
  kWDsStag,     // downsample conv only: its weights as a conv_stag image
  kWDsS1r,      // the 64 -> 128 downsample conv only: its weights as conv_s1r's extra fragment pair
  kBiasFused,   // conv2 behind a downsample conv only: bias + bias of the downsample (the folded form)
  kImages
};

// device side of conv i (its shape and plan: flope_engine::plan.shape[i] / .conv[i])
struct ConvDev {
  int in_buf = -1, out_buf = -1, res_buf = -1;
  int ip_in = -1, ip_out = -1, ip_res = -1;   // the same under option inplace (map_buffers)
  void* img[kImages] = {nullptr};
  Launch last;                                // what the last forward's last slice launched for it (flope_launch_info)
};

struct Buf { void* ptr = nullptr; size_t bytes = 0; int C = 0, h = 0, w = 0; };

}  // namespace

struct flope_engine {
  int device = 0, H = 0, W = 0, maxB = 0, dtype = 0, bod = 2048;
  int esz = 2;                       // bytes per trunk element
  int num_cus = 256;
  PlanOptions opt;
  Plan plan;                         // stem geometry, conv shapes and their static plan under `opt`
  void* stem_in = nullptr; size_t stem_in_bytes = 0;
  int* stem_q = nullptr;               // tile queues of the register-weight stem: 1024 ints per batch slice (heads 256 bytes apart; zero between launches)
  void* stem_w = nullptr; void* stem_w2 = nullptr; float* stem_w_naive = nullptr; float* stem_w_f32m = nullptr; float* stem_bias = nullptr;   // stem_w2: per-wave fragment order (stem_pool_r_kernel)
  std::vector<Buf> bufs;             // 0 stem_out, 1 pool, then per block: mid, [ds], out
  std::vector<ConvDev> convs;
  int stage_buf[10];                 // FLOPE_STAGE_* (0..9) -> buffer index
  int mid_buf[8];                    // FLOPE_STAGE_MID(li, bi) - FLOPE_STAGE_MID(1, 0) -> buffer index
  int ds_buf[3] = {-1, -1, -1}, ds_conv[3] = {-1, -1, -1};   // FLOPE_STAGE_DS(li) - FLOPE_STAGE_DS(2) -> buffer / conv index
  bool last_ds_folded[3] = {false, false, false};            // the last forward computed that shortcut inside conv2
  int final_buf = -1;
  // option inplace: the second set of buffer indices (ConvDev::ip_*, ip_final: map_buffers) and what flope_read_stage needs to serve
  // the stages of a forward that ran under it
  int ip_final = -1;
  int stage_conv[10];                // FLOPE_STAGE_* (0..9) -> the conv that writes it (-1: stem, pool)
  int mid_conv[8];                   // FLOPE_STAGE_MID(li, bi) - FLOPE_STAGE_MID(1, 0) -> conv index
  std::vector<int> ip_last_writer;   // buffer -> the last conv of a forward under inplace that stores into it (-1: none)
  bool ip_now = false;               // the map the forward being enqueued uses (run_trunk)
  bool last_inplace = false;         // the last forward ran under inplace
  std::vector<int> last_ip_out, last_ip_writer;   // ... with this map (ConvDev::ip_out, ip_last_writer at that time)
  float *feat = nullptr, *hidden = nullptr, *W1 = nullptr, *W1p = nullptr, *b1 = nullptr, *W2 = nullptr, *b2 = nullptr;
  float* r9_scratch = nullptr;
  bool weights_loaded = false;
  float* split_ws = nullptr; size_t split_ws_bytes = 0;   // fp32 partial sums of the split-K path (small batches)
  hipStream_t side[4] = {nullptr, nullptr, nullptr, nullptr};
  hipEvent_t ev_fork = nullptr, ev_join[4] = {nullptr, nullptr, nullptr, nullptr};
  std::vector<hipEvent_t> ev;        // profile mode: one event before every launch + one after the last
  int ev_n = 0;
  std::vector<int> ev_slice;         // profile = 2: the slice whose stream recorded event i
  int last_batch = 0;
  bool last_fused = false;
  std::string err;
};

namespace {

int fail(flope_engine* e, int code, const std::string& msg) {
  if (e) e->err = msg;
  g_last_error = msg;
  return code;
}

#define HIP_TRY(e, call)                                                                   \
  do {                                                                                     \
    hipError_t _s = (call);                                                                \
    if (_s != hipSuccess)                                                                  \
      return fail(e, FLOPE_EHIP, std::string(#call) + ": " + hipGetErrorString(_s));       \
  } while (0)

#define K_TRY(e, what, call)                                                               \
  do {                                                                                     \
    int _s = (call);                                                                       \
    if (_s != 0)                                                                           \
      return fail(e, FLOPE_EHIP, std::string(what) + ": " + hipGetErrorString((hipError_t)_s)); \
  } while (0)

#define MARK(e, stream, slice)                                                             \
  do {                                                                                     \
    if ((e)->opt.profile && (e)->ev_n < (int)(e)->ev.size()) {                             \
      (e)->ev_slice[(e)->ev_n] = (slice);                                                  \
      HIP_TRY(e, hipEventRecord((e)->ev[(e)->ev_n++], (hipStream_t)(stream)));             \
    }                                                                                      \
  } while (0)

// option "lag": one wave that sleeps ~us microseconds at the head of the last slice's stream (bounded by the real-time clock)
__global__ void lag_kernel(int us) {
  const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();          // 100 MHz
  while (__builtin_amdgcn_s_memrealtime() - t0 < (unsigned long long)us * 100ull) __builtin_amdgcn_s_sleep(32);
}

// the buffers of conv c under the map in force for the forward being enqueued
int in_of(const flope_engine* e, const ConvDev& c) { return e->ip_now ? c.ip_in : c.in_buf; }
int out_of(const flope_engine* e, const ConvDev& c) { return e->ip_now ? c.ip_out : c.out_buf; }
int res_of(const flope_engine* e, const ConvDev& c) { return e->ip_now ? c.ip_res : c.res_buf; }

// a slice's view of buffer bi: every tensor is batch-major, so images [start, ..) are an offset into the same buffer
void* buf_at(const flope_engine* e, int bi, int start) {
  const Buf& b = e->bufs[bi];
  return (char*)b.ptr + (size_t)start * (b.h + 2) * (b.w + 2) * b.C * e->esz;
}

// kernel arguments of conv i of the slice [start, start + batch) as launch L asks for them; *pf: the finalize launch of a split-K
// launch (it owns bias / residual / ReLU)
void conv_params(const flope_engine* e, int i, const Launch& L, int start, int batch, ConvP* p, ConvP* pf) {
  const ConvShape& s = e->plan.shape[i];
  const ConvDev& c = e->convs[i];
  const bool stag_image = L.family != kMfma && L.family != kS2r;      // conv_stag and the kernels that share its weight image
  memset(p, 0, sizeof(*p));
  p->in = buf_at(e, in_of(e, c), start); p->out = buf_at(e, out_of(e, c), start);
  p->res = res_of(e, c) >= 0 ? buf_at(e, res_of(e, c), start) : nullptr;
  p->w = c.img[stag_image ? kWStag : kWPacked]; p->bias = (const float*)c.img[kBias];
  p->B = batch; p->Hip = s.hin + 2; p->Wip = s.win + 2; p->Cin = s.cin;
  p->Ho = s.hout; p->Wo = s.wout; p->Hop = s.hout + 2; p->Wop = s.wout + 2; p->Cout = s.cout;
  p->stride = s.stride; p->ntaps = s.k == 3 ? 9 : 1;
  p->M = batch * s.hout * s.wout; p->relu = s.relu; p->nchunks = s.cin / 64;
  p->per_image = L.per_image; p->tiles_per_image = L.tiles_per_image; p->nseg = L.nseg;
  p->mtiles = L.mtiles; p->ntiles = L.ntiles; p->patch_rows_max = L.patch_rounds; p->dbg = e->opt.dbg;
  if (stag_image) p->total_tiles = L.mtiles * L.ntiles;
  p->skew = L.skew; p->prio = L.prio;
  fastdiv_magic((unsigned)(s.hout * s.wout), &p->mg_hw, &p->sh_hw);
  fastdiv_magic((unsigned)s.wout, &p->mg_w, &p->sh_w);
  if (L.shortcut_folded) {
    const int di = e->plan.conv[i].ds_conv;
    const ConvShape& sd = e->plan.shape[di];
    p->res = nullptr; p->bias = (const float*)c.img[kBiasFused];
    p->ds_in = buf_at(e, in_of(e, e->convs[di]), start); p->ds_w = e->convs[di].img[L.family == kS1r ? kWDsS1r : kWDsStag];
    p->ds_Hip = sd.hin + 2; p->ds_Wip = sd.win + 2; p->ds_Cin = sd.cin;
  }
  if (L.ksplit > 1) {
    *pf = *p;
    p->ksplit = pf->ksplit = L.ksplit; p->split_ws = pf->split_ws = e->split_ws; p->res = nullptr;
  }
  p->res_lds = L.res_lds; p->cw_imgs = L.cw_imgs; p->dbg = L.dbg; p->dbg_lds_off = L.dbg_lds_off;
  if (L.family == kR4 || L.family == kW4) fastdiv_magic((unsigned)(p->Wip + 2), &p->mg_pitch, &p->sh_pitch);
  if (L.stamps && e->split_ws)                 // diagnostic build: clock stamps of this launch (flope_debug_read_ws)
    p->split_ws = e->split_ws + (size_t)i * (kDbgRegion / 4);
}

// Option inplace: the second set of buffer indices.  Every buffer stays allocated; a forward under the option walks the same
// launches and only names other buffers:
//   conv2 whose residual buffer has the output's shape (the block input, or the materialised shortcut): stores over that residual
//   conv2 behind a folded shortcut (no residual buffer; it reads the block input at stride 2): keeps its own buffer
//   conv1 of block X.1: stores into block X.0's conv1 buffer (same shape; X.0's conv2, its only reader, is done in stream order)
// so a layer touches two maps (three with a folded shortcut) instead of five, and every reuse distance is at most two maps.
// The zero rings are never stored to, so maps of one shape share a buffer freely; maps of different shapes never do.
// Depends on the plan (which shortcuts are folded): rebuilt after a replan.
//
// Only a conv2 aliases two of its own operands (res == out; its input is another buffer, so patch and halo reads never see a store
// of the same launch).  That is safe in a kernel when (a) no two tiles store the same pixel, (b) a residual element is read only by
// the tile that stores it, or read and discarded, and (c) every store depends on its residual load through data.  Per family:
//   conv_r4<RES>        whole 8-row bands; a lane loads rb + oconst[pt] (+ 64) by inline asm and stores ob + oconst[pt] (+ 64) behind
//                       the vmcnt(0) in front of sub-step 17; the next band's loads are issued after this band's stores (other pixels)
//   conv_w4<RES>        disjoint pixel ranges [m0, mend); a lane's residual pieces (LDS-DMA into idle slots, or registers in a class
//                       walk) are its own pixel's at ooff[pt]; the stores leave in line order -- another lane of the wave stores the
//                       pixel -- but only after the owner added its residual and wrote the wave's line image; lanes past mend are
//                       clamped to pixel mend - 1, which they read and never store (okl)
//   conv_stag<RES>      flat tiles, 512 x 64 tiles, 8-row bands and their 64-column segments: a lane loads and stores at the same
//                       out_off(pt); segments are disjoint in columns and lanes past Wo / mend are clamped, read and masked; the
//                       bands prefetch the residual of this workgroup's own next tile (nobody else stores it), res_lds pieces are
//                       the lane's own 16 bytes; the first tile's residual is loaded before anything is stored
//   split-K             the main launch has no residual; conv_split_finalize / conv_f32m_finalize: one thread, one load and one
//                       store at the same offset
//   conv_s1r<RES>       whole 4-row bands; rbase and obase carry the same opix and the same per-tile offset
//   conv_mfma, naive, conv_f32m   one lane / thread loads and stores the same elements, masked by m < mend / the grid bound
//   conv_gstag, conv_s2r, folded shortcuts (conv_w4 / conv_stag / conv_s1r DSF)   no residual buffer: never in place
// No kernel declares the residual or the output __restrict__ or loads the residual through a non-coherent path.  So every family
// with a residual buffer runs in place and none is held back.
void map_buffers(flope_engine* e) {
  const Plan& pl = e->plan;
  int cur = e->stage_buf[FLOPE_STAGE_POOL], mid = -1, ds = -1, mid0 = -1;
  e->ip_last_writer.assign(e->bufs.size(), -1);
  for (size_t i = 0; i < e->convs.size(); ++i) {
    const ConvShape& s = pl.shape[i];
    ConvDev& c = e->convs[i];
    c.ip_res = -1;
    if (s.role == kConv1) {
      c.ip_in = cur;
      if (s.bi == 0) mid0 = c.out_buf;
      c.ip_out = mid = s.bi == 0 ? c.out_buf : mid0;
    } else if (s.role == kShortcut) {
      c.ip_in = cur; c.ip_out = ds = c.out_buf;
    } else {
      c.ip_in = mid;
      const bool folded = pl.conv[i].ds_conv >= 0;
      c.ip_res = s.res == 2 ? ds : cur;
      c.ip_out = folded ? c.out_buf : c.ip_res;
      cur = c.ip_out;
    }
    e->ip_last_writer[c.ip_out] = (int)i;
  }
  e->ip_final = cur;
}

template <typename V>
int upload(flope_engine* e, const std::vector<V>& host, void** dev) {
  if (*dev) { hipFree(*dev); *dev = nullptr; }
  HIP_TRY(e, hipMalloc(dev, host.size() * sizeof(V)));
  HIP_TRY(e, hipMemcpy(*dev, host.data(), host.size() * sizeof(V), hipMemcpyHostToDevice));
  return 0;
}

struct Tensors {
  std::map<std::string, std::pair<const float*, std::vector<int64_t>>> t;
  const float* get(flope_engine* e, const std::string& name, const std::vector<int64_t>& shape, int* rc) const {
    auto it = t.find(name);
    if (it == t.end()) { *rc = fail(e, FLOPE_EWEIGHTS, "state_dict entry missing: " + name); return nullptr; }
    if (it->second.second != shape) {
      std::string got, want;
      for (auto d : it->second.second) got += std::to_string(d) + ",";
      for (auto d : shape) want += std::to_string(d) + ",";
      *rc = fail(e, FLOPE_EWEIGHTS, "size mismatch for " + name + ": got [" + got + "] expected [" + want + "]");
      return nullptr;
    }
    return it->second.first;
  }
};

// fold eval-mode BN into a bias-free conv: w' = w * g / sqrt(v + eps), b' = beta - mean * g / sqrt(v + eps)
int fold(flope_engine* e, const Tensors& ts, const std::string& conv, const std::string& bn, int cout, int cin,
         int k, std::vector<float>* wf, std::vector<float>* bf) {
  int rc = 0;
  const float* w = ts.get(e, conv + ".weight", {cout, cin, k, k}, &rc); if (!w) return rc;
  const float* g = ts.get(e, bn + ".weight", {cout}, &rc); if (!g) return rc;
  const float* b = ts.get(e, bn + ".bias", {cout}, &rc); if (!b) return rc;
  const float* m = ts.get(e, bn + ".running_mean", {cout}, &rc); if (!m) return rc;
  const float* v = ts.get(e, bn + ".running_var", {cout}, &rc); if (!v) return rc;
  const size_t per = (size_t)cin * k * k;
  wf->resize((size_t)cout * per); bf->resize(cout);
  double wmax = 0.0;
  for (int co = 0; co < cout; ++co) {
    const double scale = (double)g[co] / sqrt((double)v[co] + kBnEps);
    (*bf)[co] = (float)((double)b[co] - (double)m[co] * scale);
    for (size_t i = 0; i < per; ++i) {
      const double x = (double)w[co * per + i] * scale;
      (*wf)[co * per + i] = (float)x;
      if (!(fabs(x) <= 3.0e38)) return fail(e, FLOPE_EWEIGHTS, "non-finite folded weight in " + conv);
      wmax = std::max(wmax, fabs(x));
    }
    if (!std::isfinite((*bf)[co])) return fail(e, FLOPE_EWEIGHTS, "non-finite folded bias in " + bn);
  }
  if (e->dtype == FLOPE_DT_F16 && wmax > 6.0e4)
    return fail(e, FLOPE_EWEIGHTS, "folded weights of " + conv + " exceed the float16 range; use bf16 or f32");
  return 0;
}

}  // namespace

// ================================================================================
// A HIP stream whose kernels may only occupy the compute units set in `mask` (bit i of word i / 32 = CU i in the runtime's
// enumeration, which walks the XCDs round-robin).  The live loop gives the detector -- a chain of ~80 short, narrow
// launches -- its own CUs so that it never queues behind the pose network's full-chip grids (and vice versa).
extern "C" int flope_stream_create_cu_mask(int device_id, const uint32_t* mask, int words, void** out_stream) {
  if (!mask || words < 1 || words > 32 || !out_stream) return FLOPE_EINVAL;
  *out_stream = nullptr;
  bool any = false;
  for (int i = 0; i < words; ++i) any = any || mask[i] != 0;
  if (!any) return FLOPE_EINVAL;
  if (hipSetDevice(device_id) != hipSuccess) return FLOPE_EHIP;
  hipStream_t st = nullptr;
  if (hipExtStreamCreateWithCUMask(&st, (uint32_t)words, mask) != hipSuccess) { (void)hipGetLastError(); return FLOPE_EHIP; }
  *out_stream = st;
  return FLOPE_OK;
}

extern "C" int flope_stream_destroy(int device_id, void* stream) {
  if (!stream) return FLOPE_OK;
  if (hipSetDevice(device_id) != hipSuccess) return FLOPE_EHIP;
  return hipStreamDestroy((hipStream_t)stream) == hipSuccess ? FLOPE_OK : FLOPE_EHIP;
}

extern "C" const char* flope_version(void) { return "flope_amd 0.1 (gfx950; mfma_f32_16x16x32 bf16/f16; fp32 head)"; }

extern "C" int flope_engine_geometry(flope_handle h, int* max_batch, int* dtype, int* height, int* width, int* device_id) {
  if (!h) return FLOPE_EINVAL;
  if (max_batch) *max_batch = h->maxB;
  if (dtype) *dtype = h->dtype;
  if (height) *height = h->H;
  if (width) *width = h->W;
  if (device_id) *device_id = h->device;
  return FLOPE_OK;
}

// library-internal (guard.h): the guard checks that its two engines share the head's width
extern "C" int flope_engine_bod(flope_handle h) { return h ? h->bod : FLOPE_EINVAL; }

// which head kernels a forward of this handle launches under its current options (plan.h: head_plan, the launchers' own rule)
extern "C" int flope_head_plan(flope_handle h, int* fc1, int* fc2) {
  if (!h) return FLOPE_EINVAL;
  const HeadPlan hp = head_plan(h->opt, h->bod);
  if (fc1) *fc1 = hp.fc1;
  if (fc2) *fc2 = hp.fc2;
  return FLOPE_OK;
}

extern "C" const char* flope_last_error(flope_handle h) { return h ? h->err.c_str() : g_last_error.c_str(); }

extern "C" int flope_create(int device_id, int height, int width, int max_batch, int dtype, int backbone_out_dim,
                            flope_handle* out) {
  if (!out) return fail(nullptr, FLOPE_EINVAL, "flope_create: out is NULL");
  *out = nullptr;
  if (height < 32 || width < 32 || height > 4096 || width > 4096)
    return fail(nullptr, FLOPE_EINVAL, "flope_create: crop size must be within 32..4096");
  if (max_batch < 1) return fail(nullptr, FLOPE_EINVAL, "flope_create: max_batch must be >= 1");
  if (dtype < 0 || dtype > 2) return fail(nullptr, FLOPE_EINVAL, "flope_create: unknown dtype");
  if (backbone_out_dim < 1) return fail(nullptr, FLOPE_EINVAL, "flope_create: backbone_out_dim must be >= 1");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
    return fail(nullptr, FLOPE_EHIP, "flope_create: no HIP device visible (the product path has no CPU fallback)");
  if (device_id < 0 || device_id >= ndev) return fail(nullptr, FLOPE_EINVAL, "flope_create: bad device id");
  flope_engine* e = new flope_engine();
  e->device = device_id; e->H = height; e->W = width; e->maxB = max_batch; e->dtype = dtype; e->bod = backbone_out_dim;
  e->esz = dtype == FLOPE_DT_F32 ? 4 : 2;
  e->plan = make_plan(height, width, max_batch, dtype);
  replan(e->plan, e->opt);
  const Plan& pl = e->plan;
#define CREATE_TRY(call)                                                                         \
  do {                                                                                           \
    hipError_t _s = (call);                                                                      \
    if (_s != hipSuccess) {                                                                      \
      int _rc = fail(nullptr, FLOPE_EHIP, std::string(#call) + ": " + hipGetErrorString(_s));    \
      flope_destroy(e);                                                                          \
      return _rc;                                                                                \
    }                                                                                            \
  } while (0)
  CREATE_TRY(hipSetDevice(device_id));
  {
    hipDeviceProp_t prop;
    CREATE_TRY(hipGetDeviceProperties(&prop, device_id));
    e->num_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  }
  if (dtype != FLOPE_DT_F32) {
    int s = flope_conv_mfma_init();
    if (s == 0) s = flope_stem_init();
    if (s == 0) s = flope_stem_pool_init();
    if (s == 0) s = flope_conv_stag_init();
    if (s == 0) s = flope_conv_gstag_init();
    if (s == 0) s = flope_conv_w4_init();
    if (s == 0) s = flope_conv_r4_init();
    if (s == 0) s = flope_conv_s2r_init();
    if (s == 0) s = flope_conv_s1r_init();
    if (s != 0) { int rc = fail(nullptr, FLOPE_EHIP, std::string("kernel attribute setup: ") + hipGetErrorString((hipError_t)s)); flope_destroy(e); return rc; }
  }
  if (dtype == FLOPE_DT_F32) {
    const int s = flope_conv_f32m_init();
    if (s != 0) { int rc = fail(nullptr, FLOPE_EHIP, std::string("kernel attribute setup: ") + hipGetErrorString((hipError_t)s)); flope_destroy(e); return rc; }
  }
  const size_t B = (size_t)max_batch;
  e->stem_in_bytes = B * pl.sHip * pl.sWip * 4 * e->esz;
  CREATE_TRY(hipMalloc(&e->stem_in, e->stem_in_bytes));
  CREATE_TRY(hipMemset(e->stem_in, 0, e->stem_in_bytes));
  if (dtype != FLOPE_DT_F32 && pl.stem_lds > kLdsMax) {
    int rc = fail(nullptr, FLOPE_EINVAL, "flope_create: crop too wide for the stem kernel's LDS patch"); flope_destroy(e); return rc;
  }
  auto add_buf = [&](int C, int h, int w) {
    Buf b; b.C = C; b.h = h; b.w = w; b.bytes = B * (h + 2) * (w + 2) * C * e->esz + kBufSlack;
    e->bufs.push_back(b);
    return (int)e->bufs.size() - 1;
  };
  e->stage_buf[FLOPE_STAGE_STEM] = add_buf(64, pl.Hs, pl.Ws);
  e->stage_buf[FLOPE_STAGE_POOL] = add_buf(64, pl.Hq, pl.Wq);
  int cur = e->stage_buf[FLOPE_STAGE_POOL], b_mid = -1, b_ds = -1;      // block input, conv1's output, the shortcut conv's output
  for (const ConvShape& s : pl.shape) {
    ConvDev c;
    c.out_buf = add_buf(s.cout, s.hout, s.wout);
    c.in_buf = s.role == kConv2 ? b_mid : cur;
    if (s.role == kConv1) { b_mid = c.out_buf; e->mid_buf[(s.li - 1) * 2 + s.bi] = c.out_buf; e->mid_conv[(s.li - 1) * 2 + s.bi] = (int)e->convs.size(); }
    else if (s.role == kShortcut) {
      b_ds = c.out_buf;
      if (s.li >= 2) { e->ds_buf[s.li - 2] = c.out_buf; e->ds_conv[s.li - 2] = (int)e->convs.size(); }
    } else {
      c.res_buf = s.res == 2 ? b_ds : cur;
      e->stage_buf[FLOPE_STAGE_LAYER(s.li, s.bi)] = cur = c.out_buf;
      e->stage_conv[FLOPE_STAGE_LAYER(s.li, s.bi)] = (int)e->convs.size();
    }
    e->convs.push_back(c);
  }
  e->final_buf = cur;
  e->stage_conv[FLOPE_STAGE_STEM] = e->stage_conv[FLOPE_STAGE_POOL] = -1;
  map_buffers(e);
  if (pl.shape.back().hout < 1 || pl.shape.back().wout < 1) { int rc = fail(nullptr, FLOPE_EINVAL, "flope_create: crop too small"); flope_destroy(e); return rc; }
  for (Buf& b : e->bufs) {
    CREATE_TRY(hipMalloc(&b.ptr, b.bytes));
    CREATE_TRY(hipMemset(b.ptr, 0, b.bytes));          // the zero ring is written exactly once
  }
  CREATE_TRY(hipMalloc((void**)&e->feat, B * 512 * sizeof(float)));
  CREATE_TRY(hipMalloc((void**)&e->hidden, B * (size_t)e->bod * sizeof(float)));
  CREATE_TRY(hipMalloc((void**)&e->r9_scratch, B * 9 * sizeof(float)));
  if (dtype != FLOPE_DT_F32) {          // split-K partials: tiles * ksplit <= num_cus, 256 x 128 fp32 per tile share
    e->split_ws_bytes = (size_t)e->num_cus * 256 * 128 * sizeof(float);
    CREATE_TRY(hipMalloc((void**)&e->split_ws, e->split_ws_bytes));
    CREATE_TRY(hipMalloc((void**)&e->stem_q, 4 * 1024 * sizeof(int)));
    CREATE_TRY(hipMemset(e->stem_q, 0, 4 * 1024 * sizeof(int)));
  } else {                              // conv_f32m split-K partials (option f32m_ksplit): one round of the largest tile, plan.h
    e->split_ws_bytes = f32m_ws_bytes(e->num_cus);
    CREATE_TRY(hipMalloc((void**)&e->split_ws, e->split_ws_bytes));
  }
  for (int i = 0; i < 4; ++i) {
    CREATE_TRY(hipStreamCreateWithFlags(&e->side[i], hipStreamNonBlocking));
    CREATE_TRY(hipEventCreateWithFlags(&e->ev_join[i], hipEventDisableTiming));
  }
  CREATE_TRY(hipEventCreateWithFlags(&e->ev_fork, hipEventDisableTiming));
  e->ev.resize(4 * (e->convs.size() + 8) + 2);       // profile = 2: up to four slices' marks + the fork
  e->ev_slice.assign(e->ev.size(), 0);
  for (hipEvent_t& ev : e->ev) CREATE_TRY(hipEventCreate(&ev));
  CREATE_TRY(hipDeviceSynchronize());
#undef CREATE_TRY
  *out = e;
  return FLOPE_OK;
}

extern "C" int flope_destroy(flope_handle e) {
  if (!e) return FLOPE_OK;
  hipSetDevice(e->device);
  hipDeviceSynchronize();
  for (Buf& b : e->bufs) if (b.ptr) hipFree(b.ptr);
  for (ConvDev& c : e->convs)
    for (void* p : c.img) if (p) hipFree(p);
  void* singles[] = {e->stem_in, e->stem_q, e->stem_w, e->stem_w2, e->stem_w_naive, e->stem_w_f32m, e->stem_bias, e->feat, e->hidden, e->W1, e->W1p, e->b1, e->W2, e->b2, e->r9_scratch, e->split_ws};
  for (void* p : singles) if (p) hipFree(p);
  for (hipEvent_t ev : e->ev) hipEventDestroy(ev);
  for (int i = 0; i < 4; ++i) { if (e->side[i]) hipStreamDestroy(e->side[i]); if (e->ev_join[i]) hipEventDestroy(e->ev_join[i]); }
  if (e->ev_fork) hipEventDestroy(e->ev_fork);
  delete e;
  return FLOPE_OK;
}

// developer aid (diagnostic builds, -DFLOPE_STAG_DBG + option dbg = 64): copies `bytes` of the split-K workspace, where conv launch i
// of the last forward left its clock stamps at byte offset i * 1 MiB (kDbgRegion), to host memory
extern "C" int flope_debug_read_ws(flope_handle e, void* dst_host, size_t offset, size_t bytes) {
  if (!e || !dst_host) return fail(e, FLOPE_EINVAL, "flope_debug_read_ws: NULL argument");
  if (!e->split_ws || offset + bytes > e->split_ws_bytes) return fail(e, FLOPE_EINVAL, "flope_debug_read_ws: out of range");
  HIP_TRY(e, hipSetDevice(e->device));
  HIP_TRY(e, hipDeviceSynchronize());
  HIP_TRY(e, hipMemcpy(dst_host, (const char*)e->split_ws + offset, bytes, hipMemcpyDeviceToHost));
  return FLOPE_OK;
}

// the options, their clamps and which of them the static plan depends on: plan.h (option_table)
//   f32mfma (float32 engines; stored and ignored by the 16-bit ones): 1 = the stem and the 19 trunk convs run on conv_f32m_kernel
//   (exact-fp32 MFMA), 0 (default) = on naive_conv_kernel.  Both weight images are resident, so it may be flipped between forwards.
//   f32m_ksplit (float32 engines with f32mfma = 1; stored and ignored otherwise): split-K of conv_f32m for small batches, 0 (default)
//   = off, 1 = per launch by plan.h's cost model, 2..32 = that many shares wherever a split is allowed.  May be flipped between forwards.
extern "C" int flope_set_option(flope_handle e, const char* name, int value) {
  if (!e || !name) return fail(e, FLOPE_EINVAL, "flope_set_option: NULL argument");
  const OptionDef* d = find_option(name);
  if (!d) return fail(e, FLOPE_EINVAL, std::string("flope_set_option: unknown option ") + name);
  bool replans = false;
  const int prev = set_option(e->opt, name, value, &replans);
  if (d->member == &PlanOptions::profile) e->ev_n = 0;
  if (replans) { replan(e->plan, e->opt); map_buffers(e); }
  return prev;
}

extern "C" int flope_load_weights(flope_handle e, int n, const char* const* names, const float* const* host_ptrs,
                                  const int* ndims, const int64_t* const* shapes) {
  if (!e) return fail(nullptr, FLOPE_EINVAL, "flope_load_weights: NULL handle");
  if (n < 0 || (n > 0 && (!names || !host_ptrs || !ndims || !shapes)))
    return fail(e, FLOPE_EINVAL, "flope_load_weights: NULL argument");
  HIP_TRY(e, hipSetDevice(e->device));
  e->weights_loaded = false;
  Tensors ts;
  for (int i = 0; i < n; ++i) {
    if (!names[i] || !host_ptrs[i] || ndims[i] < 0 || ndims[i] > 8 || (ndims[i] > 0 && !shapes[i]))
      return fail(e, FLOPE_EINVAL, "flope_load_weights: malformed entry " + std::to_string(i));
    std::vector<int64_t> shp(shapes[i], shapes[i] + ndims[i]);
    ts.t[names[i]] = std::make_pair(host_ptrs[i], shp);
  }
  std::vector<float> wf, bf;
  std::vector<std::vector<float>> host_bias;   // folded-BN bias of every conv, in e->convs order
  int rc;
  // stem
  if ((rc = fold(e, ts, "base.conv1", "base.bn1", 64, 3, 7, &wf, &bf)) != 0) return rc;
  if ((rc = upload(e, bf, (void**)&e->stem_bias)) != 0) return rc;
  if (e->dtype == FLOPE_DT_F32) {
    if ((rc = upload(e, naive_layout(wf, 64, 3, 7), (void**)&e->stem_w_naive)) != 0) return rc;
    if ((rc = upload(e, pack_f32m_stem(wf), (void**)&e->stem_w_f32m)) != 0) return rc;
  }
  else {
    if ((rc = upload(e, pack_stem(wf, e->dtype), &e->stem_w)) != 0) return rc;
    if ((rc = upload(e, pack_stem_frag(wf, e->dtype), &e->stem_w2)) != 0) return rc;
  }
  for (size_t i = 0; i < e->convs.size(); ++i) {
    const ConvShape& s = e->plan.shape[i];
    ConvDev& c = e->convs[i];
    if ((rc = fold(e, ts, conv_name(s), conv_name(s, true), s.cout, s.cin, s.k, &wf, &bf)) != 0) return rc;
    if ((rc = upload(e, bf, &c.img[kBias])) != 0) return rc;
    if (e->dtype == FLOPE_DT_F32) {
      if ((rc = upload(e, naive_layout(wf, s.cout, s.cin, s.k), &c.img[kWNaive])) != 0) return rc;
      if ((rc = upload(e, pack_f32m(wf, s.cout, s.cin, s.k), &c.img[kWF32m])) != 0) return rc;
    }
    else {
      if ((rc = upload(e, pack_conv(wf, s.cout, s.cin, s.k, e->dtype), &c.img[kWPacked])) != 0) return rc;
      if (has_stag_image(s) && (rc = upload(e, pack_conv32(wf, s.cout, s.cin, e->dtype), &c.img[kWStag])) != 0) return rc;
      if (has_s1r_image(s) && (rc = upload(e, pack_s1r(wf, s.cin, e->dtype), &c.img[kWS1r])) != 0) return rc;
      if (has_s2r_image(s) && (rc = upload(e, pack_s2r(wf, s.cout, s.cin, e->dtype), &c.img[kWS2r])) != 0) return rc;
      if (has_ds_s1r_image(s) && (rc = upload(e, pack_s1r_ds(wf, s.cin, e->dtype), &c.img[kWDsS1r])) != 0) return rc;
      if (has_ds_stag_image(s) && (rc = upload(e, pack_conv32_1x1(wf, s.cout, s.cin, e->dtype), &c.img[kWDsStag])) != 0) return rc;
    }
    host_bias.push_back(bf);
  }
  // conv2 of a block with a shortcut conv: bias2 + bias_ds for the folded form (whether or not the plan uses it)
  for (size_t i = 0; i + 1 < e->convs.size(); ++i)
    if (e->plan.shape[i].role == kShortcut) {
      std::vector<float> sum = host_bias[i + 1];
      for (size_t j = 0; j < sum.size(); ++j) sum[j] += host_bias[i][j];
      if ((rc = upload(e, sum, &e->convs[i + 1].img[kBiasFused])) != 0) return rc;
    }
  // head (fp32 as stored)
  const float* w1 = ts.get(e, "base.fc.0.weight", {e->bod, 512}, &rc); if (!w1) return rc;
  const float* b1 = ts.get(e, "base.fc.0.bias", {e->bod}, &rc); if (!b1) return rc;
  const float* w2 = ts.get(e, "fc_rot.weight", {9, e->bod}, &rc); if (!w2) return rc;
  const float* b2 = ts.get(e, "fc_rot.bias", {9}, &rc); if (!b2) return rc;
  auto chk = [&](const float* p, size_t cnt, const char* nm) {
    for (size_t i = 0; i < cnt; ++i) if (!std::isfinite(p[i])) return fail(e, FLOPE_EWEIGHTS, std::string("non-finite value in ") + nm);
    return 0;
  };
  if ((rc = chk(w1, (size_t)e->bod * 512, "base.fc.0.weight")) || (rc = chk(b1, e->bod, "base.fc.0.bias")) ||
      (rc = chk(w2, (size_t)9 * e->bod, "fc_rot.weight")) || (rc = chk(b2, 9, "fc_rot.bias"))) return rc;
  if ((rc = upload(e, std::vector<float>(w1, w1 + (size_t)e->bod * 512), (void**)&e->W1)) != 0) return rc;
  if (e->bod % 16 == 0 && (rc = upload(e, flope_host::pack_fc1(w1, e->bod, 512), (void**)&e->W1p)) != 0) return rc;
  if ((rc = upload(e, std::vector<float>(b1, b1 + e->bod), (void**)&e->b1)) != 0) return rc;
  if ((rc = upload(e, std::vector<float>(w2, w2 + (size_t)9 * e->bod), (void**)&e->W2)) != 0) return rc;
  if ((rc = upload(e, std::vector<float>(b2, b2 + 9), (void**)&e->b2)) != 0) return rc;
  HIP_TRY(e, hipDeviceSynchronize());
  e->weights_loaded = true;
  return FLOPE_OK;
}

struct PoseOut { const float* xyz = nullptr; int nullify = 0; float* Rt = nullptr; };   // optional [B,16] pose assembly

// One slice [start, start + x.batch) of the crop batch through the trunk + fc.0 on `stream`: per conv, what decide() says.
// head: fc_rot + Procrustes of this slice on the slice's own stream (so a slice's head overlaps the other slice's
// trunk instead of running after the join); r9_dev / R_dev are the caller's full-batch buffers, head = false skips it.
static int run_slice(flope_engine* e, const void* x_dev, int in_format, int start, const SliceCtx& x, void* stream, bool marks,
                     bool head, float* r9_dev, float* R_dev, const PoseOut& po = PoseOut()) {
  const int dt = e->dtype, batch = x.batch;
  const Plan& pl = e->plan;
  const PlanOptions& o = e->opt;
  const size_t in_img_bytes = (size_t)e->H * e->W * 3 * (in_format == 0 ? 4 : (in_format == 3 ? 1 : 2));
  const char* xs = (const char*)x_dev + (size_t)start * in_img_bytes;
  char* stem_in = (char*)e->stem_in + (size_t)start * pl.sHip * pl.sWip * 4 * e->esz;
  float* feat = e->feat + (size_t)start * 512;
  float* hidden = e->hidden + (size_t)start * e->bod;
#define SMARK() do { if (marks) MARK(e, stream, x.slice); } while (0)
  void* stem_out = buf_at(e, e->stage_buf[FLOPE_STAGE_STEM], start);
  void* pool_out = buf_at(e, e->stage_buf[FLOPE_STAGE_POOL], start);
  const bool fused = o.fuse_stem && dt != FLOPE_DT_F32;
  if (fused) {
    SMARK();
#ifdef FLOPE_STAG_DBG
    flope_stem_pool_set_dbg(((o.dbg & 64) && e->split_ws) ? (void*)(e->split_ws + (size_t)30 * (kDbgRegion / 4)) : nullptr);
#endif
    // the register-weight form (weights in VGPRs, 51 KB of LDS: three workgroups per CU) where the option asks for it; else the
    // LDS-weight forms -- persistent where that measured faster (same-run A/B at B = 256: 224 x 224 crops +2.7 % on the step; 512 x 512
    // crops -7 % on the kernel.  stem_persist: 1 = auto, 2 = always, 0 = never)
    const bool stem_r = o.stem_r && e->stem_w2 && e->stem_q;
    K_TRY(e, "stem+maxpool", flope_stem_pool_launch(xs, in_format, batch, e->H, e->W, pl.Hs, pl.Ws, pl.Hq, pl.Wq, e->stem_w, stem_r ? e->stem_w2 : nullptr,
                                                   stem_r ? e->stem_q + 1024 * (x.slices > 1 ? x.slice : 0) : nullptr,
                                                   e->stem_bias, pool_out, dt,
                                                   stem_r ? flope_stem_pool_r_blocks_per_cu() * e->num_cus
                                                          : (o.stem_persist == 2 || (o.stem_persist == 1 && pl.Hq * pl.Wq <= 64 * 64)) ? 2 * e->num_cus : 0,
                                                   stream));
  } else {
    SMARK();
    K_TRY(e, "prep_input", flope_prep_input_launch(xs, in_format, batch, e->H, e->W, stem_in, pl.sHip, pl.sWip, dt, stream));
    if (dt == FLOPE_DT_F32 && o.f32mfma) {
      const Launch L = f32m_stem_launch(pl, x);
      F32mConvP p; memset(&p, 0, sizeof(p));
      p.in = (const float*)stem_in; p.out = (float*)stem_out; p.w = e->stem_w_f32m; p.bias = e->stem_bias;
      p.B = batch; p.Hip = pl.sHip; p.Wip = pl.sWip; p.Cin_stored = 4; p.Cin = 3; p.Ho = pl.Hs; p.Wo = pl.Ws;
      p.Hop = pl.Hs + 2; p.Wop = pl.Ws + 2; p.Cout = 64; p.KH = 7; p.KW = 7; p.stride = 2; p.in_off = 0; p.relu = 1;
      p.M = batch * pl.Hs * pl.Ws; p.nsteps = kF32mStemSteps;
      fastdiv_magic((unsigned)(pl.Hs * pl.Ws), &p.mg_hw, &p.sh_hw);
      fastdiv_magic((unsigned)pl.Ws, &p.mg_w, &p.sh_w);
      SMARK();
      K_TRY(e, "stem (fp32 MFMA)", flope_conv_f32m_launch(&p, L.mt, 1, L.grid, L.lds_bytes, 0, stream));
    } else if (dt == FLOPE_DT_F32) {
      NaiveConvP p; memset(&p, 0, sizeof(p));
      p.in = (const float*)stem_in; p.out = (float*)stem_out; p.w = e->stem_w_naive; p.bias = e->stem_bias;
      p.B = batch; p.Hip = pl.sHip; p.Wip = pl.sWip; p.Cin_stored = 4; p.Cin = 3; p.Ho = pl.Hs; p.Wo = pl.Ws;
      p.Hop = pl.Hs + 2; p.Wop = pl.Ws + 2; p.Cout = 64; p.KH = 7; p.KW = 7; p.stride = 2; p.in_off = 0; p.relu = 1;
      SMARK();
      K_TRY(e, "stem (fp32)", flope_naive_conv_launch(&p, stream));
    } else {
      StemP p; memset(&p, 0, sizeof(p));
      p.in = stem_in; p.out = stem_out; p.w = e->stem_w; p.bias = e->stem_bias;
      p.B = batch; p.Hip = pl.sHip; p.Wip = pl.sWip; p.Ho = pl.Hs; p.Wo = pl.Ws;
      p.tiles_per_image = pl.stem_tiles; p.patch_rows_max = pl.stem_rows;
      SMARK();
      K_TRY(e, "stem", flope_stem_launch(&p, dt, pl.stem_lds, stream));
    }
    PoolP pp; pp.in = stem_out; pp.out = pool_out; pp.B = batch; pp.Hip = pl.Hs + 2; pp.Wip = pl.Ws + 2; pp.C = 64; pp.Ho = pl.Hq; pp.Wo = pl.Wq;
    SMARK();
    K_TRY(e, "maxpool", flope_maxpool_launch(&pp, dt, stream));
  }
  for (size_t i = 0; i < e->convs.size(); ++i) {
    ConvDev& c = e->convs[i];
    const ConvShape& s = pl.shape[i];
    const Launch L = decide(o, pl, (int)i, x);
    if (x.slice == x.slices - 1) c.last = L;           // (under inline0 the last slice is not the last one enqueued)
    ConvP p, pf;
    if (L.family != kFolded && L.family != kNaive && L.family != kF32m) conv_params(e, (int)i, L, start, batch, &p, &pf);
    if (L.family != kFolded) SMARK();
    switch (L.family) {
      case kFolded: break;                           // computed inside the next launch (conv_stag DSF)
      case kNaive: {
        NaiveConvP q; memset(&q, 0, sizeof(q));
        q.in = (const float*)buf_at(e, in_of(e, c), start); q.out = (float*)buf_at(e, out_of(e, c), start);
        q.res = res_of(e, c) >= 0 ? (const float*)buf_at(e, res_of(e, c), start) : nullptr;
        q.w = (const float*)c.img[kWNaive]; q.bias = (const float*)c.img[kBias];
        q.B = batch; q.Hip = s.hin + 2; q.Wip = s.win + 2; q.Cin_stored = s.cin; q.Cin = s.cin; q.Ho = s.hout; q.Wo = s.wout;
        q.Hop = s.hout + 2; q.Wop = s.wout + 2; q.Cout = s.cout; q.KH = s.k; q.KW = s.k; q.stride = s.stride;
        q.in_off = s.k == 3 ? 0 : 1; q.relu = s.relu;
        K_TRY(e, conv_name(s).c_str(), flope_naive_conv_launch(&q, stream));
        break;
      }
      case kF32m: {
        F32mConvP q; memset(&q, 0, sizeof(q));
        q.in = (const float*)buf_at(e, in_of(e, c), start); q.out = (float*)buf_at(e, out_of(e, c), start);
        q.res = res_of(e, c) >= 0 ? (const float*)buf_at(e, res_of(e, c), start) : nullptr;
        q.w = (const float*)c.img[kWF32m]; q.bias = (const float*)c.img[kBias];
        q.B = batch; q.Hip = s.hin + 2; q.Wip = s.win + 2; q.Cin_stored = s.cin; q.Cin = s.cin; q.Ho = s.hout; q.Wo = s.wout;
        q.Hop = s.hout + 2; q.Wop = s.wout + 2; q.Cout = s.cout; q.KH = s.k; q.KW = s.k; q.stride = s.stride;
        q.in_off = s.k == 3 ? 0 : 1; q.relu = s.relu;
        q.M = batch * s.hout * s.wout; q.csteps = s.cin / 16; q.nsteps = f32m_steps(s.cin, s.k);
        fastdiv_magic((unsigned)(s.hout * s.wout), &q.mg_hw, &q.sh_hw);
        fastdiv_magic((unsigned)s.wout, &q.mg_w, &q.sh_w);
        if (L.ksplit > 1) { q.ksplit = L.ksplit; q.split_ws = e->split_ws; }   // split launch + finalize (which owns bias / residual / ReLU)
        K_TRY(e, conv_name(s).c_str(), flope_conv_f32m_launch(&q, L.mt, 0, L.grid, L.lds_bytes, e->split_ws_bytes, stream));
        break;
      }
      case kGstag: K_TRY(e, conv_name(s).c_str(), flope_conv_gstag_launch(&p, dt, stream)); break;
      case kS1r: K_TRY(e, conv_name(s).c_str(), flope_conv_s1r_launch(&p, c.img[kWS1r], dt, L.grid, o.coldyw, stream)); break;
      case kR4: K_TRY(e, conv_name(s).c_str(), flope_conv_r4_launch(&p, dt, L.grid, stream)); break;
      case kW4: K_TRY(e, conv_name(s).c_str(), flope_conv_w4_launch(&p, dt, L.grid, L.mt, stream)); break;
      case kStagFlat: case kStag512x64: case kStagBands:
        K_TRY(e, conv_name(s).c_str(), flope_conv_stag_launch(&p, dt, L.grid, L.lds_bytes, stream));
        if (L.ksplit > 1) K_TRY(e, conv_name(s).c_str(), flope_conv_split_finalize_launch(&pf, dt, stream));
        break;
      case kS2r: K_TRY(e, conv_name(s).c_str(), flope_conv_s2r_launch(&p, c.img[kWS2r], dt, L.grid, stream)); break;
      case kMfma: K_TRY(e, conv_name(s).c_str(), flope_conv_mfma_launch(&p, dt, L.cfg, L.patch, L.nbuf, L.lds_bytes, stream)); break;
    }
  }
  const int final_buf = e->ip_now ? e->ip_final : e->final_buf;
  const Buf& bl = e->bufs[final_buf];
  SMARK();
  K_TRY(e, "avgpool", flope_avgpool_launch(buf_at(e, final_buf, start), feat, batch, bl.h, bl.w, 512, dt, stream));
  SMARK();
  K_TRY(e, "fc1", flope_fc1_launch(feat, e->W1, o.fc1_packed ? e->W1p : nullptr, e->b1, hidden, batch, 512, e->bod, stream));
  if (head) {
    SMARK();
    float* r9 = (r9_dev ? r9_dev : e->r9_scratch) + (size_t)start * 9;
    float* Rp = R_dev ? R_dev + (size_t)start * 9 : nullptr;
    const float* xyzp = po.xyz ? po.xyz + (size_t)start * 3 : nullptr;
    float* Rtp = po.Rt ? po.Rt + (size_t)start * 16 : nullptr;
    int k4 = 0;
    if (o.fc2_k4) {
      k4 = flope_fc2_procrustes_k4_launch(hidden, e->W2, e->b2, r9, Rp, batch, e->bod, xyzp, po.nullify, Rtp, stream);
      if (k4 < 0) return fail(e, FLOPE_EHIP, "fc_rot+procrustes: launch failed");
    }
    if (!k4) K_TRY(e, "fc_rot+procrustes", flope_fc2_procrustes_launch(hidden, e->W2, e->b2, r9, Rp, batch, e->bod, xyzp, po.nullify, Rtp, stream));
  }
  SMARK();
#undef SMARK
  return FLOPE_OK;
}

// trunk + fc.0 for the whole batch.  With the "streams" option (default 2) and a large enough batch the
// crops are split into slices (plan.h: slices()) that run the same launch sequence on internal streams forked from /
// joined to the caller's stream: the tail of one slice's kernel (the last, partly filled round of
// workgroups -- up to 24 % of a launch at B = 256) overlaps the head of the other's.
static int run_trunk(flope_engine* e, const void* x_dev, int in_format, int batch, void* stream, bool head = false,
                     float* r9_dev = nullptr, float* R_dev = nullptr, const PoseOut& po = PoseOut()) {
  if (!e->weights_loaded) return fail(e, FLOPE_ESTATE, "forward before flope_load_weights");
  if (!x_dev) return fail(e, FLOPE_EINVAL, "forward: x_dev is NULL");
  if (batch < 1 || batch > e->maxB) return fail(e, FLOPE_EINVAL, "forward: batch must be within 1..max_batch");
  if (in_format < 0 || in_format > 3) return fail(e, FLOPE_EINVAL, "forward: unknown input format");
  HIP_TRY(e, hipSetDevice(e->device));               // the handle's device, whatever the caller's current device is
  e->ev_n = 0;
  e->last_fused = e->opt.fuse_stem && e->dtype != FLOPE_DT_F32;
  e->last_batch = batch;
  for (int i = 0; i < 3; ++i) e->last_ds_folded[i] = e->ds_conv[i] >= 0 && e->plan.conv[e->ds_conv[i]].folded;
  e->ip_now = e->last_inplace = e->opt.inplace != 0;
  if (e->ip_now) {
    e->last_ip_out.resize(e->convs.size());
    for (size_t i = 0; i < e->convs.size(); ++i) e->last_ip_out[i] = e->convs[i].ip_out;
    e->last_ip_writer = e->ip_last_writer;
  }
  const Slices sl = slices(e->opt, batch, e->opt.profile);
  const int ns = sl.n;
  if (ns == 1) return run_slice(e, x_dev, in_format, 0, slice_ctx(sl, 0, batch, e->num_cus), stream, true, head, r9_dev, R_dev, po);
  hipStream_t user = (hipStream_t)stream;
  if (e->opt.profile == 2) MARK(e, user, 0);          // time zero of flope_profile_timeline
  HIP_TRY(e, hipEventRecord(e->ev_fork, user));
  // each slice's whole sequence goes to its own stream; the hardware queues interleave them, and a slice's short tail round
  // overlaps another slice's next launch.  Time line (option profile = 2, tools/slice_timeline.py): the slices walk the same
  // layers side by side and finish within microseconds of each other.
  // Option inline0 (default): slice 0's sequence goes onto the caller's stream itself.  It starts without the hop from the caller's
  // queue to a side queue (first launch eligible 12 us after the fork instead of 28), the side slices start one hop later -- the
  // offset that option lag buys with a sleeping wave, which is therefore skipped -- and the join waits for one event fewer.  The
  // side slices are enqueued first, so that their barrier is armed before slice 0's launches fill the caller's queue (the other
  // order measured 0.3 - 0.6 % slower in three of four passes).  Same-run pairs, time lines: profiles/step_schedule_ab.txt, DESIGN.md 21.
  const int first_side = e->opt.inline0 ? 1 : 0;
  const bool marks = e->opt.profile == 2;
  int rc_all = FLOPE_OK, forked = first_side;              // side slices [first_side, forked) were forked
  for (int s = first_side; s < ns && rc_all == FLOPE_OK; ++s) {
    if (hipStreamWaitEvent(e->side[s], e->ev_fork, 0) != hipSuccess) { rc_all = fail(e, FLOPE_EHIP, "hipStreamWaitEvent(fork) failed"); break; }

    forked = s + 1;
    // the last slice starts ~20 us late (one sleeping wave): the time line (profile = 2) shows the slices walking the same layers
    // side by side, every pair of launches starting in the same microsecond -- i.e. their prologue fills and epilogue drains
    // coincide; a small offset is +0.7 .. +1.4 % on the step (5 .. 30 us all do; 80 us and more lose: profiles/r03_slice_lag.txt)
    // (measured at B = 256 x 224 x 224 only: applied from 192 crops up, where a step is >= 35 x the offset)
    if (e->opt.lag && !e->opt.inline0 && s == ns - 1 && batch >= 192) {
      hipLaunchKernelGGL(lag_kernel, dim3(1), dim3(64), 0, e->side[s], e->opt.lag);
      if (hipGetLastError() != hipSuccess) { rc_all = fail(e, FLOPE_EHIP, "lag kernel launch failed"); break; }
    }
    rc_all = run_slice(e, x_dev, in_format, sl.start[s], slice_ctx(sl, s, batch, e->num_cus), e->side[s], marks, head, r9_dev, R_dev, po);
  }
  if (e->opt.inline0 && rc_all == FLOPE_OK)
    rc_all = run_slice(e, x_dev, in_format, sl.start[0], slice_ctx(sl, 0, batch, e->num_cus), user, marks, head, r9_dev, R_dev, po);
  // join every stream that was forked -- also after a failed launch, so that work already queued on the side
  // streams stays ordered before the caller's next use of x / r9 / R / Rt (slice 0 under inline0 is on the caller's stream already)
  const std::string first_err = rc_all != FLOPE_OK ? e->err : std::string();
  for (int s = first_side; s < forked; ++s) {
    if (hipEventRecord(e->ev_join[s], e->side[s]) != hipSuccess || hipStreamWaitEvent(user, e->ev_join[s], 0) != hipSuccess) {
      hipStreamSynchronize(e->side[s]);
      if (rc_all == FLOPE_OK) rc_all = fail(e, FLOPE_EHIP, "joining the batch-slice streams failed");
    }
  }
  if (rc_all != FLOPE_OK) {
    if (!first_err.empty()) { e->err = first_err; g_last_error = first_err; }
    e->last_batch = 0;
  }
  return rc_all;
}

extern "C" int flope_forward(flope_handle e, const void* x_dev, int in_format, int batch, float* r9_dev, float* R_dev,
                             void* stream) {
  if (!e) return fail(nullptr, FLOPE_EINVAL, "flope_forward: NULL handle");
  return run_trunk(e, x_dev, in_format, batch, stream, true, r9_dev, R_dev);
}

extern "C" int flope_forward_poses(flope_handle e, const void* x_dev, int in_format, int batch, const float* xyz_dev,
                                   int nullify_yaw, float* r9_dev, float* R_dev, float* Rt_dev, void* stream) {
  if (!e) return fail(nullptr, FLOPE_EINVAL, "flope_forward_poses: NULL handle");
  if (!Rt_dev) return fail(e, FLOPE_EINVAL, "flope_forward_poses: Rt_dev is NULL");
  PoseOut po; po.xyz = xyz_dev; po.nullify = nullify_yaw != 0; po.Rt = Rt_dev;
  return run_trunk(e, x_dev, in_format, batch, stream, true, r9_dev, R_dev, po);
}

extern "C" int flope_extract_features(flope_handle e, const void* x_dev, int in_format, int batch, float* feat_dev,
                                      void* stream) {
  if (!e) return fail(nullptr, FLOPE_EINVAL, "flope_extract_features: NULL handle");
  if (!feat_dev) return fail(e, FLOPE_EINVAL, "flope_extract_features: feat_dev is NULL");
  int rc = run_trunk(e, x_dev, in_format, batch, stream);
  if (rc) return rc;
  HIP_TRY(e, hipMemcpyAsync(feat_dev, e->hidden, (size_t)batch * e->bod * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return FLOPE_OK;
}

extern "C" int flope_read_stage(flope_handle e, int stage, int batch, float* dst_dev, int64_t* dims_out, void* stream) {
  if (!e) return fail(nullptr, FLOPE_EINVAL, "flope_read_stage: NULL handle");
  if (!dst_dev || !dims_out) return fail(e, FLOPE_EINVAL, "flope_read_stage: NULL argument");
  if (batch < 1 || batch > e->maxB) return fail(e, FLOPE_EINVAL, "flope_read_stage: bad batch");
  HIP_TRY(e, hipSetDevice(e->device));
  if (stage == FLOPE_STAGE_FEAT || stage == FLOPE_STAGE_HIDDEN) {
    const int nn = stage == FLOPE_STAGE_FEAT ? 512 : e->bod;
    dims_out[0] = batch; dims_out[1] = nn; dims_out[2] = 1; dims_out[3] = 1;
    HIP_TRY(e, hipMemcpyAsync(dst_dev, stage == FLOPE_STAGE_FEAT ? e->feat : e->hidden, (size_t)batch * nn * sizeof(float),
                              hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return FLOPE_OK;
  }
  int bi = -1;
  if (stage >= 0 && stage <= 9) bi = e->stage_buf[stage];
  else if (stage >= FLOPE_STAGE_MID(1, 0) && stage <= FLOPE_STAGE_MID(4, 1)) bi = e->mid_buf[stage - FLOPE_STAGE_MID(1, 0)];
  else if (stage >= FLOPE_STAGE_DS(2) && stage <= FLOPE_STAGE_DS(4)) {
    if (e->last_ds_folded[stage - FLOPE_STAGE_DS(2)])
      return fail(e, FLOPE_ESTATE, "flope_read_stage: the shortcut activation is not materialised when the 1x1 conv is folded into conv2 (set option dsfuse=0)");
    bi = e->ds_buf[stage - FLOPE_STAGE_DS(2)];
  }
  if (bi < 0) return fail(e, FLOPE_EINVAL, "flope_read_stage: unknown stage");
  if (e->last_inplace) {           // the map of the last forward: a stage is where its conv stored it, if no later conv stored there too
    int conv = -1;
    if (stage >= 0 && stage <= 9) conv = e->stage_conv[stage];
    else if (stage >= FLOPE_STAGE_MID(1, 0) && stage <= FLOPE_STAGE_MID(4, 1)) conv = e->mid_conv[stage - FLOPE_STAGE_MID(1, 0)];
    else conv = e->ds_conv[stage - FLOPE_STAGE_DS(2)];
    if (conv >= 0) bi = e->last_ip_out[conv];
    if (e->last_ip_writer[bi] != conv)
      return fail(e, FLOPE_ESTATE, "flope_read_stage: a later conv stored over this activation under option inplace (set option inplace=0)");
  }
  if (stage == FLOPE_STAGE_STEM && e->last_fused)
    return fail(e, FLOPE_ESTATE, "flope_read_stage: the stem activation is not materialised by the fused stem+maxpool kernel (set option fuse_stem=0)");
  const Buf& b = e->bufs[bi];
  dims_out[0] = batch; dims_out[1] = b.C; dims_out[2] = b.h; dims_out[3] = b.w;
  K_TRY(e, "read_stage", flope_read_stage_launch(b.ptr, dst_dev, batch, b.C, b.h, b.w, e->dtype, stream));
  return FLOPE_OK;
}

extern "C" double flope_forward_flops(flope_handle e, int batch) {
  if (!e) return 0.0;
  double macs = (double)e->plan.Hs * e->plan.Ws * 64 * 147;
  for (const ConvShape& c : e->plan.shape) macs += (double)c.hout * c.wout * c.cout * c.cin * c.k * c.k;
  macs += 512.0 * e->bod + 9.0 * e->bod;
  return 2.0 * macs * batch;
}

extern "C" int flope_forward_launches(flope_handle e) { return e ? forward_launches(e->plan, e->opt) : 0; }

// profile mode ("profile" option): per-launch GPU time of the LAST flope_forward, from HIP
// events recorded on the caller's stream around every launch.  Synchronises on the last event.
extern "C" int flope_profile_read(flope_handle e, float* ms_out, int cap) {
  if (!e || !ms_out) return fail(e, FLOPE_EINVAL, "flope_profile_read: NULL argument");
  if (e->opt.profile != 1 || e->ev_n < 2) return fail(e, FLOPE_ESTATE, "flope_profile_read: no forward with option profile = 1 (profile = 2 records a time line: flope_profile_timeline)");
  HIP_TRY(e, hipEventSynchronize(e->ev[e->ev_n - 1]));
  const int n = std::min(cap, e->ev_n - 1);
  for (int i = 0; i < n; ++i) HIP_TRY(e, hipEventElapsedTime(&ms_out[i], e->ev[i], e->ev[i + 1]));
  return n;
}

// profile = 2: the last forward as it ran in production (slices on their own streams), as a time line: event i was recorded on
// slice slice_out[i]'s stream in front of that slice's next launch (behind its last one), ms_out[i] = milliseconds since the fork.
// Event 0 is the fork itself.  Returns the number of events.
extern "C" int flope_profile_timeline(flope_handle e, float* ms_out, int* slice_out, int cap) {
  if (!e || !ms_out || !slice_out) return fail(e, FLOPE_EINVAL, "flope_profile_timeline: NULL argument");
  if (e->opt.profile != 2 || e->ev_n < 2) return fail(e, FLOPE_ESTATE, "flope_profile_timeline: no forward with option profile = 2");
  HIP_TRY(e, hipSetDevice(e->device));
  HIP_TRY(e, hipDeviceSynchronize());
  const int n = std::min(cap, e->ev_n);
  for (int i = 0; i < n; ++i) {
    ms_out[i] = 0.f;
    if (i > 0) HIP_TRY(e, hipEventElapsedTime(&ms_out[i], e->ev[0], e->ev[i]));
    slice_out[i] = e->ev_slice[i];
  }
  return n;
}

// launch idx of flope_forward: "layer|kernel" label and its algorithmic FLOPs for `batch` crops.  After a forward: the kernels its
// last slice launched and their tiling; before one: what decide() gives for the last slice of a forward of `batch` crops.
extern "C" int flope_launch_info(flope_handle e, int idx, int batch, char* name, int name_cap, double* flops) {
  if (!e || !name || name_cap < 1 || !flops) return fail(e, FLOPE_EINVAL, "flope_launch_info: NULL argument");
  std::vector<Launch> L;
  if (e->last_batch > 0) for (const ConvDev& c : e->convs) L.push_back(c.last);
  else {
    const Slices sl = slices(e->opt, batch, e->opt.profile);
    L = decide_all(e->opt, e->plan, slice_ctx(sl, sl.n - 1, batch, e->num_cus));
  }
  int conv;
  const std::string s = launch_name(e->plan, e->opt, L, e->bod, idx, &conv, flops);
  if (s.empty()) return fail(e, FLOPE_EINVAL, "flope_launch_info: bad index");
  snprintf(name, name_cap, "%s", s.c_str());
  *flops *= batch;
  return FLOPE_OK;
}

// plan introspection for DESIGN.md / tests: writes one line per conv into buf
extern "C" int flope_describe_plan(flope_handle e, char* buf, int buflen) {
  if (!e || !buf || buflen < 1) return FLOPE_EINVAL;
  snprintf(buf, buflen, "%s", describe(e->plan, e->opt).c_str());
  return FLOPE_OK;
}
