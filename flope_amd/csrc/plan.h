// Host-side launch planner of the pose network: options, the static plan of every conv, the batch slices and the decision
// what ONE conv of ONE slice launches (kernel family, tiling, grid, LDS bytes) -- plain integer / floating-point arithmetic, no
// HIP, shared by engine.hip (which owns device state and launches what decide() says), the `_ok` guards of the kernel files and
// tests/host_harness/harness.cpp (tests/test_host.py pins it against tests/golden/plan_matrix.json on the CPU).
#pragma once

#include "../../include/flope_amd.h"
#include "w4_sched.h"

#include <limits.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

namespace flope_plan {

constexpr size_t kLdsTwoBlocks = 80 * 1024;   // <= this: two workgroups per CU
constexpr size_t kLdsMax = 160 * 1024;
constexpr size_t kGstagLds = 3 * 32768 + 3 * 16384;
constexpr size_t kR4Lds = (size_t)2 * 5 * 8192 + 18 * 4096 + 4 * 2048;      // patch buffers, resident weights, line images
constexpr size_t kS1rLds = 2 * 4 * 6 * 32 * 64 + 4 * 14 * 1024;
constexpr size_t kS2rLds = 2 * 18 * 32 * 128;
constexpr size_t kF32mLds = kLdsTwoBlocks + 4096;   // conv_f32m: reserved, never touched -- more than half a CU's LDS = one workgroup per CU

// ---- options ---------------------------------------------------------------------------------------------------------------
struct PlanOptions {
  int patch = 1;         // conv_mfma: pixel tiles from an LDS patch (3x3 stride 1) instead of gathered
  int bm256 = 1;         // conv_mfma: 256-pixel tiles for the 64-channel layers
  int persist = 0;       // conv_stag flat tiles on a persistent grid (one workgroup per CU)
  int rows_grid = 0;     // layer-1 persistent grid: 0 = one workgroup per CU, -1 = the slice's share of the CUs, > 0 = that many
  int split = 0;         // 0: default halves; 1..100: percent of the batch in slice 0; > 100: (value - 100) images
  int fc1_packed = 1;
  int w4mtlo = 0;        // smallest tile height the per-launch choice may take (0: 7 with two slices in flight, 5 alone)
  int lag = 20;          // inline0 = 0 only: microseconds by which the last batch slice starts late (0 = off)
  int w4mt = 0;          // conv_w4 tile height: 0 = per launch, 5..8 = 160..256 pixels (where the shape has that instantiation)
  int fc2_k4 = 1;        // fc_rot: K split over the four waves of a workgroup per image
  int ksplit = 1;        // 2: always the largest split
  int stem_r = 1;        // 1: the register-weight stem (three workgroups per CU); 0: the LDS-weight forms (stem_persist)
  int stem_persist = 1;  // LDS-weight stem: 1 = persistent where that measured faster, 2 = always, 0 = never
  int rowseg = 1;        // layer 1 on maps wider than 64 columns: 8-row bands cut into 64-column segments
  int skew = 1;          // conv_stag / conv_w4: LDS patch rows at pitch W + 4 (conflict-free fragment reads across row wraps)
  int r4 = 1;            // layer 1 (64 -> 64 on the 56-wide map) on conv_r4
  int s1r = 1;           // 1: layer2.0.conv2 / layer2.1.conv1 / conv2 on conv_s1r (224^2 crops), 0: conv_w4
  int s2r_grid = 0;      // workgroups of a conv_s2r launch (0: one per CU)
  int s2r = 1;           // 1: layer2.0.conv1 on conv_s2r (224^2 crops), 0: conv_mfma<gather>
  int w4 = 1;            // 0 = conv_stag for the flat 256 x 128 tiles, 1 = conv_w4 (4 waves)
  int w4cw = 4;          // conv_w4 class walk: tiles per persistent workgroup aimed at (0 / 1 = one tile per workgroup)
  int w4cwf = 0;         // ... bit 0: also with several batch slices in flight, bit 1: also where the walk fills < 85 % of the slice's CUs
  int prio = 0;          // conv_stag: 1 = s_setprio 1 for waves 4..7, 2 = for waves 0..3
  int reslds = 1;        // conv_stag flat tiles: the residual arrives by LDS-DMA
  int gstag = 1;         // 1 = Cin >= 128 (K = 576 is too short to amortise the 8-wave prologue), 2 = every stride-2 3x3
  int dsfuse = 1;        // fold a block's 1x1 stride-2 shortcut into its conv2
  int stag = 3;          // 0 off, 1 Cout >= 128 layers, 2 also the 64-channel layer (512 x 64 tiles), 3 64-channel layer as 8-row bands where the shape allows
  int streams = 2;       // batch slices in flight (each on its own stream)
  int fuse_stem = 1;     // input conversion + stem + max-pool in one launch
  int ldspad = 0;        // conv_mfma: KB of LDS added to a launch (occupancy experiments)
  int dbg = 0;           // diagnostic builds: ablation bits, 64 / 128 = clock stamps
  int nbuf = 2;          // conv_mfma ring depth asked for (3 where the weight tile is 16 KB per step)
  int f32mfma = 0;       // FLOPE_DT_F32 only: 1 = stem and trunk convs on the exact-fp32 MFMA (conv_f32m.hip), 0 = naive_conv_kernel (the checker)
  int f32m_ksplit = 0;   // FLOPE_DT_F32 with f32mfma = 1 only: 0 = off, 1 = split-K per launch by the cost model of f32m_ksplit(), 2..32 = force that share count (rounded down to 2 / 4 / 8 / 16 / 32) wherever a split is allowed
  int inline0 = 1;       // several batch slices: slice 0 runs on the caller's stream itself (no fork hop in front of it, one join fewer; the hop offsets the side slices, so lag's sleeping wave is skipped)
  int inplace = 0;       // 1: a BasicBlock's conv2 writes over its residual input and block X.1's conv1 over block X.0's conv1 output (engine.hip: map_buffers)
  int coldyw = 2;        // conv_s1r: 1 = the next band's LDS-DMA pieces are issued by the SIMD's younger waves (4-7) alone, at the head of their sub-tile; 2 = that, and the first band runs while the weights arrive (loaded four steps ahead in its step stream); 0 = pieces by all eight waves in their first three steps, all weights in front of the first band
  int profile = 0;       // 1: one slice, an event around every launch (flope_profile_read); 2: the slices as in production, events on every slice's stream (flope_profile_timeline)
};

// how set_option stores a value: kBool v != 0; kClamp lo..hi; kMask v & hi; kInOrZero lo..hi else 0; kZeroOrClamp <= 0 -> 0 else
// lo..hi; kNbuf 2 -> 2 else 3
enum OptionKind { kBool, kClamp, kMask, kInOrZero, kZeroOrClamp, kNbuf };
struct OptionDef { const char* name; int PlanOptions::*member; OptionKind kind; int lo, hi; bool replans; };

inline const std::vector<OptionDef>& option_table() {
  typedef PlanOptions O;
  static const std::vector<OptionDef> t = {
      {"patch", &O::patch, kBool, 0, 1, true},
      {"bm256", &O::bm256, kBool, 0, 1, true},
      {"persist", &O::persist, kBool, 0, 1, false},
      {"rows_grid", &O::rows_grid, kClamp, -1, INT_MAX, false},
      {"split", &O::split, kClamp, 0, INT_MAX, false},
      {"fc1_packed", &O::fc1_packed, kBool, 0, 1, false},
      {"w4mtlo", &O::w4mtlo, kZeroOrClamp, 5, 8, false},
      {"lag", &O::lag, kClamp, 0, 500, false},
      {"w4mt", &O::w4mt, kInOrZero, 5, 8, false},
      {"fc2_k4", &O::fc2_k4, kBool, 0, 1, false},
      {"ksplit", &O::ksplit, kClamp, 0, 2, false},
      {"stem_r", &O::stem_r, kBool, 0, 1, false},
      {"stem_persist", &O::stem_persist, kClamp, 0, 2, false},
      {"rowseg", &O::rowseg, kBool, 0, 1, true},
      {"skew", &O::skew, kBool, 0, 1, true},
      {"r4", &O::r4, kBool, 0, 1, false},
      {"s1r", &O::s1r, kBool, 0, 1, false},
      {"s2r_grid", &O::s2r_grid, kClamp, INT_MIN, INT_MAX, false},
      {"s2r", &O::s2r, kBool, 0, 1, false},
      {"w4", &O::w4, kBool, 0, 1, false},
      {"w4cw", &O::w4cw, kClamp, 0, 64, false},
      {"w4cwf", &O::w4cwf, kMask, 0, 3, false},
      {"prio", &O::prio, kClamp, 0, 2, false},
      {"reslds", &O::reslds, kBool, 0, 1, false},
      {"gstag", &O::gstag, kClamp, 0, 2, true},
      {"dsfuse", &O::dsfuse, kBool, 0, 1, true},
      {"stag", &O::stag, kClamp, 0, 3, true},
      {"streams", &O::streams, kClamp, 1, 4, false},
      {"fuse_stem", &O::fuse_stem, kBool, 0, 1, false},
      {"ldspad", &O::ldspad, kClamp, INT_MIN, INT_MAX, false},
      {"dbg", &O::dbg, kClamp, INT_MIN, INT_MAX, false},
      {"nbuf", &O::nbuf, kNbuf, 2, 3, true},
      {"profile", &O::profile, kClamp, 0, 2, false},
      {"f32mfma", &O::f32mfma, kBool, 0, 1, false},
      {"f32m_ksplit", &O::f32m_ksplit, kClamp, 0, 32, false},
      {"inline0", &O::inline0, kBool, 0, 1, false},
      {"inplace", &O::inplace, kBool, 0, 1, false},
      {"coldyw", &O::coldyw, kClamp, 0, 2, false},
  };
  return t;
}

inline const OptionDef* find_option(const char* name) {
  for (const OptionDef& d : option_table())
    if (std::string(d.name) == name) return &d;
  return nullptr;
}

// stores `value` as the option's kind says; returns the previous value, or FLOPE_EINVAL for a name find_option does not know
// (a stored value may be negative too: ask find_option where that matters).  *replan: the static plan depends on this option.
inline int set_option(PlanOptions& o, const char* name, int value, bool* replan) {
  const OptionDef* d = find_option(name);
  if (replan) *replan = d && d->replans;
  if (!d) return FLOPE_EINVAL;
  const int prev = o.*(d->member);
  const int clamped = value < d->lo ? d->lo : (value > d->hi ? d->hi : value);
  int v = clamped;
  switch (d->kind) {
    case kBool: v = value != 0; break;
    case kClamp: break;
    case kMask: v = value & d->hi; break;
    case kInOrZero: v = clamped == value ? value : 0; break;
    case kZeroOrClamp: v = value <= 0 ? 0 : clamped; break;
    case kNbuf: v = value == 2 ? 2 : 3; break;
  }
  o.*(d->member) = v;
  return prev;
}

// ---- the network's shapes -----------------------------------------------------------------------------------------------------
enum ConvRole { kConv1, kShortcut, kConv2 };     // of a BasicBlock; a shortcut conv (1x1) directly precedes the conv2 that adds it
struct ConvShape {
  int li = 0, bi = 0, role = kConv1;             // base.layer<li>.<bi>
  int cin = 0, cout = 0, k = 0, stride = 1;
  int hin = 0, win = 0, hout = 0, wout = 0;      // unpadded
  int res = 0;                                   // residual input: 0 none, 1 the block's input, 2 the shortcut conv in front of it
  int relu = 0;
};

inline std::string conv_name(const ConvShape& s, bool bn = false) {
  const std::string p = "base.layer" + std::to_string(s.li) + "." + std::to_string(s.bi);
  if (s.role == kShortcut) return p + (bn ? ".downsample.1" : ".downsample.0");
  return p + (bn ? ".bn" : ".conv") + (s.role == kConv1 ? "1" : "2");
}

// which weight images flope_load_weights builds for a conv (16-bit modes)
inline bool has_stag_image(const ConvShape& s) { return s.k == 3 && s.cin % 64 == 0; }
inline bool has_s1r_image(const ConvShape& s) { return s.k == 3 && s.stride == 1 && s.cin == 128 && s.cout == 128; }
inline bool has_s2r_image(const ConvShape& s) { return s.k == 3 && s.stride == 2 && s.cin == 64 && s.cout == 128; }
inline bool has_ds_s1r_image(const ConvShape& s) { return s.k == 1 && s.stride == 2 && s.cin == 64 && s.cout == 128; }
inline bool has_ds_stag_image(const ConvShape& s) { return s.k == 1 && s.cout >= 128 && s.cin % 64 == 0; }

inline int out_dim(int n, int k, int s, int p) { return (n + 2 * p - k) / s + 1; }

// ---- shape predicates of the special kernels ------------------------------------------------------------------------------------
// what a kernel's launch guard looks at, as plain ints (dims_of reads them from a ConvP)
struct ConvDims {
  int stride, ntaps, Cin, Cout, Ho, Wo, Hip, Wip, ksplit;
  bool res, ds, ds_w;                            // residual input; folded shortcut input and its weights
  int ds_Cin, ds_Hip, ds_Wip;
};
template <typename P>
inline ConvDims dims_of(const P& p) {
  return {p.stride, p.ntaps, p.Cin, p.Cout, p.Ho, p.Wo, p.Hip, p.Wip, p.ksplit, p.res != nullptr, p.ds_in != nullptr, p.ds_w != nullptr,
          p.ds_Cin, p.ds_Hip, p.ds_Wip};
}
inline bool r4_ok(const ConvDims& p) {
  return p.stride == 1 && p.ntaps == 9 && p.Cin == 64 && p.Cout == 64 && p.Wo == 56 && p.Ho % 8 == 0 &&
         10 * (p.Wip + 2) * 4 <= 5 * 512 && p.ksplit <= 1 && !p.ds;
}
inline bool s1r_ok(const ConvDims& p) {
  if (p.ds && !(p.ds_Cin == 64 && p.ds_Hip == 2 * p.Ho + 2 && p.ds_Wip == 2 * p.Wo + 2 && p.ds_w && !p.res)) return false;
  return p.stride == 1 && p.ntaps == 9 && p.Cin == 128 && p.Cout == 128 && p.Wo == 28 && (p.Ho & 3) == 0 &&
         p.ksplit <= 1 && p.Wip == p.Wo + 2 && p.Hip == p.Ho + 2;
}
inline bool s2r_ok(const ConvDims& p) {
  return p.stride == 2 && p.ntaps == 9 && p.Cin == 64 && p.Cout == 128 && p.Wo == 28 && (p.Ho & 3) == 0 && !p.res && !p.ds &&
         p.ksplit <= 1 && p.Wip == 2 * p.Wo + 2 && p.Hip == 2 * p.Ho + 2;
}
// LDS bytes of the conv_w4 variant (pt patch rounds, mt pixel tiles per wave, folded shortcut, class walk); 0 = not instantiated
inline size_t w4_lds(int pt, int mt, int dsf, int pers) {
  if (pt < 4 || pt > 6 || mt < 5 || mt > 8 || (mt < 7 && pt != 4) || (pers && (mt != 7 || pt > 5))) return 0;
  return w4_lds_bytes(pt, dsf && pers);
}

// ---- the static plan --------------------------------------------------------------------------------------------------------------
struct ConvPlan {
  int cfg = 0, patch = 0, nbuf = 2, per_image = 0, tiles_per_image = 0, ntiles = 0, rows_max = 0;   // conv_mfma
  size_t lds = 0;
  int stag = 0, stag_patch_bytes = 0, nseg = 1;  // stag: 0 conv_mfma, 1 flat tiles, 2 8-row bands, 3 conv_gstag
  size_t stag_lds = 0;
  int w4_patch[9] = {0};                         // conv_w4 on 32 mt-pixel tiles, mt = 5..7: patch rounds of such a tile (0: not available)
  // folded shortcut (conv_stag DSF): on a 1x1 downsample conv, folded = 1 means "computed inside layerX.0.conv2";
  // on that conv2, ds_conv is the index of the downsample
  int folded = 0, ds_conv = -1;
};

struct Plan {
  int H = 0, W = 0, maxB = 0, dtype = 0;
  // stem: 4 input channels, 3-pixel border, slack on the right/bottom for the kx=7 / ky pad taps
  int sHip = 0, sWip = 0, Hs = 0, Ws = 0, Hq = 0, Wq = 0, stem_tiles = 0, stem_rows = 0;
  size_t stem_lds = 0;
  std::vector<ConvShape> shape;
  std::vector<ConvPlan> conv;
};

inline void tile_dims(int cfg, int* BM, int* BN) {
  *BM = cfg == 2 ? 256 : 128;
  *BN = cfg == 1 ? 128 : 64;
}

// stem geometry and the 20 convs of the four layers
inline Plan make_plan(int H, int W, int maxB, int dtype) {
  Plan pl;
  pl.H = H; pl.W = W; pl.maxB = maxB; pl.dtype = dtype;
  pl.sHip = H + 6; pl.sWip = (W + 8 + 1) & ~1;
  pl.Hs = out_dim(H, 7, 2, 3); pl.Ws = out_dim(W, 7, 2, 3);
  const int HoWo = pl.Hs * pl.Ws;
  pl.stem_tiles = (HoWo + 255) / 256;
  int span = 1;
  for (int t = 0; t < pl.stem_tiles; ++t) {
    const int m0 = t * 256, me = std::min(m0 + 256, HoWo);
    span = std::max(span, (me - 1) / pl.Ws - m0 / pl.Ws + 1);
  }
  pl.stem_rows = 2 * (span - 1) + 7;
  pl.stem_lds = (size_t)7 * 64 * 64 + (size_t)pl.stem_rows * pl.sWip * 8;
  pl.Hq = out_dim(pl.Hs, 3, 2, 1); pl.Wq = out_dim(pl.Ws, 3, 2, 1);
  int ch = 64, hh = pl.Hq, ww = pl.Wq;
  const int couts[4] = {64, 128, 256, 512}, strides[4] = {1, 2, 2, 2};
  for (int li = 0; li < 4; ++li)
    for (int bi = 0; bi < 2; ++bi) {
      const int s = bi == 0 ? strides[li] : 1, co = couts[li];
      const int ho = out_dim(hh, 3, s, 1), wo = out_dim(ww, 3, s, 1);
      ConvShape c; c.li = li + 1; c.bi = bi;
      c.role = kConv1; c.cin = ch; c.cout = co; c.k = 3; c.stride = s; c.hin = hh; c.win = ww; c.hout = ho; c.wout = wo; c.relu = 1;
      pl.shape.push_back(c);
      const bool shortcut = bi == 0 && (s != 1 || ch != co);
      if (shortcut) { c.role = kShortcut; c.k = 1; c.relu = 0; pl.shape.push_back(c); }
      c.role = kConv2; c.cin = co; c.k = 3; c.stride = 1; c.hin = ho; c.win = wo; c.res = shortcut ? 2 : 1; c.relu = 1;
      pl.shape.push_back(c);
      ch = co; hh = ho; ww = wo;
    }
  pl.conv.resize(pl.shape.size());
  return pl;
}

// exact worst-case number of padded input rows a patch tile needs
inline int patch_rows(const ConvShape& c, int B, int BM, bool per_image) {
  const int HoWo = c.hout * c.wout, Hip = c.hin + 2;
  long M = (long)B * HoWo;
  int worst = 0;
  auto rows_of = [&](long m0, long mend) {
    const long ml = mend - 1;
    const long b0 = m0 / HoWo, ho0 = (m0 - b0 * HoWo) / c.wout;
    const long b1 = ml / HoWo, ho1 = (ml - b1 * HoWo) / c.wout;
    return (int)((b1 * Hip + ho1 * c.stride + 2) - (b0 * Hip + ho0 * c.stride) + 1);
  };
  if (per_image) {
    const int tpi = (HoWo + BM - 1) / BM;
    for (int t = 0; t < tpi; ++t) {
      const long m0 = (long)t * BM, mend = std::min<long>(m0 + BM, HoWo);
      worst = std::max(worst, rows_of(m0, mend));
    }
  } else {
    for (long m0 = 0; m0 < M; m0 += BM) worst = std::max(worst, rows_of(m0, std::min<long>(m0 + BM, M)));
  }
  return worst;
}

inline ConvPlan plan_conv(const PlanOptions& o, const ConvShape& c, int B) {
  ConvPlan pc;
  const int HoWo = c.hout * c.wout;
  const int Wip = c.win + 2;
  struct Cand { int cfg, patch, per_image, rows, nbuf; size_t lds; };
  std::vector<Cand> cands;
  const bool can_patch = o.patch && c.k == 3 && c.stride == 1;
  std::vector<int> cfgs;
  if (c.cout == 64) { if (o.bm256) cfgs.push_back(2); cfgs.push_back(0); }
  else cfgs.push_back(1);
  // a 3-deep ring pays where the weight tile is 16 KB per step (Cout >= 128); for the 64-channel layers
  // it would push the 256-pixel tile out of LDS and cost more than it hides
  std::vector<int> depths;
  if (o.nbuf == 3 && c.cout >= 128) depths.push_back(3);
  depths.push_back(2);
  // preference: deepest ring first, then patch before gather, flat tiles before per-image tiles
  for (int nb : depths)
    for (int cfg : cfgs) {
      int BM, BN; tile_dims(cfg, &BM, &BN);
      if (can_patch)
        for (int pi = 0; pi < 2; ++pi) {
          const int rows = patch_rows(c, B, BM, pi != 0);
          cands.push_back({cfg, 1, pi, rows, nb, (size_t)nb * BN * 128 + (((size_t)rows * Wip * 128 + 4095) & ~(size_t)4095)});
        }
    }
  for (int nb : depths)
    for (int cfg : cfgs) {
      int BM, BN; tile_dims(cfg, &BM, &BN);
      cands.push_back({cfg, 0, 0, 0, nb, (size_t)nb * BN * 128 + (size_t)nb * BM * 128});
    }
  // first candidate that lets two workgroups share a CU; else the smallest that fits at all
  const Cand* pick = nullptr;
  for (const Cand& cd : cands)
    if (cd.lds <= kLdsTwoBlocks) { pick = &cd; break; }
  if (!pick)
    for (const Cand& cd : cands)
      if (cd.lds <= kLdsMax && (!pick || cd.lds < pick->lds)) pick = &cd;
  int BM, BN; tile_dims(pick->cfg, &BM, &BN);
  pc.cfg = pick->cfg; pc.patch = pick->patch; pc.nbuf = pick->nbuf; pc.per_image = pick->per_image; pc.rows_max = pick->rows; pc.lds = pick->lds;
  pc.tiles_per_image = (HoWo + BM - 1) / BM;
  pc.ntiles = c.cout / BN;
  // second-generation kernel (conv_stag.hip): 256 x 128 tiles, 32-channel steps, double-buffered patch
  if (o.stag && c.k == 3 && c.stride == 1 && c.cin % 64 == 0 && (c.cout >= 128 || (c.cout == 64 && o.stag >= 2))) {
    const int sbm = c.cout == 64 ? 512 : 256, sbn = c.cout == 64 ? 64 : 128;
    const int rows = patch_rows(c, B, sbm, false);
    const long pieces = (long)rows * (Wip + (o.skew ? 2 : 0)) * 4;   // skew: LDS row pitch W + 4, conflict-free fragment reads across row wraps (conv_stag.hip)
    int P = (int)((pieces + 511) / 512);
    if (P < 2) P = 2;                                  // kernel instantiations: 2..6 and 8 DMA rounds per patch burst
    if (P < 4 && c.cout >= 128 && o.dsfuse) P = 4;     // 32 KB buffers: room for a folded shortcut's gathered pixel tiles
    if (P == 7) P = 8;                                 // (every round is 8 KB of L2 -> LDS traffic per half-chunk and tile)
    const size_t lds = (size_t)6 * sbn * 64 + (size_t)2 * P * 8192;   // 3 double tiles + 2 patch buffers
    if (P <= 8 && lds <= kLdsMax) { pc.stag = 1; pc.stag_patch_bytes = P; pc.stag_lds = lds; }
    if (c.cout >= 128)                                  // the 4-wave kernel's smaller tiles (conv_w4.hip, MT = 5..7)
      for (int mt = 5; mt <= 7; ++mt) {
        const long pcs = (long)patch_rows(c, B, 32 * mt, false) * (Wip + 2) * 4;
        const int Pm = std::max(4, (int)((pcs + 511) / 512));
        pc.w4_patch[mt] = (mt == 7 ? Pm <= 6 : Pm == 4) ? Pm : 0;      // below 7: the 4-round instantiations only
      }
    // layer-1 shape: 8-row bands of one image per tile (constant tile geometry, 7 bands per 56-row image)
    if (c.cout == 64 && o.stag >= 3 && c.hout % 8 == 0 && c.wout <= 64) {
      int Pr = (int)(((long)10 * Wip * 4 + 511) / 512);
      // odd Pr (3, 5) = the instantiations that keep the 72 KB weight panel of a 64 -> 64 layer resident in LDS
      if (c.cin == 64 && Pr <= 5) Pr = Pr <= 3 ? 3 : 5; else Pr = Pr <= 6 ? 6 : 8;
      const size_t ldsr = ((Pr & 1) ? (size_t)18 * 4096 : (size_t)6 * sbn * 64) + (size_t)2 * Pr * 8192;
      if (Pr <= 8 && ldsr <= kLdsMax) { pc.stag = 2; pc.stag_patch_bytes = Pr; pc.stag_lds = ldsr; }
    } else if (c.cout == 64 && o.stag >= 3 && o.rowseg && c.hout % 8 == 0 && c.wout > 64) {
      // wide maps (512 x 512 crops: layer 1 is 128 x 128): 8-row bands cut into 64-column segments, 10 x 66-pixel patches
      // (2640 pieces -> 6 DMA rounds), ring weights
      pc.stag = 2; pc.stag_patch_bytes = 6; pc.nseg = (c.wout + 63) / 64;
      pc.stag_lds = (size_t)6 * sbn * 64 + (size_t)2 * 6 * 8192;
    }
  }
  // 3x3 stride-2 convs: the gathered-tile variant of the same 8-wave structure (conv_gstag)
  if (o.stag && o.gstag && c.k == 3 && c.stride == 2 && c.cin % 64 == 0 && c.cin >= (o.gstag >= 2 ? 64 : 128) && c.cout % 128 == 0) pc.stag = 3;
  return pc;
}

inline void replan(Plan& pl, const PlanOptions& o) {
  for (size_t i = 0; i < pl.shape.size(); ++i) pl.conv[i] = plan_conv(o, pl.shape[i], pl.maxB);
  // fold each block's 1x1 stride-2 shortcut into the conv2 that consumes it when that conv2 runs on conv_stag 256x128
  // tiles with >= 32 KB patch buffers (one gathered 64-channel pixel tile pair fits one buffer)
  if (o.dsfuse && pl.dtype != FLOPE_DT_F32)
    for (size_t i = 0; i + 1 < pl.shape.size(); ++i) {
      const ConvShape& cd = pl.shape[i];
      const ConvShape& c2 = pl.shape[i + 1];
      const ConvPlan& p2 = pl.conv[i + 1];
      if (cd.k == 1 && c2.k == 3 && c2.res == 2 && p2.stag == 1 && c2.cout >= 128 && p2.stag_patch_bytes >= 4 &&
          p2.stag_patch_bytes != 7 && cd.cin % 64 == 0 && cd.stride == 2) {
        pl.conv[i].folded = 1;
        pl.conv[i + 1].ds_conv = (int)i;
      }
    }
}

// static part of the choice between conv_w4 (4 waves) and conv_stag for a flat 256 x 128 conv (decide() still sends split-K
// launches and variants that are not instantiated to conv_stag)
inline bool w4_eligible(const PlanOptions& o, const ConvShape& s, const ConvPlan& c) {
  return o.w4 && !o.persist && c.stag == 1 && s.cout >= 128 && o.skew && c.stag_patch_bytes >= 4 && c.stag_patch_bytes <= 6;
}

// ---- batch slices -------------------------------------------------------------------------------------------------------------------
struct Slices { int n = 1, plan_slices = 1; int start[4] = {0, 0, 0, 0}, count[4] = {0, 0, 0, 0}; };

// With the "streams" option (default 2) and a large enough batch the crops are split into slices that run the same launch
// sequence on their own streams.  plan_slices: the slices of the production schedule -- profile = 1 times every launch on ONE
// stream, but with the kernel variants (tile heights, class walk) the production schedule of this batch picks, so that the
// per-launch table describes the kernels the un-profiled step runs.
inline Slices slices(const PlanOptions& o, int batch, int profile) {
  Slices sl;
  int ns = o.streams >= 2 ? o.streams : 1;
  while (ns > 1 && batch / ns < 32) --ns;              // keep every slice large enough to fill the chip
  sl.plan_slices = ns;
  if (profile == 1) ns = 1;
  sl.n = ns;
  // slice boundaries on multiples of 8 images (whole tiles in every layer) when the batch allows it
  auto bound = [&](int k) { const int b_ = (int)((long)batch * k / ns); return (batch >= 16 * ns && k > 0 && k < ns) ? ((b_ + 4) & ~7) : b_; };
  for (int s = 0; s < ns; ++s) { sl.start[s] = bound(s); sl.count[s] = bound(s + 1) - sl.start[s]; }
  if (ns == 2) {
    // equal halves by default -- 128/128 beats 96/160 by 1 - 2.5 % in every autotune run (profiles/r04_autotune_runs.txt);
    // "split" overrides, and PoseEngine.autotune still tries 3/8 and 7/16 (multiples of 8 images, so every layer's tiles stay whole)
    int first = o.split > 100 ? o.split - 100 : (int)((long)batch * o.split / 100);
    if (o.split == 0) first = batch >= 128 ? (batch / 2) & ~7 : batch / 2;
    first = std::max(1, std::min(batch - 1, first));
    sl.start[0] = 0; sl.count[0] = first; sl.start[1] = first; sl.count[1] = batch - first;
  }
  return sl;
}

// what a decision may look at besides the options and the plan
struct SliceCtx { int batch = 1, whole_batch = 1, slice = 0, slices = 1, plan_slices = 1, num_cus = 256; };

inline SliceCtx slice_ctx(const Slices& sl, int s, int whole_batch, int num_cus) {
  SliceCtx x;
  x.batch = sl.count[s]; x.whole_batch = whole_batch; x.slice = s; x.slices = sl.n; x.plan_slices = sl.plan_slices; x.num_cus = num_cus;
  return x;
}

// ---- the decision for one conv of one slice ---------------------------------------------------------------------------------------
enum Family { kFolded, kNaive, kGstag, kS1r, kR4, kW4, kStagFlat, kStag512x64, kStagBands, kS2r, kMfma, kF32m };   // kFolded: no launch of its own

struct Launch {
  int family = kFolded;
  // ConvP's tiling fields as the launched kernel reads them
  int mtiles = 0, ntiles = 0, tiles_per_image = 0, per_image = 0, nseg = 0;
  int patch_rounds = 0;          // ConvP::patch_rows_max: patch DMA rounds (conv_stag lineage), padded patch rows (conv_mfma)
  int total_tiles = 0;           // tiles the grid walks: mtiles * ntiles; 4-row bands of conv_s1r / conv_s2r
  int grid = 0;                  // workgroups of the (main) launch
  size_t lds_bytes = 0;
  int mt = 0, cw_imgs = 0, walk_groups = 0;   // conv_w4: pixel tiles per wave; class walk: images per walk step, workgroups per channel tile (0: one tile per workgroup)
  int ksplit = 1;                // > 1: split-K main launch + finalize launch (which owns bias / residual / ReLU)
  int res_lds = 0, skew = 0, prio = 0;
  int shortcut_folded = 0;       // the block's 1x1 stride-2 shortcut is computed inside this launch
  int cfg = 0, patch = 0, nbuf = 0;           // conv_mfma
  int dbg = 0, dbg_lds_off = 0;  // ConvP::dbg / dbg_lds_off
  int stamps = 0;                // diagnostic builds: the launch leaves clock stamps in its region of the split-K workspace
};

// conv_f32m (float32 on the exact-fp32 MFMA): a wave owns mp x 16 pixels x 64 channels, a workgroup four consecutive pixel tiles
// of one 64-channel block, and a CU holds ONE workgroup (kF32mLds; measured).  So a launch takes whole rounds of
// `cus` workgroups, and a workgroup's time grows with mp: the cheapest of mp = 4 / 2 / 1 by rounds x (4 mp + 1) -- the + 1 stands
// for a workgroup's prologue and epilogue, an estimate of a quarter of one pixel tile's K loop -- ties to the larger tile (fewer
// weight loads per MFMA).  (Every output is summed in the same order whatever mp is.)
inline int f32m_mp(int M, int cout, int cus) {
  int best = 4;
  long best_cost = -1;
  for (int mp = 4; mp >= 1; mp >>= 1) {
    const long wgs = (long)((M + 64 * mp - 1) / (64 * mp)) * (cout / 64);
    const long cost = (wgs + cus - 1) / cus * (4 * mp + 1);
    if (best_cost < 0 || cost < best_cost) { best_cost = cost; best = mp; }
  }
  return best;
}
inline void f32m_launch(Launch& L, int M, int cout, int cus) {
  L = Launch();
  L.family = kF32m; L.mt = f32m_mp(M, cout, cus); L.lds_bytes = kF32mLds;
  L.mtiles = (M + 64 * L.mt - 1) / (64 * L.mt); L.ntiles = cout / 64;
  L.total_tiles = L.grid = L.mtiles * L.ntiles;
}

// ---- split-K of conv_f32m (option f32m_ksplit) ----
// A conv_f32m workgroup walks all n = K / 16 steps of its tile alone, so at small batches a launch is a few workgroups that each
// run 36 .. 288 serial steps on an otherwise idle chip.  A split launch gives every tile S workgroups; workgroup `share` walks the
// steps [f32m_share_begin(n, S, share), f32m_share_begin(n, S, share + 1)) from +0 and stores raw partial sums, and a second,
// ordered launch (conv_f32m_finalize_kernel) adds bias + share 0 + share 1 + ... in that order, the residual, ReLU.
// THE partition formula: the engine, the kernel's host-side guard and the host walk of tests/host_harness all use this one.
constexpr int f32m_share_begin(int nsteps, int S, int share) { return (int)((long)share * nsteps / S); }
constexpr int kF32mMinShareSteps = 4;        // every share walks at least this many steps (the 4-step 1x1 shortcut of layer 2 never splits)
constexpr int kF32mMaxSplit = 32;
// the partial sums of one split launch: at most one round of the chip (total_tiles * S <= cus) of the largest tile (256 pixels x
// 64 channels), 16 MiB at 256 CUs -- S * M * Cout <= total_tiles * S * (64 mp) * 64 fits by that rule
inline size_t f32m_ws_bytes(int cus) { return (size_t)cus * 256 * 64 * sizeof(float); }
// Cost model of option value 1, in shader-clock cycles at the 2.4 GHz maximum clock: a share's serial K loop + the finalize launch
// where S > 1, fitted to the per-launch table of tools/bench_f32m_ksplit.py --per-launch (profiles/f32m_ksplit_per_launch.txt,
// DESIGN.md 17; one MI355X, profile = 1, B = 1 x 224^2, MP = 1):
//   kF32mStepCycles = 655 per pixel tile of the wave: unsplit launches of n = 36 / 72 / 144 / 288 steps take 15.5 / 25.5 / 45 / 84.6 us
//     = 6 us (what a 4-step launch costs as well) + 0.273 us per step -- 1.28 x the 512 cycles of 16 back-to-back MFMAs
//   finalize = kF32mFinalizeCycles + S kF32mFinalizeShareCycles = 4300 + 720 S (1.8 us + 0.3 us per share): what a split launch of
//     S = 2 / 4 / 8 / 16 / 32 shares of layer 4 (n = 288) takes beyond 6 us + 0.273 us ceil(n / S): 2.5 / 3.2 / 4.1 / 6.3 / 11.1 us;
//     layer 3 (n = 144) gives 2.2 / 3.0 / 4.4 / 7.1.  The per-share term (finalize reads S partial sums per output, one after the
//     other) is why x32 measured SLOWER than x16 there; the first, derived model (512 cycles, one 4 us launch) picked x32.
constexpr long kF32mStepCycles = 655, kF32mFinalizeCycles = 4300, kF32mFinalizeShareCycles = 720;
// S for a conv_f32m launch of total_tiles workgroups of mp pixel tiles per wave and nsteps K steps; option as PlanOptions::f32m_ksplit.
// A split is allowed when (a) the batch runs in one slice (one workspace per engine), (b) total_tiles * S <= cus (at most one
// round) and (c) every share has >= kF32mMinShareSteps steps.  Returns 1 where none is allowed or none pays.
inline int f32m_ksplit(int option, int total_tiles, int mp, int nsteps, int plan_slices, int cus) {
  if (option <= 0 || plan_slices != 1) return 1;
  int best = 1;
  long best_cost = (long)nsteps * kF32mStepCycles * mp;
  for (int S = 2; S <= kF32mMaxSplit; S *= 2) {
    if ((long)total_tiles * S > cus || nsteps / S < kF32mMinShareSteps) break;
    if (option >= 2) { if (S <= option) best = S; continue; }
    const long cost = (long)((nsteps + S - 1) / S) * kF32mStepCycles * mp + kF32mFinalizeCycles + S * kF32mFinalizeShareCycles;
    if (cost < best_cost) { best_cost = cost; best = S; }
  }
  return best;
}

inline Launch f32m_stem_launch(const Plan& pl, const SliceCtx& x) {
  Launch L;
  f32m_launch(L, x.batch * pl.Hs * pl.Ws, 64, x.num_cus);
  return L;
}

inline ConvDims conv_dims(const Plan& pl, int i) {
  const ConvShape& s = pl.shape[i];
  const int dsi = pl.conv[i].ds_conv;
  ConvDims d = {s.stride, s.k == 3 ? 9 : 1, s.cin, s.cout, s.hout, s.wout, s.hin + 2, s.win + 2, 0, s.res != 0 && dsi < 0, dsi >= 0, false, 0, 0, 0};
  if (dsi >= 0) { const ConvShape& cd = pl.shape[dsi]; d.ds_Cin = cd.cin; d.ds_Hip = cd.hin + 2; d.ds_Wip = cd.win + 2; }
  return d;
}

inline Launch decide(const PlanOptions& o, const Plan& pl, int i, const SliceCtx& x) {
  const ConvShape& s = pl.shape[i];
  const ConvPlan& c = pl.conv[i];
  const int batch = x.batch, M = batch * s.hout * s.wout, cus = x.num_cus;
  Launch L;
  if (c.folded) return L;                            // computed inside the next launch (conv_stag DSF)
  int BM, BN; tile_dims(c.cfg, &BM, &BN);
  L.per_image = c.per_image; L.tiles_per_image = c.tiles_per_image;
  L.mtiles = c.per_image ? batch * c.tiles_per_image : (M + BM - 1) / BM;
  L.ntiles = c.ntiles; L.patch_rounds = c.rows_max; L.dbg = o.dbg;
  L.total_tiles = L.grid = L.mtiles * L.ntiles;
  L.cfg = c.cfg; L.patch = c.patch; L.nbuf = c.nbuf;
  if (pl.dtype == FLOPE_DT_F32 && o.f32mfma) {
    f32m_launch(L, M, s.cout, cus);
    if (o.f32m_ksplit) {                             // (the stem, 13 steps, has its own launch and is never split)
      L.ksplit = f32m_ksplit(o.f32m_ksplit, L.total_tiles, L.mt, s.k * s.k * s.cin / 16, x.plan_slices, cus);
      L.grid = L.total_tiles * L.ksplit;
    }
    return L;
  }
  if (pl.dtype == FLOPE_DT_F32) { L.family = kNaive; return L; }
  ConvDims d = conv_dims(pl, i);
  if (c.stag == 3) {
    L.family = kGstag; L.per_image = 0; L.mtiles = (M + 255) / 256; L.ntiles = s.cout / 128;
    L.total_tiles = L.grid = L.mtiles * L.ntiles; L.lds_bytes = kGstagLds;
    return L;
  }
  if (!c.stag) {
    if (o.s2r && has_s2r_image(s) && s2r_ok(d)) {      // patch in LDS, weights through registers (conv_s2r.hip)
      L.family = kS2r; L.total_tiles = batch * (s.hout >> 2);
      L.grid = std::min(o.s2r_grid > 0 ? o.s2r_grid : cus, L.total_tiles); L.lds_bytes = kS2rLds; L.stamps = (o.dbg & 64) != 0;
      return L;
    }
    L.family = kMfma; L.lds_bytes = c.lds + (size_t)o.ldspad * 1024;
    return L;
  }
  // conv_stag lineage: flat 256 x 128 (512 x 64) tiles or 8-row bands
  const int sbm = s.cout == 64 ? 512 : 256;
  L.per_image = 0; L.mtiles = (M + sbm - 1) / sbm; L.ntiles = s.cout == 64 ? 1 : s.cout / 128; L.patch_rounds = c.stag_patch_bytes;
  L.total_tiles = L.mtiles * L.ntiles;
  L.skew = o.skew; L.prio = o.prio; L.shortcut_folded = c.ds_conv >= 0;
  // weights in registers, K split over wave pairs (conv_s1r.hip)
  if (o.s1r && has_s1r_image(s) && c.stag == 1 && (c.ds_conv < 0 || has_ds_s1r_image(pl.shape[c.ds_conv]))) {
    d.ds_w = c.ds_conv >= 0;
    if (s1r_ok(d)) {
      L.family = kS1r; L.total_tiles = batch * (s.hout >> 2); L.grid = std::min(cus, L.total_tiles); L.lds_bytes = kS1rLds;
      L.stamps = (o.dbg & 64) != 0;
      return L;
    }
  }
  if (c.stag == 2) { L.per_image = 2; L.nseg = c.nseg; L.tiles_per_image = s.hout / 8 * c.nseg; L.mtiles = batch * L.tiles_per_image; L.total_tiles = L.mtiles; }
  // persistent grid: one workgroup per CU (a multiple of ntiles so a workgroup keeps its channel tile); the
  // row-band kernel is always persistent and shares the CUs with the other batch slices in flight
  const int share = std::max(1, (int)((long)cus * batch / std::max(1, x.whole_batch)));
  int gridb = (o.persist && c.ds_conv < 0) ? std::min(L.total_tiles, share) : L.total_tiles;
  if (c.stag == 2)    // one workgroup per CU: two whole-chip grids interleave more evenly than grids sized to the slice's share of
    // the CUs: +0.7 .. +2.5 % on the two-slice step in un-profiled same-run pairs, DESIGN.md 9.7c.  rows_grid = -1 restores the
    // share, > 0 sets the grid.
    gridb = std::min(L.total_tiles, o.rows_grid > 0 ? o.rows_grid : o.rows_grid < 0 ? share : cus);
  gridb -= gridb % L.ntiles;
  if (gridb < L.ntiles) gridb = L.ntiles;
  L.grid = gridb;
  // layer 1 (64 -> 64 on the 56-wide map) on the 4-wave row-band kernel (conv_r4.hip)
  if (c.stag == 2 && o.r4 && c.nseg <= 1 && !(o.dbg & 128) && r4_ok(d)) {
    L.family = kR4; L.lds_bytes = kR4Lds; L.stamps = (o.dbg & 64) != 0;
    return L;
  }
  // split-K for small batches: with fewer tiles than half the CUs a tile's serial K loop (up to 72 double steps) is the
  // layer's latency; give every tile ksplit workgroups, each a share of the input channels.  A split pays its fp32
  // partial sums (128 KB per workgroup, written and read back) and a finalize launch, so the factor is chosen by a small
  // cost model fitted to B = 16 / 31 @ 512^2 (layer 3, 128 tiles, x2: 40 vs 37 us -- a loss; layer 4, 124 tiles, x2: a win;
  // layer 4, 64 tiles, x4: 37 vs 55 us): gain = T (1 - 1/s) - (5 us + 0.066 us * tiles * s), T = 0.75 us per double step.
  int ksp = 1;
  if (o.ksplit && c.stag == 1 && x.plan_slices == 1 && !o.persist && L.total_tiles * 2 <= cus) {
    const int bodies = s.cin / 64;
    const double T = 0.75 * 9.0 * bodies;
    double best = 0.0;
    for (int sp = 2; sp <= bodies && bodies % sp == 0 && L.total_tiles * sp <= cus; sp *= 2) {
      const double gain = o.ksplit == 2 ? sp : T * (1.0 - 1.0 / sp) - (5.0 + 0.066 * L.total_tiles * sp);
      if (gain > best) { best = gain; ksp = sp; }
    }
  }
  if (ksp > 1) gridb = L.total_tiles * ksp;
  const bool one_tile_each = ksp == 1 && gridb == L.total_tiles;
  L.stamps = (o.dbg & (64 | 128)) && ksp == 1;
  // flat 256 x 128 tiles, no split-K -> the 4-wave kernel (conv_w4.hip)
  if (w4_eligible(o, s, c) && one_tile_each && !(o.dbg & 128)) {
    // workgroup tiles of 256 .. 160 pixels (8 .. 5 pixel tiles per wave; one tile per workgroup): the cheapest by whole rounds
    // of the chip x the time of a tile -- ~15 k cycles of prologue + epilogue, and per double step 128 cycles of MFMAs per
    // pixel tile + ~500 of everything else (clock stamps: 1.52 k at 8, 1.4 k at 7); ties go to the larger tile
    const int dsf = c.ds_conv >= 0 ? 1 : 0;
    int mt = 8;
    if (o.w4mt != 8) {
      const double dsteps = 9.0 * (s.cin / 64 + dsf);
      // Measured (profiles/r03_conv_w4_tile_height_ab.txt): with two batch slices in flight only 224 against 256 pays (+1.8 % on
      // the step; letting the choice go down to 128 or sizing it to the slice's share of the CUs loses 2 - 5 %: the other slice's
      // launches fill what a coarse tiling leaves idle).  A launch that has the chip to itself (one slice: batches below 64, the
      // profile pass) gains another ~12 % from 192 / 160-pixel tiles where they save a round.
      const int mt_lo = o.w4mtlo ? o.w4mtlo : (x.plan_slices == 1 ? 5 : 7);
      auto cost = [&](int m) {
        const int t = (M + 32 * m - 1) / (32 * m) * L.ntiles;
        return (double)((t + cus - 1) / cus) * (15000.0 + dsteps * (128.0 * m + 500.0));
      };
      double best = o.w4mt ? 1e30 : cost(8);
      for (int m = 7; m >= mt_lo; --m) {
        if (!c.w4_patch[m] || (o.w4mt && o.w4mt != m)) continue;
        const double cm = cost(m);
        if (cm < best) { best = cm; mt = m; }
      }
    }
    // class walk (option w4cw = tiles per workgroup aimed at): 224-pixel tiles, every tile whole, a walk step of G tiles = whole
    // images (G a multiple of the tiling's period lcm(Ho Wo, 224) / 224), G | mtiles.  The largest k <= w4cw that allows it.
    // Measured at B = 256 (profiles/r04_conv_w4_class_walk_ab.txt): one slice -2.3 % per step (layer 2 at 4 tiles per workgroup
    // -14 %, layer 3 at 2 tiles -5 %); with two slices in flight +0.5 % -- 896 tiles of 224 pixels are 3.5 per CU, equal walks
    // leave 32 CUs idle where the one-tile-per-workgroup launches of the two slices fill each other's gaps.  So: where a launch
    // has the chip to itself (option w4cwf overrides).
    int gw = 0, cw_imgs = 0;
    if (o.w4cw >= 2 && (x.plan_slices == 1 || (o.w4cwf & 1)) && (o.w4mt == 0 || o.w4mt == 7) && c.w4_patch[7] && M % 224 == 0 &&
        w4_lds(c.w4_patch[7], 7, dsf, 1) != 0) {
      const long hw = (long)s.hout * s.wout;
      long a_ = hw, b_ = 224; while (b_) { const long t_ = a_ % b_; a_ = b_; b_ = t_; }   // gcd
      const int period = (int)(hw / a_), mt7 = M / 224;
      // ... and that still fills this slice's share of the CUs (a walk of 112 workgroups on 256 CUs loses more than the tile
      // boundaries it saves: profiles/r04_conv_w4_class_walk_layers.txt)
      for (int k = std::min(o.w4cw, mt7); k >= 2 && !gw; --k)
        if (mt7 % k == 0 && (mt7 / k) % period == 0 && ((o.w4cwf & 2) || (long)(mt7 / k) * L.ntiles * 100 >= (long)share * 85)) { gw = mt7 / k; cw_imgs = (int)((long)gw * 224 / hw); }
      if (gw) mt = 7;
    }
    const int pt = mt != 8 ? c.w4_patch[mt] : c.stag_patch_bytes;
    const size_t lds = w4_lds(pt, mt, dsf, gw ? 1 : 0);
    if (lds != 0) {                                  // (a variant that is not instantiated stays on conv_stag's flat tiles)
      L.family = kW4; L.mt = mt; L.walk_groups = gw; L.cw_imgs = gw ? cw_imgs : 0; L.lds_bytes = lds;
      if (mt != 8) { L.mtiles = (M + 32 * mt - 1) / (32 * mt); L.total_tiles = L.mtiles * L.ntiles; L.patch_rounds = pt; }
      L.grid = gw ? gw * L.ntiles : L.total_tiles;
      L.res_lds = (o.reslds && d.res && s.cout >= 128 && c.stag_patch_bytes >= 4) ? 1 : 0;
      return L;
    }
  }
  L.family = c.stag == 2 ? kStagBands : (s.cout == 64 ? kStag512x64 : kStagFlat);
  L.ksplit = ksp; L.grid = gridb;
  L.res_lds = (o.reslds && d.res && c.stag == 1 && s.cout >= 128 && c.stag_patch_bytes >= 4 && one_tile_each) ? 1 : 0;
  L.lds_bytes = c.stag_lds;
  if ((o.dbg & 128) && L.lds_bytes + 2048 <= kLdsMax) { L.dbg_lds_off = (int)L.lds_bytes; L.lds_bytes += 2048; }
  else if (o.dbg & 128) L.dbg &= ~128;
  return L;
}

inline std::vector<Launch> decide_all(const PlanOptions& o, const Plan& pl, const SliceCtx& x) {
  std::vector<Launch> v;
  for (size_t i = 0; i < pl.shape.size(); ++i) v.push_back(decide(o, pl, (int)i, x));
  return v;
}

// ---- names ------------------------------------------------------------------------------------------------------------------------
inline std::string label(const Launch& L) {
  switch (L.family) {
    case kNaive: return "naive_conv_kernel";
    case kGstag: return "conv_gstag_kernel<256x128,s2>";
    case kS1r: return "conv_s1r_kernel<4rows x28>";
    case kR4: return "conv_r4_kernel<8rows x56>";
    case kW4: return "conv_w4_kernel<256x128>";
    case kStagFlat: return "conv_stag_kernel<256x128>";
    case kStag512x64: return "conv_stag_kernel<512x64>";
    case kStagBands: return "conv_stag_kernel<8rows x64>";
    case kS2r: return "conv_s2r_kernel<4rows x28>";
    case kF32m: {
      char k[64];
      snprintf(k, sizeof k, "conv_f32m_kernel<%dx64>", 64 * L.mt);
      return k;
    }
    case kMfma: {
      int BM, BN; tile_dims(L.cfg, &BM, &BN);
      char k[96];
      snprintf(k, sizeof k, "conv_mfma_kernel<%dx%d,%s,ring%d>", BM, BN, L.patch ? "patch" : "gather", L.nbuf);
      return k;
    }
  }
  return "";
}

inline std::string detail(const Launch& L) {
  char d[96] = "";
  if (L.family == kS1r && L.shortcut_folded) return "[shortcut folded in]";
  if (L.family == kW4 && L.walk_groups) snprintf(d, sizeof d, "[%d px tiles, walk: %d workgroups x %d tiles]", 32 * L.mt, L.grid, L.mtiles / L.walk_groups);
  else if (L.family == kW4) snprintf(d, sizeof d, "[%d px tiles]", 32 * L.mt);
  else if (L.ksplit > 1) snprintf(d, sizeof d, "[split-K x%d]", L.ksplit);
  return d;
}

inline int head_launches(const Plan& pl, const PlanOptions& o) { return (o.fuse_stem && pl.dtype != FLOPE_DT_F32) ? 1 : 3; }   // front of the trunk: input + stem + maxpool
inline int tail_launches() { return 3; }                                                                                        // avgpool, fc.0, fc_rot + Procrustes
inline int forward_launches(const Plan& pl, const PlanOptions& o) {
  int n = (int)pl.conv.size() + tail_launches() + head_launches(pl, o);
  for (const ConvPlan& c : pl.conv) n -= c.folded;
  return n;
}

// ---- the regression head behind layer4.1 (pool_head.hip): which kernel fc.0 and fc_rot run on ------------------------------------
// The ONE statement of that choice: the launchers of pool_head.hip ask these functions, flope_head_plan reports them, and
// tests/test_host.py pins them over the widths tests/test_gpu_head.py runs.  (launch_name below labels the head "fc1_kernel" /
// "fc2_procrustes_kernel" whatever ran: tests/golden/plan_matrix.json pins those labels.)
enum HeadFc1 { kFc1Packed = 0, kFc1RowMajor = 1, kFc1Simple = 2 };           // fc1_packed_kernel<1>, fc1_kernel, fc1_simple_kernel
enum HeadFc2 { kFc2K4 = 0, kFc2WaveVector = 1, kFc2WaveScalar = 2 };         // fc2_procrustes_k4_kernel, fc2_procrustes_kernel<vector / scalar K loop>
constexpr int kHeadK = 512;                                                  // layer4.1's channels: K of fc.0

// fc.0 [N, K]: the MFMA kernels walk K in blocks of 32 and N in tiles of 16; the packed one also stages 16 feature rows of
// K + 4 floats in LDS (inside the default 64 KiB dynamic-LDS limit) and needs the fragment-order image of the weights
inline int head_fc1_variant(bool have_packed, int K, int N) {
  const bool mfma = K % 32 == 0 && N % 16 == 0;
  if (mfma && have_packed && (size_t)16 * (K + 4) * sizeof(float) <= 64 * 1024) return kFc1Packed;
  return mfma ? kFc1RowMajor : kFc1Simple;
}
// fc_rot [9, K]: four waves per image take K / 4 each in steps of 256; else one wave per image, 16-byte loads where K allows
inline int head_fc2_variant(bool k4, int K) {
  if (k4 && K % 1024 == 0) return kFc2K4;
  return K % 4 == 0 ? kFc2WaveVector : kFc2WaveScalar;
}
struct HeadPlan { int fc1, fc2; };
// (the engine uploads the packed image whenever bod % 16 == 0, which the packed kernel needs anyway)
inline HeadPlan head_plan(const PlanOptions& o, int bod) {
  return {head_fc1_variant(o.fc1_packed != 0 && bod % 16 == 0, kHeadK, bod), head_fc2_variant(o.fc2_k4 != 0, bod)};
}

// launch idx of a forward whose convs launch L[conv]: "layer|kernel", the conv behind it (-1: none) and its FLOPs per crop;
// empty for a bad index
inline std::string launch_name(const Plan& pl, const PlanOptions& o, const std::vector<Launch>& L, int bod, int idx, int* conv, double* flops) {
  std::vector<int> live;                             // convs that are launched (folded shortcuts are not)
  for (size_t i = 0; i < pl.conv.size(); ++i) if (!pl.conv[i].folded) live.push_back((int)i);
  const int nc = (int)live.size(), nh = head_launches(pl, o);
  *conv = -1; *flops = 0.0;
  if (idx < 0 || idx >= nc + tail_launches() + nh) return "";
  const double stem_flops = 2.0 * pl.Hs * pl.Ws * 64 * 147;
  if (nh == 1 && idx == 0) { *flops = stem_flops; return "input+stem+maxpool|stem_pool_kernel"; }
  if (nh == 3 && idx == 0) return "prep_input|prep_input_kernel";
  if (nh == 3 && idx == 1) {
    *flops = stem_flops;
    if (pl.dtype == FLOPE_DT_F32 && o.f32mfma) return "stem|conv_f32m_kernel<7x7,4ch>";
    return pl.dtype == FLOPE_DT_F32 ? "stem|naive_conv_kernel" : "stem|stem_mfma_kernel";
  }
  if (nh == 3 && idx == 2) return "maxpool|maxpool_kernel";
  idx -= nh;
  if (idx == nc) return "avgpool|avgpool_kernel";
  if (idx == nc + 1) { *flops = 2.0 * 512 * bod; return "fc1|fc1_kernel"; }
  if (idx == nc + 2) { *flops = 2.0 * 9 * bod; return "fc_rot+procrustes|fc2_procrustes_kernel"; }
  const int ci = live[idx];
  const ConvShape& s = pl.shape[ci];
  *conv = ci;
  *flops = 2.0 * s.hout * s.wout * s.cout * s.cin * s.k * s.k;
  std::string layer = conv_name(s);
  if (pl.conv[ci].ds_conv >= 0) {
    const ConvShape& cd = pl.shape[pl.conv[ci].ds_conv];
    layer += "+shortcut";
    *flops += 2.0 * cd.hout * cd.wout * cd.cout * cd.cin;
  }
  return layer + detail(L[ci]) + "|" + label(L[ci]);
}

// plan introspection for DESIGN.md / tests: one line per conv
inline std::string describe(const Plan& pl, const PlanOptions& o) {
  std::string out;
  char line[256];
  snprintf(line, sizeof line, "stem: tiles/img=%d rows=%d lds=%zu\n", pl.stem_tiles, pl.stem_rows, pl.stem_lds);
  out += line;
  for (size_t i = 0; i < pl.shape.size(); ++i) {
    const ConvShape& s = pl.shape[i];
    const ConvPlan& c = pl.conv[i];
    const std::string name = conv_name(s);
    const char* n = name.c_str();
    const bool w4 = w4_eligible(o, s, c);
    if (c.stag == 3) snprintf(line, sizeof line, "%s: 3x3 s2 %d->%d out %dx%d conv_gstag 256x128 (gathered tiles) lds=%zu\n", n, s.cin, s.cout, s.hout, s.wout, kGstagLds);
    else if (c.folded) snprintf(line, sizeof line, "%s: 1x1 s2 %d->%d out %dx%d folded into the next conv (conv_stag DSF)\n", n, s.cin, s.cout, s.hout, s.wout);
    else if (c.stag && c.ds_conv >= 0) snprintf(line, sizeof line, "%s: 3x3 s1 %d->%d out %dx%d %s 256x128 patch_rounds=%d lds=%zu, shortcut folded in (+%d K)\n", n, s.cin, s.cout, s.hout, s.wout, w4 ? "conv_w4" : "conv_stag", c.stag_patch_bytes, c.stag_lds, pl.shape[c.ds_conv].cin);
    else if (c.stag == 2 && c.nseg > 1) snprintf(line, sizeof line, "%s: 3x3 s1 %d->%d out %dx%d conv_stag 8-row bands x %d column segments of 64 patch_rounds=%d lds=%zu\n", n, s.cin, s.cout, s.hout, s.wout, c.nseg, c.stag_patch_bytes, c.stag_lds);
    else if (c.stag == 1 && w4) snprintf(line, sizeof line, "%s: 3x3 s1 %d->%d out %dx%d conv_w4 256x128 patch_rounds=%d lds=%zu\n", n, s.cin, s.cout, s.hout, s.wout, c.stag_patch_bytes, w4_lds(c.stag_patch_bytes, 8, 0, 0));
    else if (c.stag) snprintf(line, sizeof line, c.stag == 2 ? "%s: 3x3 s1 %d->%d out %dx%d conv_stag 8-row bands x 64 patch_rounds=%d lds=%zu\n" : "%s: 3x3 s1 %d->%d out %dx%d conv_stag 256x128 patch_rounds=%d lds=%zu\n", n, s.cin, s.cout, s.hout, s.wout, c.stag_patch_bytes, c.stag_lds);
    else snprintf(line, sizeof line, "%s: %dx%d s%d %d->%d out %dx%d cfg=%d patch=%d ring=%d per_image=%d rows=%d lds=%zu\n", n,
                  s.k, s.k, s.stride, s.cin, s.cout, s.hout, s.wout, c.cfg, c.patch, c.nbuf, c.per_image, c.rows_max, c.lds);
    out += line;
  }
  return out;
}

}  // namespace flope_plan
