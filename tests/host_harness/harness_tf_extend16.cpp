// CPU-only test harness of option extend_mfma's planner (flope_amd/csrc/tf_encoder_stream.h): the eligibility rule, the
// 64-key blocks a workgroup of tf_attn16_extend loads, the 32-key steps a wave takes at an unaligned first query, where the LDS row of
// a key comes from, the output row of a query, the launch, and the checks of flope_tf_stream_attention_extend.
// tests/test_tf_extend_mfma_host.py holds them against brute force without a GPU and runs tfx_selfcheck once in a stand-alone program
// built with -DTF_EXTEND16_MAIN under AddressSanitizer + UBSan.  Not part of the product.
#include "tf_encoder_stream.h"

#include <algorithm>
#include <vector>

extern "C" {

int tfx_ok(int dtype, int head_dim, int model_dim) { return flope_tf_plan::tf_extend_mfma_ok(dtype, head_dim, model_dim) ? 1 : 0; }
int tfx_positions_ok(int pos0, int len) { return flope_tf_plan::tf_extend_mfma_positions_ok(pos0, len) ? 1 : 0; }
int tfx_pos_max() { return flope_tf_plan::kTfExtendMfmaPosMax; }
int tfx_block_live(int len, int y) { return flope_tf_plan::tf_extend_mfma_block_live(len, y) ? 1 : 0; }
int tfx_lo(int pos0, int y, int W) { return flope_tf_plan::tf_extend_mfma_lo(pos0, y, W); }
int tfx_first_block(int pos0, int y, int W) { return flope_tf_plan::tf_extend_mfma_first_block(pos0, y, W); }
int tfx_last_block(int pos0, int len, int y) { return flope_tf_plan::tf_extend_mfma_last_block(pos0, len, y); }
int tfx_q0(int pos0, int y, int wave) { return flope_tf_plan::tf_extend_mfma_q0(pos0, y, wave); }
int tfx_step_taken(int q0, int kb, int Labs, int W) { return flope_tf_plan::tf_extend_mfma_step_taken(q0, kb, Labs, W) ? 1 : 0; }
long long tfx_out_row(int off_b, int pos0, int qi) { return flope_tf_plan::tf_extend_mfma_out_row(off_b, pos0, qi); }
// the 64 keys of block t for workgroup y: kinds and rows
void tfx_block_keys(int t, int pos0, int len, int capacity, int W, int y, int* kinds, int* rows) {
  for (int r = 0; r < flope_tf_plan::kTfAttnTiledKB; ++r) {
    const flope_tf_plan::TfExtendKey k = flope_tf_plan::tf_extend_mfma_key(t * flope_tf_plan::kTfAttnTiledKB + r, pos0, len, capacity, W, y);
    kinds[r] = k.kind; rows[r] = k.row;
  }
}
// out: grid_x, grid_y, block, lds
void tfx_launch(int n, int H, int max_len, int head_dim, long long* out) {
  const flope_tf_plan::TfExtendLaunch l = flope_tf_plan::tf_extend_mfma_launch(n, H, max_len, head_dim);
  out[0] = l.grid_x; out[1] = l.grid_y; out[2] = l.block; out[3] = (long long)l.lds;
}
// flope_tf_stream_attention_extend's check; out: bad, smax, max_len, total (-1 where untouched)
int tfx_check_hook(int tracks, int capacity, int window, int max_tokens, int n, int seq_len, const int* lengths, const int* cached, int* out) {
  out[0] = out[1] = out[2] = out[3] = -1;
  return flope_tf_plan::tf_stream_check_attention_extend(tracks, capacity, window, max_tokens, n, seq_len, lengths, cached, &out[0], &out[1], &out[2], &out[3]);
}

// One chunk (pos0, len) of a track with a linear cache (W = 0) or a ring, walked as the kernel walks it: 0, or a code naming the first
// property that failed.
//   1  a live query block has no blocks, or a dead one is called live
//   2  a visible key of a chunk query lies in no block its workgroup loads, or in a step its wave does not take
//   3  a visible key's source is not its rule: chunk row j - pos0 for j >= pos0, otherwise the cache row that HOLDS key j before the call
//   4  a key of a loaded block outside [lo_wg, Labs) is not a zero row, or one inside is
//   5  a cache or chunk row outside the cache / the chunk
//   6  a query's output row is not off + its chunk row
int tfx_walk(int pos0, int len, int capacity, int W) {
  using namespace flope_tf_plan;
  std::vector<long long> held((size_t)capacity, -1);       // the pre-call cache: row -> the key it holds
  for (int j = W ? std::max(0, pos0 - capacity) : 0; j < (W ? pos0 : std::min(pos0, capacity)); ++j) held[(size_t)(j % capacity)] = j;
  const int Labs = pos0 + len, off_b = 1000;
  const int ny = (len + 127) / 128;
  if (tf_extend_mfma_block_live(len, ny) || tf_extend_mfma_block_live(len, -1)) return 1;
  for (int y = 0; y < ny; ++y) {
    if (!tf_extend_mfma_block_live(len, y)) return 1;
    const int lo_wg = tf_extend_mfma_lo(pos0, y, W), t0 = tf_extend_mfma_first_block(pos0, y, W), t1 = tf_extend_mfma_last_block(pos0, len, y);
    if (t0 > t1 || t0 < 0) return 1;
    for (int t = t0; t <= t1 + 1; ++t)                     // (t1 + 1: the block the loop loads behind the last one)
      for (int r = 0; r < 64; ++r) {
        const int j = t * 64 + r;
        const TfExtendKey k = tf_extend_mfma_key(j, pos0, len, capacity, W, y);
        const bool inside = j >= lo_wg && j < Labs;
        if (inside != (k.kind != kTfExtendKeyZero)) return 4;
        if (k.kind == kTfExtendKeyCache && (k.row < 0 || k.row >= capacity)) return 5;
        if (k.kind == kTfExtendKeyChunk && (k.row < 0 || k.row >= len)) return 5;
      }
    for (int wave = 0; wave < 4; ++wave) {
      const int q0 = tf_extend_mfma_q0(pos0, y, wave);
      for (int qq = 0; qq < 32; ++qq) {
        const int i = 128 * y + 32 * wave + qq, p = pos0 + i;
        if (i >= len) break;
        if (p != q0 + qq) return 6;
        if (tf_extend_mfma_out_row(off_b, pos0, p) != off_b + i) return 6;
        for (int j = tf_window_lo(p, W); j <= p; ++j) {
          const int t = j / 64, kb = j & ~31;
          if (t < t0 || t > t1) return 2;
          if (!tf_extend_mfma_step_taken(q0, kb, Labs, W)) return 2;
          const TfExtendKey k = tf_extend_mfma_key(j, pos0, len, capacity, W, y);
          if (j >= pos0) { if (k.kind != kTfExtendKeyChunk || k.row != j - pos0) return 3; }
          else if (k.kind != kTfExtendKeyCache || held[(size_t)k.row] != j) return 3;
        }
      }
    }
  }
  return 0;
}

// The properties tests/test_tf_extend_mfma_host.py states, on heap arrays sized exactly (the sanitizer's business): 0, or a code that
// names the first property that failed.
int tfx_selfcheck(int scale) {
  using namespace flope_tf_plan;
  for (int c = 1; c <= (scale == 1 ? 8 : 4); ++c)
    for (int w = 0; w <= c; ++w)
      for (int a = 0; a <= 2 * c + 1; ++a)
        for (int l = 1; l <= 2 * c + 2; ++l)
          for (int da = -1; da <= 1; ++da)
            for (int dl = -1; dl <= 1; ++dl) {
              if (scale == 1 && (da || dl)) continue;
              const int capacity = c * scale, W = w * scale, pos0 = a * scale + da, len = l * scale + dl;
              if (pos0 < 0 || len < 1 || (!W && pos0 + len > capacity)) continue;
              if (tfx_walk(pos0, len, capacity, W)) return 1;
            }
  // the hook's checks
  const int n = 3;
  std::vector<int> lengths = {5, 9, 2}, cached = {0, 8, 1}, out(4);
  if (tfx_check_hook(3, 16, 0, 64, n, 9, lengths.data(), cached.data(), out.data()) != kTfStreamOk) return 2;
  if (out[1] != 9 || out[2] != 5 || out[3] != 7) return 3;
  cached[1] = 9;
  if (tfx_check_hook(3, 16, 0, 64, n, 9, lengths.data(), cached.data(), out.data()) != kTfStreamCached || out[0] != 1) return 4;
  cached[1] = -1;
  if (tfx_check_hook(3, 16, 0, 64, n, 9, lengths.data(), cached.data(), out.data()) != kTfStreamCached || out[0] != 1) return 4;
  cached[1] = 8;
  if (tfx_check_hook(3, 8, 0, 64, n, 9, lengths.data(), cached.data(), out.data()) != kTfStreamLength || out[0] != 1) return 5;
  if (tfx_check_hook(3, 8, 8, 64, n, 9, lengths.data(), cached.data(), out.data()) != kTfStreamOk || out[1] != 8) return 6;
  if (tfx_check_hook(2, 16, 0, 64, n, 9, lengths.data(), cached.data(), out.data()) != kTfStreamCount) return 7;
  if (tfx_check_hook(3, 16, 0, 6, n, 9, lengths.data(), cached.data(), out.data()) != kTfStreamTokens) return 8;
  if (tfx_check_hook(3, 16, 0, 64, n, 8, lengths.data(), cached.data(), out.data()) != kTfStreamLength || out[0] != 1) return 9;
  if (tfx_check_hook(3, 16, 0, 64, n, 9, nullptr, cached.data(), out.data()) != kTfStreamCount) return 10;
  if (tfx_check_hook(3, 16, 0, 64, n, 9, lengths.data(), nullptr, out.data()) != kTfStreamCount) return 10;
  // launches: every query has a lane, the ring is tf_attn_tiled's
  for (int max_len : {1, 127, 128, 129, 4096})
    for (int hd : {32, 64, 96, 128}) {
      const TfExtendLaunch l = tf_extend_mfma_launch(3, 6, max_len, hd);
      if (l.block != 256 || l.grid_x != 18u || (int)l.grid_y * 128 < max_len || ((int)l.grid_y - 1) * 128 >= max_len || l.lds != tf_attn_tiled_lds(hd)) return 11;
    }
  // positions: the last chunk the kernel takes, and the first it does not
  if (!tf_extend_mfma_positions_ok(kTfExtendMfmaPosMax - 7, 7) || tf_extend_mfma_positions_ok(kTfExtendMfmaPosMax - 6, 7)) return 12;
  if (tfx_walk(kTfExtendMfmaPosMax - 300, 300, 64, 33)) return 13;
  return 0;
}

}  // extern "C"

#ifdef TF_EXTEND16_MAIN
#include <stdio.h>
int main() {
  int rc = 0;
  for (int scale : {1, 32})
    if ((rc = tfx_selfcheck(scale))) { printf("tfx_selfcheck(%d) = %d\n", scale, rc); return rc; }
  printf("tfx_selfcheck = 0\n");
  return 0;
}
#endif
