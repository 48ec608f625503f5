// Host-only view of the step_split planner of flope_amd/csrc/tf_encoder_stream.h: the partition of a token's visible
// keys into (wave, block, lane), the lane groups of the value pass, the LDS bytes, both launches, the eligibility rule, where a key of
// a step or of an extend query lies, and the checks of flope_tf_stream_attention -- the functions tf_encoder.hip calls, with C linkage.
// tests/test_tf_step_split_host.py holds them against brute force without a GPU and runs tfs_selfcheck once in a stand-alone program
// built with -DTF_SPLIT_MAIN under AddressSanitizer + UBSan.  Not part of the product.
#include "tf_encoder_stream.h"

#include <vector>

extern "C" {

using namespace flope_tf_plan;

int tfs_waves() { return kTfSplitWaves; }
int tfs_block() { return kTfSplitBlock; }
int tfs_key_block(int k) { return tf_split_block(k); }
int tfs_key_lane(int k) { return tf_split_lane(k); }
int tfs_block_wave(int b) { return tf_split_wave(b); }
int tfs_blocks(int L) { return tf_split_blocks(L); }
int tfs_wave_blocks(int L, int w) { return tf_split_wave_blocks(L, w); }
int tfs_lanes(int head_dim, int esz) { return tf_split_lanes(head_dim, esz); }
int tfs_ok(int head_dim, int esz) { return tf_step_split_ok(head_dim, esz); }
int tfs_vec_ok(int head_dim, int esz) { return tf_step_vec_ok(head_dim, esz); }
long long tfs_lds(int head_dim) { return (long long)tf_split_lds(head_dim); }
int tfs_cache_row(int k, int slo, int capacity) { return tf_split_cache_row(k, slo, capacity); }
void tfs_step_launch(int n, int H, int head_dim, long long* out) {
  const TfStreamLaunch l = tf_step_split_launch(n, H, head_dim);
  out[0] = l.grid_x; out[1] = l.block; out[2] = (long long)l.lds;
}
void tfs_extend_launch(int n, int H, int max_len, int head_dim, long long* out) {
  const TfExtendLaunch l = tf_extend_split_launch(n, H, max_len, head_dim);
  out[0] = l.grid_x; out[1] = l.grid_y; out[2] = l.block; out[3] = (long long)l.lds;
}
int tfs_check_attention(int tracks, int capacity, int window, int max_tokens, int n, int seq_len, const int* lengths, int* bad, int* max_pos) {
  return tf_stream_check_attention(tracks, capacity, window, max_tokens, n, seq_len, lengths, bad, max_pos);
}

// The walk of tf_attn_split_row over the L visible keys of a query, as the kernel makes it: wave w, its blocks in ascending order, lane
// l scores key 64 b + l; in the value pass group g of 64 / lps lane groups takes keys g, g + G, .. of the block.  owner[k] counts the
// (wave, block, lane) that score key k, taker[k] the lane groups that add its value.  0, or the first failure
int tfs_walk_partition(int L, int lps, int* owner, int* taker) {
  const int G = 64 / lps;
  for (int k = 0; k < L; ++k) owner[k] = taker[k] = 0;
  int walked = 0;
  for (int w = 0; w < kTfSplitWaves; ++w) {
    int nbw = 0, last = -1;
    for (int b = w; b < tf_split_blocks(L); b += kTfSplitWaves) {
      if (tf_split_wave(b) != w || b <= last) return 1;
      last = b; ++nbw;
      const int k0 = b * kTfSplitBlock, cnt = L - k0 < kTfSplitBlock ? L - k0 : kTfSplitBlock;
      if (cnt < 1) return 2;
      for (int l = 0; l < 64; ++l)
        if (l < cnt) {
          const int k = k0 + l;
          if (k < 0 || k >= L || tf_split_block(k) != b || tf_split_lane(k) != l) return 3;
          ++owner[k];
        }
      for (int g = 0; g < G; ++g)
        for (int t = g; t < cnt; t += G) { if (k0 + t >= L) return 4; ++taker[k0 + t]; }
    }
    if (nbw != tf_split_wave_blocks(L, w)) return 5;
    walked += nbw;
  }
  return walked == tf_split_blocks(L) ? 0 : 6;
}

// Where the kernels find visible key k of the query at chunk row i of an extend (pos0 tokens held; a step is i = 0, len = 1):
// *cached: 1 a cache row (*row), 0 the chunk's row *row.  The TfSplitKeys the kernels build, spelled with the same functions
void tfs_extend_key(int pos0, int i, int capacity, int W, int k, int* cached, int* row) {
  const int p = pos0 + i, lo = tf_window_lo(p, W);
  const int nc = tf_extend_cached(pos0, lo), c0 = tf_extend_chunk0(pos0, lo), slo = W ? tf_stream_slot(lo, capacity) : 0;
  if (k < nc) { *cached = 1; *row = W ? tf_split_cache_row(k, slo, capacity) : k; }
  else { *cached = 0; *row = c0 + k - nc; }
}

// Every property once, on ranges small enough for a sanitizer run: 0 or the first failure
int tfs_selfcheck(int maxL) {
  std::vector<int> owner((size_t)maxL), taker((size_t)maxL);
  for (int lps = 1; lps <= 64; lps *= 2)
    for (int L = 1; L <= maxL; ++L) {
      if (int rc = tfs_walk_partition(L, lps, owner.data(), taker.data())) return 10 + rc;
      for (int k = 0; k < L; ++k)
        if (owner[k] != 1 || taker[k] != 1) return 20;
    }
  for (int capacity = 1; capacity <= 9; ++capacity)
    for (int W = 0; W <= capacity; ++W)
      for (int pos0 = 0; pos0 <= 2 * capacity + 1; ++pos0)
        for (int len = 1; len <= capacity + 2; ++len) {
          if (!W && pos0 + len > capacity) continue;
          for (int i = 0; i < len; ++i) {
            const int p = pos0 + i, lo = tf_window_lo(p, W);
            for (int k = 0; k <= p - lo; ++k) {
              int cached, row;
              tfs_extend_key(pos0, i, capacity, W, k, &cached, &row);
              const int j = lo + k;                                    // the key's absolute position
              if (cached != (j < pos0)) return 30;
              if (cached && row != (W ? j % capacity : j)) return 31;
              if (cached && (row < 0 || row >= capacity)) return 32;
              if (!cached && (row != j - pos0 || row < 0 || row > i)) return 33;
            }
          }
        }
  for (int hd = 1; hd <= 256; ++hd)
    for (int esz = 2; esz <= 4; esz += 2) {
      const int ve = 16 / esz;
      bool want = hd % ve == 0;
      if (want) { const int lps = hd / ve; want = lps <= 64 && (lps & (lps - 1)) == 0; }
      if ((tf_step_split_ok(hd, esz) != 0) != want) return 40;
      if (tf_step_split_ok(hd, esz) && !tf_step_vec_ok(hd, esz)) return 41;
    }
  if (tf_split_lds(128) > 64 * 1024) return 50;
  return 0;
}

}  // extern "C"

#ifdef TF_SPLIT_MAIN
#include <stdio.h>
int main() {
  const int rc = tfs_selfcheck(700);
  printf("tfs_selfcheck = %d\n", rc);
  return rc;
}
#endif
