// CPU-only test harness of flope_tf_stream_extend's planner (flope_amd/csrc/tf_encoder_stream.h): the argument checks
// over host arrays for linear and windowed states, the per-sequence table, smax and the LDS figure, the advance of the positions,
// the launches of tf_attn_extend and tf_cache_append, where a chunk query's keys lie, and which cache rows the append writes.
// tests/test_tf_extend_host.py holds them against brute force without a GPU and runs tfe_selfcheck once in a stand-alone program built
// with -DTF_EXTEND_MAIN under AddressSanitizer + UBSan.  Not part of the product.
#include "tf_encoder_stream.h"

#include <algorithm>
#include <vector>

extern "C" {

int tfe_cached(int pos0, int lo) { return flope_tf_plan::tf_extend_cached(pos0, lo); }
int tfe_chunk0(int pos0, int lo) { return flope_tf_plan::tf_extend_chunk0(pos0, lo); }
int tfe_keys(int pos0, int len, int W) { return flope_tf_plan::tf_extend_keys(pos0, len, W); }
int tfe_window_lo(int p, int W) { return flope_tf_plan::tf_window_lo(p, W); }
int tfe_run0(int slo, int nk, int capacity) { return flope_tf_plan::tf_stream_run0(slo, nk, capacity); }
int tfe_append_writes(int i, int len, int capacity) { return flope_tf_plan::tf_stream_append_writes(i, len, capacity) ? 1 : 0; }
int tfe_append_slot(int pos0, int i, int capacity) { return flope_tf_plan::tf_stream_append_slot(pos0, i, capacity); }
long long tfe_lds_max() { return (long long)flope_tf_plan::kTfStepLdsMax; }

// out: grid_x, grid_y, block, lds
void tfe_extend_launch(int n, int H, int max_len, int smax, long long* out) {
  const flope_tf_plan::TfExtendLaunch l = flope_tf_plan::tf_extend_launch(n, H, max_len, smax);
  out[0] = l.grid_x; out[1] = l.grid_y; out[2] = l.block; out[3] = (long long)l.lds;
}
// out: grid_x, block, lds
void tfe_append_launch(int n, int max_len, int units, long long* out) {
  const flope_tf_plan::TfStreamLaunch l = flope_tf_plan::tf_cache_append_launch(n, max_len, units);
  out[0] = l.grid_x; out[1] = l.block; out[2] = (long long)l.lds;
}

// One extend call as flope_tf_stream_extend makes it: tf_varlen_plan first (its code + 100 comes back: 99 batch, 98 a length, 97 the
// token limit, 96 overflow), then the state's check; when accepted, the table (2 n ints), off (n + 1 ints) and the advance.  window = 0:
// a linear state.  lengths == NULL: every chunk has seq_len tokens.  pos: `tracks` ints, changed only by an accepted call.  *bad and
// *smax as the checks leave them (-1 where untouched).
int tfe_extend(int* pos, int tracks, int capacity, int window, int max_tokens, int n, int seq_len, const int* lengths, const int* rows, int* tab, int* off,
               int* bad, int* smax) {
  using namespace flope_tf_plan;
  std::vector<char> seen((size_t)(tracks > 0 ? tracks : 0));
  std::vector<int> full;
  if (!lengths && n > 0) full.assign((size_t)n, seq_len);
  const int* len = lengths ? lengths : full.data();
  *bad = -1; *smax = -1;
  int T = 0, max_len = 0;
  int rc = tf_varlen_plan(len, n, seq_len, max_tokens, off, &T, &max_len, bad);
  if (rc) return rc + 100;
  rc = tf_stream_check_extend(pos, tracks, capacity, window, n, len, rows, seen.data(), bad, smax);
  if (rc) return rc;
  tf_stream_extend_table(pos, n, rows, tab);
  tf_stream_extend_advance(pos, n, len, rows);
  return rc;
}

// A ring (window >= 1) or a linear cache (window = 0) of one track as sets of positions, walked as the two kernels walk it: 0, or a
// code naming the first property that failed for the chunk (pos0, len).
//   1  the append writes a row twice, a row outside the cache, or not exactly the rows of the chunk's last min(len, capacity) tokens
//   2  behind the call a key that a later query (any position >= pos0 + len) can see is not in its row
//   3  a chunk query reads a cached key the pre-call cache does not hold in that row (append behind the attention: never)
//   4  a chunk query's keys are not lo .. p in order, each once, split into cached keys and chunk rows as the kernel splits them
// append_first != 0 walks the other order (the append in front of the attention) and returns 3 where the hazard bites.
int tfe_walk(int pos0, int len, int capacity, int W, int append_first) {
  using namespace flope_tf_plan;
  // the pre-call cache: row r holds the latest position < pos0 with that row (a linear cache: positions 0 .. pos0 - 1), -1 if none
  std::vector<long long> held((size_t)capacity, -1);
  for (int j = 0; j < pos0; ++j)
    if (W) held[(size_t)tf_stream_slot(j, capacity)] = j;
    else if (j < capacity) held[(size_t)j] = j;
  std::vector<long long> after(held);
  std::vector<int> writes((size_t)capacity, 0);
  int written = 0;
  for (int i = 0; i < len; ++i) {
    const bool w = W ? tf_stream_append_writes(i, len, capacity) : true;
    if (!w) continue;
    const int row = W ? tf_stream_append_slot(pos0, i, capacity) : pos0 + i;
    if (row < 0 || row >= capacity || writes[(size_t)row]++) return 1;
    after[(size_t)row] = (long long)pos0 + i;
    ++written;
  }
  if (written != (W ? std::min(len, capacity) : len)) return 1;
  for (int i = std::max(0, len - capacity); i < len; ++i)
    if (after[(size_t)(W ? (pos0 + i) % capacity : pos0 + i)] != (long long)pos0 + i) return 1;
  // a later query at p >= pos0 + len sees keys tf_window_lo(p, W) .. p - 1 of the cache; the first such query sees the most
  {
    const int p = pos0 + len;
    for (int j = tf_window_lo(p, W); j < p; ++j)
      if (after[(size_t)(W ? j % capacity : j)] != j) return 2;
  }
  const std::vector<long long>& seen_cache = append_first ? after : held;
  for (int i = 0; i < len; ++i) {
    const int p = pos0 + i, lo = tf_window_lo(p, W), nc = tf_extend_cached(pos0, lo), c0 = tf_extend_chunk0(pos0, lo), L = p - lo + 1;
    if (L != tf_window_keys(p, W) || L > tf_extend_keys(pos0, len, W) || nc < 0 || nc > L) return 4;
    const int slo = W ? tf_stream_slot(lo, capacity) : 0;
    const int first = W ? tf_stream_run0(slo, nc, capacity) : nc;
    if (first < 0 || first > nc) return 4;
    for (int j = 0; j < L; ++j) {                 // key lo + j, as the score pass finds it
      if (j < nc) {
        int row = W ? slo + j : j;
        if (W && row >= capacity) row -= capacity;
        // ... and as the value pass does: run one from slo, run two from row 0
        const int vrow = j < first ? slo + j : j - first;
        if (row != vrow || row < 0 || row >= capacity) return 4;
        if (seen_cache[(size_t)row] != (long long)lo + j) return 3;
      } else {
        const int cr = c0 + j - nc;               // chunk row
        if (cr < 0 || cr > i || pos0 + cr != lo + j) return 4;
      }
    }
    if (c0 + (L - nc) - 1 != i) return 4;        // the last key is the query's own
  }
  return 0;
}

// The properties tests/test_tf_extend_host.py states, on heap arrays sized exactly (the sanitizer's business): 0, or a code that names
// the first property that failed.
int tfe_selfcheck(int tracks) {
  using namespace flope_tf_plan;
  for (int capacity = 1; capacity <= 9; ++capacity)
    for (int W = 0; W <= capacity; ++W)
      for (int pos0 = 0; pos0 <= 2 * capacity + 1; ++pos0)
        for (int len = 1; len <= 2 * capacity + 2; ++len) {
          if (!W && pos0 + len > capacity) continue;
          if (tfe_walk(pos0, len, capacity, W, 0)) return 1;
          // the other order fails exactly where the chunk's first query has a cached key (W >= 2, pos0 >= 1) and the chunk reaches the
          // row of the first of them: max(0, pos0 + 1 - W) + capacity <= pos0 + len - 1 -- a track of W - 1 tokens or more:
          // len >= capacity - W + 2
          if (W) {
            const int rc = tfe_walk(pos0, len, capacity, W, 1);
            const bool expect = W >= 2 && pos0 >= 1 && std::max(0, pos0 + 1 - W) + capacity <= pos0 + len - 1;
            if (rc != (expect ? 3 : 0)) return 2;
          }
        }
  const int capacity = 5;
  std::vector<int> pos((size_t)tracks, 0), rows((size_t)tracks), lens((size_t)tracks), tab((size_t)2 * tracks), off((size_t)tracks + 1);
  int bad, smax;
  for (int r = 0; r < tracks; ++r) { rows[(size_t)r] = tracks - 1 - r; lens[(size_t)r] = 1 + r % 3; }
  // linear: accepted, table and positions; then one more chunk of 3 passes the capacity for the tracks that hold 3
  if (tfe_extend(pos.data(), tracks, capacity, 0, 3 * tracks, tracks, 3, lens.data(), rows.data(), tab.data(), off.data(), &bad, &smax)) return 3;
  for (int r = 0; r < tracks; ++r)
    if (tab[(size_t)2 * r] != tracks - 1 - r || tab[(size_t)2 * r + 1] != 0 || pos[(size_t)(tracks - 1 - r)] != 1 + r % 3 || off[(size_t)r + 1] - off[(size_t)r] != 1 + r % 3) return 4;
  if (smax != (tracks >= 3 ? 3 : tracks)) return 5;
  std::vector<int> keep(pos);
  int rc = tfe_extend(pos.data(), tracks, capacity, 0, 3 * tracks, tracks, 3, nullptr, rows.data(), tab.data(), off.data(), &bad, &smax);
  if (tracks >= 3 ? (rc != kTfStreamRoom || bad != 2) : rc != kTfStreamOk) return 6;
  if (tracks >= 3 && pos != keep) return 7;
  // a ring takes any length, up to INT_MAX
  std::fill(pos.begin(), pos.end(), INT_MAX - 4);
  if (tfe_extend(pos.data(), tracks, capacity, 3, 4 * tracks, tracks, 4, nullptr, nullptr, tab.data(), off.data(), &bad, &smax) || smax != 3) return 8;
  if (tfe_extend(pos.data(), tracks, capacity, 3, 4 * tracks, tracks, 4, nullptr, nullptr, tab.data(), off.data(), &bad, &smax) != kTfStreamFull || bad != 0) return 9;
  for (int t = 0; t < tracks; ++t)
    if (pos[(size_t)t] != INT_MAX) return 10;
  // the varlen checks come first
  lens[0] = 0;
  if (tfe_extend(pos.data(), tracks, capacity, 3, 4 * tracks, tracks, 4, lens.data(), rows.data(), tab.data(), off.data(), &bad, &smax) != kTfVarlenLength + 100 || bad != 0) return 11;
  if (tfe_extend(pos.data(), tracks, capacity, 3, tracks, tracks, 4, nullptr, rows.data(), tab.data(), off.data(), &bad, &smax) != kTfVarlenTokens + 100) return 12;
  // launches: every query has a wave, the score rows fit
  for (int max_len : {1, 3, 4, 5, 255, 256, 257, 4096}) {
    const TfExtendLaunch l = tf_extend_launch(tracks, 6, max_len, kTfStreamMaxCapacity);
    if (l.block != 256 || l.grid_x != (unsigned)tracks * 6 || l.grid_y < 1 || l.grid_y > 64 || l.lds > kTfStepLdsMax) return 13;
    if (l.grid_y < 64 && (int)l.grid_y * 4 < max_len) return 14;
  }
  return 0;
}

}  // extern "C"

#ifdef TF_EXTEND_MAIN
#include <stdio.h>
int main() {
  int rc = 0;
  for (int tracks : {1, 2, 7, 64})
    if ((rc = tfe_selfcheck(tracks))) { printf("tfe_selfcheck(%d) = %d\n", tracks, rc); return rc; }
  printf("tfe_selfcheck = 0\n");
  return 0;
}
#endif
