// CPU-only test harness of sliding-window causal attention and the ring cache of a windowed stream state: the first
// visible key (flope_amd/csrc/tf_attn_plan.h: tf_window_lo, which tf_attn_row and tf_attn_stream_row call) and the host rules of
// flope_amd/csrc/tf_encoder_stream.h -- the open check, the windowed step and prefill checks, the slot of a position, the two row runs
// a step's value pass walks, and which tokens a fill writes.  tests/test_tf_window_host.py holds them against brute force without a
// GPU and runs tfw_selfcheck once in a stand-alone program built with -DTF_WINDOW_MAIN under AddressSanitizer + UBSan.  Not part of
// the product.
#include "tf_encoder_stream.h"

#include <limits.h>

#include <vector>

extern "C" {

int tfw_lo(int i, int W) { return flope_tf_plan::tf_window_lo(i, W); }
int tfw_keys(int i, int W) { return flope_tf_plan::tf_window_keys(i, W); }
int tfw_slot(int p, int capacity) { return flope_tf_plan::tf_stream_slot(p, capacity); }
int tfw_run0(int slo, int nk, int capacity) { return flope_tf_plan::tf_stream_run0(slo, nk, capacity); }
int tfw_fill_writes(int i, int len, int capacity) { return flope_tf_plan::tf_stream_fill_writes(i, len, capacity) ? 1 : 0; }
int tfw_check_open(int tracks, int capacity, int window) { return flope_tf_plan::tf_stream_check_open_window(tracks, capacity, window); }
int tfw_max_capacity() { return flope_tf_plan::kTfStreamMaxCapacity; }
long long tfw_step_lds(int max_pos) { return (long long)flope_tf_plan::tf_step_lds(max_pos); }
long long tfw_lds_max() { return (long long)flope_tf_plan::kTfStepLdsMax; }

int tfw_check_reset(int tracks, int n, const int* rows, int* bad) {
  *bad = -1;
  return flope_tf_plan::tf_stream_check_reset(tracks, n, rows, bad);
}
// lo[i] and keys[i] of every query i < L under window W
void tfw_lo_table(int L, int W, int* lo, int* keys) {
  for (int i = 0; i < L; ++i) { lo[i] = flope_tf_plan::tf_window_lo(i, W); keys[i] = flope_tf_plan::tf_window_keys(i, W); }
}
// row[i]: the ring row tf_cache_append writes token i of a sequence of len tokens to, -1 where it writes none
void tfw_fill_table(int len, int capacity, int* row) {
  for (int i = 0; i < len; ++i) row[i] = flope_tf_plan::tf_stream_fill_writes(i, len, capacity) ? flope_tf_plan::tf_stream_slot(i, capacity) : -1;
}

// One step call as flope_tf_stream_step makes it on a windowed state: check; when accepted, the table (2 n ints) and the advance.
// pos: `tracks` ints, changed only by an accepted call.  *bad and *max_pos as the check leaves them (-1 where untouched).
int tfw_step(int* pos, int tracks, int window, int max_tokens, int n, const int* rows, int* tab, int* bad, int* max_pos) {
  using namespace flope_tf_plan;
  std::vector<char> seen((size_t)(tracks > 0 ? tracks : 0));
  *bad = -1; *max_pos = -1;
  const int rc = tf_stream_check_step_window(pos, tracks, window, max_tokens, n, rows, seen.data(), bad, max_pos);
  if (rc) return rc;
  tf_stream_step_table(pos, n, rows, tab);
  tf_stream_advance(pos, n, rows);
  return rc;
}

int tfw_prefill(int* pos, int tracks, int n, int seq_len, const int* lengths, const int* rows, int* bad) {
  using namespace flope_tf_plan;
  std::vector<char> seen((size_t)(tracks > 0 ? tracks : 0));
  *bad = -1;
  const int rc = tf_stream_check_prefill_window(tracks, n, rows, seen.data(), bad);
  if (rc) return rc;
  tf_stream_set_lengths(pos, n, seq_len, lengths, rows);
  return rc;
}

// The cache rows the step at position p reads, in the order tf_attn_stream_row's value pass walks them (two runs), without the token's
// own: out gets tf_window_keys(p, W) - 1 rows; returns that count.  Every index is formed as the kernel forms it.
int tfw_step_rows(int p, int W, int capacity, int* out) {
  using namespace flope_tf_plan;
  const int lo = tf_window_lo(p, W), slo = tf_stream_slot(lo, capacity), nk = p - lo, first = tf_stream_run0(slo, nk, capacity);
  int m = 0;
  for (int j = 0; j < first; ++j) out[m++] = slo + j;
  for (int j = 0; j < nk - first; ++j) out[m++] = j;
  return m;
}
// ... and the row of key lo + j as the score pass forms it: one add, one conditional subtract
int tfw_score_row(int p, int W, int capacity, int j) {
  using namespace flope_tf_plan;
  int row = tf_stream_slot(tf_window_lo(p, W), capacity) + j;
  if (row >= capacity) row -= capacity;
  return row;
}

// A model of one track's ring on heap arrays sized exactly (the sanitizer's business): ring[r] = the absolute position whose k | v
// row r holds, -1 = never written.  Steps `steps` tokens from position `start` (behind a fill of `start` tokens when start > 0) and
// holds every read and write to the rules.  0, or a code that names the first property that failed.
int tfw_selfcheck_ring(int capacity, int W, int start, int steps) {
  using namespace flope_tf_plan;
  if (tf_stream_check_open_window(1, capacity, W)) return 1;
  std::vector<int> ring((size_t)capacity, -1), rows((size_t)W);
  std::vector<int> writes((size_t)capacity, 0);
  if (start > 2 * capacity && (tf_stream_fill_writes(0, start, capacity) || tf_stream_fill_writes(start - capacity - 1, start, capacity))) return 4;
  for (int i = start > 2 * capacity ? start - 2 * capacity : 0; i < start; ++i)      // the fill: each row at most once, the last min(len, capacity) tokens
    if (tf_stream_fill_writes(i, start, capacity)) {
      const int r = tf_stream_slot(i, capacity);
      if (r < 0 || r >= capacity) return 2;
      if (writes[(size_t)r]++) return 3;
      ring[(size_t)r] = i;
    } else if (i >= start - capacity) return 4;
  int filled = 0;
  for (int r = 0; r < capacity; ++r) filled += writes[(size_t)r];
  if (filled != (start < capacity ? start : capacity)) return 5;
  for (int p = start; p < start + steps; ++p) {
    const int lo = tf_window_lo(p, W), slot = tf_stream_slot(p, capacity);
    if (lo != (p + 1 - W > 0 ? p + 1 - W : 0) || tf_window_keys(p, W) != p - lo + 1 || tf_window_keys(p, W) > W) return 6;
    if (slot < 0 || slot >= capacity) return 7;
    if (ring[(size_t)slot] >= lo) return 8;                              // the row a step overwrites is outside its window
    ring[(size_t)slot] = p;                                              // the kernel stores first, then reads keys lo .. p - 1
    const int m = tfw_step_rows(p, W, capacity, rows.data());
    if (m != p - lo) return 9;
    for (int j = 0; j < m; ++j) {
      if (rows[(size_t)j] < 0 || rows[(size_t)j] >= capacity) return 10;
      if (ring[(size_t)rows[(size_t)j]] != lo + j) return 11;            // key lo + j, in key order, never a stale row
      if (tfw_score_row(p, W, capacity, j) != rows[(size_t)j]) return 12;
    }
  }
  return 0;
}

// The argument checks on heap arrays sized exactly
int tfw_selfcheck_checks(int tracks) {
  using namespace flope_tf_plan;
  const int W = 3;
  std::vector<int> pos((size_t)tracks, 0), rows((size_t)tracks), tab((size_t)2 * tracks), lens((size_t)tracks);
  int bad, mp;
  for (int r = 0; r < tracks; ++r) rows[(size_t)r] = tracks - 1 - r;
  for (int t = 0; t < 3 * W; ++t) {                                      // past any capacity: never full
    if (tfw_step(pos.data(), tracks, W, tracks, tracks, rows.data(), tab.data(), &bad, &mp) || mp != (t < W - 1 ? t : W - 1)) return 20;
    for (int r = 0; r < tracks; ++r)
      if (tab[(size_t)2 * r] != tracks - 1 - r || tab[(size_t)2 * r + 1] != t) return 21;
  }
  pos[(size_t)tracks - 1] = INT_MAX;                                     // the only full there is; row 0 names track tracks - 1
  if (tfw_step(pos.data(), tracks, W, tracks, tracks, rows.data(), tab.data(), &bad, &mp) != kTfStreamFull || bad != 0) return 22;
  if (tfw_step(pos.data(), tracks, W, tracks, tracks, nullptr, tab.data(), &bad, &mp) != kTfStreamFull || bad != tracks - 1) return 23;
  for (int t = 0; t + 1 < tracks; ++t)
    if (pos[(size_t)t] != 3 * W) return 24;                              // a refusal moves nothing
  pos[(size_t)tracks - 1] = INT_MAX - 1;
  if (tracks == 1) {
    if (tfw_step(pos.data(), tracks, W, tracks, tracks, nullptr, tab.data(), &bad, &mp) || pos[0] != INT_MAX || mp != W - 1) return 25;
  }
  if (tracks >= 2) {
    rows[1] = rows[0];
    if (tfw_step(pos.data(), tracks, W, tracks, tracks, rows.data(), tab.data(), &bad, &mp) != kTfStreamDuplicate || bad != 1) return 26;
    rows[1] = tracks;
    if (tfw_step(pos.data(), tracks, W, tracks, tracks, rows.data(), tab.data(), &bad, &mp) != kTfStreamRange || bad != 1) return 27;
    rows[1] = tracks - 2;
  }
  if (tfw_step(pos.data(), tracks, W, tracks, 0, rows.data(), tab.data(), &bad, &mp) != kTfStreamCount) return 28;
  // prefill: lengths past any capacity are accepted, positions are the lengths
  for (int b = 0; b < tracks; ++b) lens[(size_t)b] = 1 + 5 * b;
  for (int r = 0; r < tracks; ++r) rows[(size_t)r] = r;
  if (tfw_prefill(pos.data(), tracks, tracks, 1 + 5 * tracks, lens.data(), rows.data(), &bad)) return 29;
  for (int b = 0; b < tracks; ++b)
    if (pos[(size_t)b] != 1 + 5 * b) return 30;
  rows[0] = tracks;
  if (tfw_prefill(pos.data(), tracks, tracks, 9, lens.data(), rows.data(), &bad) != kTfStreamRange || bad != 0 || pos[0] != 1) return 31;
  return 0;
}

}  // extern "C"

#ifdef TF_WINDOW_MAIN
#include <stdio.h>
int main() {
  int rc = 0;
  for (int capacity : {1, 2, 4, 6, 7, 64, 96})
    for (int W = 1; W <= capacity; W += (W < 8 ? 1 : 13))
      for (int start : {0, 1, capacity - 1, capacity, capacity + 1, 3 * capacity + 2})
        if ((rc = tfw_selfcheck_ring(capacity, W, start, 3 * capacity + 5))) {
          printf("tfw_selfcheck_ring(%d, %d, %d) = %d\n", capacity, W, start, rc);
          return rc;
        }
  if ((rc = tfw_selfcheck_ring(4096, 4096, INT_MAX - 5000, 4999)) || (rc = tfw_selfcheck_ring(256, 256, INT_MAX - 300, 299))) {
    printf("tfw_selfcheck_ring at INT_MAX = %d\n", rc);
    return rc;
  }
  for (int tracks : {1, 2, 7, 64})
    if ((rc = tfw_selfcheck_checks(tracks))) { printf("tfw_selfcheck_checks(%d) = %d\n", tracks, rc); return rc; }
  printf("tfw_selfcheck = 0\n");
  return 0;
}
#endif
