// CPU-only test harness of the streaming forward's planner (flope_amd/csrc/tf_encoder_stream.h): the argument checks of
// flope_tf_stream_step / _prefill / _reset over host arrays, the capacity limit and the launches of tf_attn_step and tf_cache_append.
// tests/test_tf_stream_host.py holds them against brute force without a GPU and runs tfs_selfcheck once in a stand-alone program
// built with -DTF_STREAM_MAIN under AddressSanitizer + UBSan.  Not part of the product.
#include "tf_encoder_stream.h"

#include <algorithm>
#include <vector>

extern "C" {

int tfs_max_capacity() { return flope_tf_plan::kTfStreamMaxCapacity; }
long long tfs_lds_max() { return (long long)flope_tf_plan::kTfStepLdsMax; }
long long tfs_step_lds(int max_pos) { return (long long)flope_tf_plan::tf_step_lds(max_pos); }
int tfs_check_open(int tracks, int capacity) { return flope_tf_plan::tf_stream_check_open(tracks, capacity); }
int tfs_vec(int esz) { return flope_tf_plan::tf_stream_vec(esz); }
int tfs_step_vec_ok(int head_dim, int esz) { return flope_tf_plan::tf_step_vec_ok(head_dim, esz) ? 1 : 0; }
int tfs_cache_fill_vec_ok(int model_dim, int esz) { return flope_tf_plan::tf_cache_fill_vec_ok(model_dim, esz) ? 1 : 0; }

// out: grid_x, block, lds
void tfs_step_launch(int n, int H, int max_pos, long long* out) {
  const flope_tf_plan::TfStreamLaunch l = flope_tf_plan::tf_step_launch(n, H, max_pos);
  out[0] = l.grid_x; out[1] = l.block; out[2] = (long long)l.lds;
}
void tfs_cache_fill_launch(int n, int max_len, int units, long long* out) {
  const flope_tf_plan::TfStreamLaunch l = flope_tf_plan::tf_cache_fill_launch(n, max_len, units);
  out[0] = l.grid_x; out[1] = l.block; out[2] = (long long)l.lds;
}

// One step call as flope_tf_stream_step makes it: check; when accepted, the table (2 n ints) and the advance.  pos: `tracks` ints,
// changed only by an accepted call.  Returns the check's code; *bad and *max_pos as the check leaves them (-1 where untouched).
int tfs_step(int* pos, int tracks, int capacity, int max_tokens, int n, const int* rows, int* tab, int* bad, int* max_pos) {
  using namespace flope_tf_plan;
  std::vector<char> seen((size_t)(tracks > 0 ? tracks : 0));
  *bad = -1; *max_pos = -1;
  const int rc = tf_stream_check_step(pos, tracks, capacity, max_tokens, n, rows, seen.data(), bad, max_pos);
  if (rc) return rc;
  tf_stream_step_table(pos, n, rows, tab);
  tf_stream_advance(pos, n, rows);
  return rc;
}

int tfs_prefill(int* pos, int tracks, int capacity, int n, int seq_len, const int* lengths, const int* rows, int* bad) {
  using namespace flope_tf_plan;
  std::vector<char> seen((size_t)(tracks > 0 ? tracks : 0));
  *bad = -1;
  const int rc = tf_stream_check_prefill(tracks, capacity, n, seq_len, lengths, rows, seen.data(), bad);
  if (rc) return rc;
  tf_stream_set_lengths(pos, n, seq_len, lengths, rows);
  return rc;
}

int tfs_check_reset(int tracks, int n, const int* rows, int* bad) {
  *bad = -1;
  return flope_tf_plan::tf_stream_check_reset(tracks, n, rows, bad);
}

// The properties tests/test_tf_stream_host.py states, on heap arrays sized exactly (the sanitizer's business): 0, or a code that names
// the first property that failed.
int tfs_selfcheck(int tracks) {
  using namespace flope_tf_plan;
  // the LDS figure covers 4 (pos + 1) floats at every position up to the limit, and the limit is the largest capacity that fits
  for (int p = 0; p < kTfStreamMaxCapacity; ++p)
    if (tf_step_lds(p) != (size_t)16 * ((size_t)p + 1) || tf_step_lds(p) > kTfStepLdsMax) return 1;
  if (tf_step_lds(kTfStreamMaxCapacity) <= kTfStepLdsMax) return 2;
  if (tf_stream_check_open(tracks, kTfStreamMaxCapacity) || !tf_stream_check_open(tracks, kTfStreamMaxCapacity + 1) || !tf_stream_check_open(0, 1) ||
      !tf_stream_check_open(tracks, 0))
    return 3;
  const int capacity = 3;
  std::vector<int> pos((size_t)tracks, 0), rows((size_t)tracks), tab((size_t)2 * tracks);
  int bad, mp;
  // every track, in reverse order, until full
  for (int r = 0; r < tracks; ++r) rows[(size_t)r] = tracks - 1 - r;
  for (int t = 0; t < capacity; ++t) {
    if (tfs_step(pos.data(), tracks, capacity, tracks, tracks, rows.data(), tab.data(), &bad, &mp) || mp != t) return 4;
    for (int r = 0; r < tracks; ++r)
      if (tab[(size_t)2 * r] != tracks - 1 - r || tab[(size_t)2 * r + 1] != t) return 5;
  }
  if (tfs_step(pos.data(), tracks, capacity, tracks, tracks, rows.data(), tab.data(), &bad, &mp) != kTfStreamFull || bad != 0) return 6;
  if (tfs_step(pos.data(), tracks, capacity, tracks, tracks, nullptr, tab.data(), &bad, &mp) != kTfStreamFull || bad != 0) return 7;
  for (int t = 0; t < tracks; ++t)
    if (pos[(size_t)t] != capacity) return 8;                      // a refusal moves nothing
  // each refusal names its row
  std::fill(pos.begin(), pos.end(), 0);
  for (int r = 0; r < tracks; ++r) rows[(size_t)r] = r;
  if (tracks >= 2) {
    for (int r = 1; r < tracks; ++r) {
      const int keep = rows[(size_t)r];
      rows[(size_t)r] = rows[(size_t)r - 1];
      if (tfs_step(pos.data(), tracks, capacity, tracks, tracks, rows.data(), tab.data(), &bad, &mp) != kTfStreamDuplicate || bad != r) return 9;
      rows[(size_t)r] = tracks;
      if (tfs_step(pos.data(), tracks, capacity, tracks, tracks, rows.data(), tab.data(), &bad, &mp) != kTfStreamRange || bad != r) return 10;
      rows[(size_t)r] = -1;
      if (tfs_step(pos.data(), tracks, capacity, tracks, tracks, rows.data(), tab.data(), &bad, &mp) != kTfStreamRange || bad != r) return 11;
      rows[(size_t)r] = keep;
    }
  }
  if (tfs_step(pos.data(), tracks, capacity, tracks, 0, rows.data(), tab.data(), &bad, &mp) != kTfStreamCount) return 12;
  if (tfs_step(pos.data(), tracks, capacity, tracks, tracks + 1, rows.data(), tab.data(), &bad, &mp) != kTfStreamCount) return 13;
  if (tracks >= 2 && tfs_step(pos.data(), tracks, capacity, tracks - 1, tracks, rows.data(), tab.data(), &bad, &mp) != kTfStreamCount) return 14;
  if (tracks >= 2 && tfs_step(pos.data(), tracks, capacity, tracks, tracks - 1, nullptr, tab.data(), &bad, &mp) != kTfStreamCount) return 15;
  for (int t = 0; t < tracks; ++t)
    if (pos[(size_t)t] != 0) return 16;
  // prefill: lengths within capacity, positions set for the named tracks only
  std::vector<int> lens((size_t)tracks);
  for (int b = 0; b < tracks; ++b) lens[(size_t)b] = 1 + b % capacity;
  if (tfs_prefill(pos.data(), tracks, capacity, tracks, capacity, lens.data(), rows.data(), &bad)) return 17;
  for (int b = 0; b < tracks; ++b)
    if (pos[(size_t)b] != 1 + b % capacity) return 18;
  lens[(size_t)tracks - 1] = capacity + 1;
  if (tfs_prefill(pos.data(), tracks, capacity, tracks, capacity + 1, lens.data(), rows.data(), &bad) != kTfStreamLength || bad != tracks - 1) return 19;
  if (tfs_prefill(pos.data(), tracks, capacity, tracks, capacity + 1, nullptr, nullptr, &bad) != kTfStreamLength || bad != 0) return 20;
  if (pos[(size_t)tracks - 1] != 1 + (tracks - 1) % capacity) return 21;
  rows[0] = tracks;
  if (tfs_check_reset(tracks, 1, rows.data(), &bad) != kTfStreamRange || bad != 0) return 22;
  if (tfs_check_reset(tracks, 0, rows.data(), &bad) != kTfStreamCount || tfs_check_reset(tracks, 0, nullptr, &bad)) return 23;
  return 0;
}

}  // extern "C"

#ifdef TF_STREAM_MAIN
#include <stdio.h>
int main() {
  int rc = 0;
  for (int tracks : {1, 2, 7, 64})
    if ((rc = tfs_selfcheck(tracks))) { printf("tfs_selfcheck(%d) = %d\n", tracks, rc); return rc; }
  printf("tfs_selfcheck = 0\n");
  return 0;
}
#endif
