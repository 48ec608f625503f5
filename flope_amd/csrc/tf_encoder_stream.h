// The streaming causal forward of the encoder (flope_tf_stream_*) as far as it is plain integer arithmetic, no HIP:
// the argument checks of step / prefill / reset over host arrays, the capacity limit, and grid, block and LDS of tf_attn_step and
// of the one cache copy, tf_cache_append.  Shared by tf_encoder.hip and tests/host_harness/harness_tf_stream.cpp (tests/test_tf_stream_host.py holds it
// against brute force on the CPU, tests/test_gpu_tf_stream.py the device against it).
// Below them, the same for a windowed state (flope_tf_stream_open_window): a ring cache, absolute positions, keys
// tf_window_lo(p, W) .. p -- new functions beside the old ones (tests/host_harness/harness_tf_window.cpp, tests/test_tf_window_host.py).
// Below those, flope_tf_stream_extend: its checks, table, smax and advance for both kinds of state, the launches of
// tf_attn_extend, where a chunk query's keys lie and which rows tf_cache_append writes and where -- the prefill's copy is the append
// at pos0 = 0, and a step's table is an extend's: where two names below mean one function (tf_cache_fill_launch and
// tf_cache_append_launch, tf_stream_fill_writes and tf_stream_append_writes, tf_stream_step_table and tf_stream_extend_table), both
// stay because the host harnesses of the stream, window and extend planners are built against them by name
// (tests/host_harness/harness_tf_extend.cpp, tests/test_tf_extend_host.py).
// Below those, option step_split: the partition of a token's visible keys over the waves, blocks and lanes of a workgroup,
// the LDS and launches of tf_attn_step_split / tf_attn_extend_split, the eligibility rule, and the checks of flope_tf_stream_attention
// (tests/host_harness/harness_tf_split.cpp, tests/test_tf_step_split_host.py).
// Below those, option extend_mfma: which 64-key blocks a workgroup of tf_attn16_extend loads, where key j of a block comes
// from (zeros, a cache row, a chunk row), the output row of a query, the launch, the eligibility rule, and the checks of
// flope_tf_stream_attention_extend (tests/host_harness/harness_tf_extend16.cpp, tests/test_tf_extend_mfma_host.py).
// Below those, a state with a distance table (flope_tf_stream_open_bias): how many distances a state needs, the planes
// check, the first non-finite entry, the entry a visible key reads and the test the biased kernels make in front of their first load
// (tests/host_harness/harness_tf_stream_bias.cpp, tests/test_tf_stream_bias_host.py).
#pragma once

#include <limits.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "tf_attn_plan.h"

namespace flope_tf_plan {

// tf_attn_step: one wave per (row, head), four waves per workgroup; a wave's score row holds the keys 0 .. pos of its track, and a
// launch sizes every row for the largest position of the call
constexpr int kTfStepWaves = 4;
constexpr size_t kTfStepLdsMax = 64 * 1024;          // what a launch gets without asking for more
constexpr size_t tf_step_lds(int max_pos) { return (size_t)kTfStepWaves * ((size_t)max_pos + 1) * sizeof(float); }
// the largest capacity whose last position (capacity - 1) still fits: 4096
constexpr int kTfStreamMaxCapacity = (int)(kTfStepLdsMax / (kTfStepWaves * sizeof(float)));
static_assert(tf_step_lds(kTfStreamMaxCapacity - 1) <= kTfStepLdsMax && tf_step_lds(kTfStreamMaxCapacity) > kTfStepLdsMax,
              "kTfStreamMaxCapacity is the largest capacity whose score rows fit");
static_assert(kTfStreamMaxCapacity >= 4096, "a track holds at least 4096 tokens");

struct TfStreamLaunch { unsigned grid_x, block; size_t lds; };
// n rows of H heads at positions <= max_pos
inline TfStreamLaunch tf_step_launch(int n, int H, int max_pos) {
  return {(unsigned)(((long long)n * H + kTfStepWaves - 1) / kTfStepWaves), 64u * kTfStepWaves, tf_step_lds(max_pos)};
}
// tf_cache_append (the prefill's copy and the extend's append): one thread per unit (a 16-byte vector or one element) of the k | v
// columns of the n x max_len rows a ragged batch may hold; units: those of the 2 model_dim columns of a cache row
inline TfStreamLaunch tf_cache_fill_launch(int n, int max_len, int units) {
  const size_t total = (size_t)n * max_len * units;
  return {(unsigned)((total + 255) / 256), 256u, 0};
}
// elements per 16-byte vector of a cache of esz-byte elements, and whether a head slice (tf_attn_step) or the k | v columns
// (tf_cache_append) of a row move as whole vectors: the cache and the handle's qkv buffer are 16-byte aligned, rows are 2 and 3
// model_dim elements, so what has to divide is the first column of the slice and its width
constexpr int tf_stream_vec(int esz) { return 16 / esz; }
constexpr bool tf_step_vec_ok(int head_dim, int esz) { return head_dim % tf_stream_vec(esz) == 0; }
constexpr bool tf_cache_fill_vec_ok(int model_dim, int esz) { return model_dim % tf_stream_vec(esz) == 0; }

enum {
  kTfStreamOk = 0,
  kTfStreamCount = -1,      // n < 1, n > the limit, or a NULL track list with n != tracks
  kTfStreamRange = -2,      // rows[*bad] is no track
  kTfStreamDuplicate = -3,  // rows[*bad] names a track an earlier row named
  kTfStreamFull = -4,       // step: the track of row *bad already holds capacity tokens
  kTfStreamLength = -5,     // prefill: lengths[*bad] > capacity
  kTfStreamOpen = -6        // open: tracks < 1 or capacity outside 1 .. kTfStreamMaxCapacity
};

inline int tf_stream_check_open(int tracks, int capacity) {
  return tracks >= 1 && capacity >= 1 && capacity <= kTfStreamMaxCapacity ? kTfStreamOk : kTfStreamOpen;
}

// The track of row r: rows[r], or r with a NULL list
inline int tf_stream_track(const int* rows, int r) { return rows ? rows[r] : r; }

// n rows name n distinct tracks of `tracks`; rows == NULL: n == tracks and row r is track r.  seen: scratch of `tracks` bytes.
inline int tf_stream_check_rows(int tracks, int limit, int n, const int* rows, char* seen, int* bad) {
  if (n < 1 || n > limit || n > tracks) return kTfStreamCount;
  if (!rows) return n == tracks ? kTfStreamOk : kTfStreamCount;
  memset(seen, 0, (size_t)tracks);
  for (int r = 0; r < n; ++r) {
    if (rows[r] < 0 || rows[r] >= tracks) { *bad = r; return kTfStreamRange; }
    if (seen[rows[r]]) { *bad = r; return kTfStreamDuplicate; }
    seen[rows[r]] = 1;
  }
  return kTfStreamOk;
}

// step: 1 <= n <= min(tracks, max_tokens), distinct tracks in range, none at capacity.  *max_pos: the largest position of the call
// (the position a row's token takes is what its track holds).  Writes nothing but *bad / *max_pos and the scratch.
inline int tf_stream_check_step(const int* pos, int tracks, int capacity, int max_tokens, int n, const int* rows, char* seen, int* bad,
                                int* max_pos) {
  const int rc = tf_stream_check_rows(tracks, max_tokens, n, rows, seen, bad);
  if (rc) return rc;
  int mx = 0;
  for (int r = 0; r < n; ++r) {
    const int p = pos[tf_stream_track(rows, r)];
    if (p >= capacity) { *bad = r; return kTfStreamFull; }
    if (p > mx) mx = p;
  }
  *max_pos = mx;
  return kTfStreamOk;
}
// ... its device table, (track, position) per row -- an extend's too, (track, pos0) per sequence -- and the positions behind it
inline void tf_stream_step_table(const int* pos, int n, const int* rows, int* tab) {
  for (int r = 0; r < n; ++r) { tab[2 * r] = tf_stream_track(rows, r); tab[2 * r + 1] = pos[tf_stream_track(rows, r)]; }
}
inline void tf_stream_advance(int* pos, int n, const int* rows) {
  for (int r = 0; r < n; ++r) ++pos[tf_stream_track(rows, r)];
}

// prefill: n sequences for n distinct tracks, every length (seq_len with a NULL list) within capacity; the limits of the ragged
// forward itself (tf_varlen_plan) are checked by the caller in front of this
inline int tf_stream_check_prefill(int tracks, int capacity, int n, int seq_len, const int* lengths, const int* rows, char* seen, int* bad) {
  const int rc = tf_stream_check_rows(tracks, tracks, n, rows, seen, bad);
  if (rc) return rc;
  for (int b = 0; b < n; ++b)
    if ((lengths ? lengths[b] : seq_len) > capacity) { *bad = b; return kTfStreamLength; }
  return kTfStreamOk;
}
inline void tf_stream_set_lengths(int* pos, int n, int seq_len, const int* lengths, const int* rows) {
  for (int b = 0; b < n; ++b) pos[tf_stream_track(rows, b)] = lengths ? lengths[b] : seq_len;
}

// reset: rows == NULL: every track (n is ignored); otherwise n >= 1 tracks in range.  A track named twice is reset once: harmless.
inline int tf_stream_check_reset(int tracks, int n, const int* rows, int* bad) {
  if (!rows) return kTfStreamOk;
  if (n < 1) return kTfStreamCount;
  for (int r = 0; r < n; ++r)
    if (rows[r] < 0 || rows[r] >= tracks) { *bad = r; return kTfStreamRange; }
  return kTfStreamOk;
}

// ---- a windowed state: sliding-window causal attention over a ring cache -------------------------------------------
// The cache keeps its shape [tracks][capacity][2 d]; the token at absolute position p lives in row p % capacity, and a step at
// position p attends to keys tf_window_lo(p, W) .. p, W <= capacity.  Positions are absolute and never wrap: a track is full only at
// INT_MAX tokens.
constexpr int tf_stream_slot(int p, int capacity) { return p % capacity; }

// The pos - lo cached keys of a step are nk consecutive ring rows from slo = lo % capacity on; they wrap at most once (nk < W <=
// capacity), so tf_attn_stream_row's value pass walks two contiguous runs: tf_stream_run0 rows from slo, the rest from row 0
constexpr int tf_stream_run0(int slo, int nk, int capacity) { return nk < capacity - slo ? nk : capacity - slo; }

inline int tf_stream_check_open_window(int tracks, int capacity, int window) {
  return tf_stream_check_open(tracks, capacity) == kTfStreamOk && window >= 1 && window <= capacity ? kTfStreamOk : kTfStreamOpen;
}

// step: as tf_stream_check_step, with kTfStreamFull only for a track that holds INT_MAX tokens.  *max_pos: the largest visible key
// count of the call - 1, min(p, W - 1) over its rows; tf_step_launch(n, H, *max_pos) sizes the score rows, *max_pos + 1 is smax.
inline int tf_stream_check_step_window(const int* pos, int tracks, int window, int max_tokens, int n, const int* rows, char* seen, int* bad,
                                       int* max_pos) {
  const int rc = tf_stream_check_rows(tracks, max_tokens, n, rows, seen, bad);
  if (rc) return rc;
  int mx = 0;
  for (int r = 0; r < n; ++r) {
    const int p = pos[tf_stream_track(rows, r)];
    if (p == INT_MAX) { *bad = r; return kTfStreamFull; }
    const int vis = tf_window_keys(p, window) - 1;
    if (vis > mx) mx = vis;
  }
  *max_pos = mx;
  return kTfStreamOk;
}

// prefill: n sequences for n distinct tracks; a length is limited by the ragged forward alone (tf_varlen_plan, checked by the caller
// in front of this), not by capacity: the ring keeps the last min(len, capacity) tokens, which hold every key a later step sees
inline int tf_stream_check_prefill_window(int tracks, int n, const int* rows, char* seen, int* bad) {
  return tf_stream_check_rows(tracks, tracks, n, rows, seen, bad);
}
// ... and which tokens tf_cache_append writes into a ring (tf_stream_append_writes below is this function): token i of len only if no later token of the sequence takes its row -- the
// last min(len, capacity) -- so every row is written at most once (where they go: tf_stream_append_slot below)
constexpr bool tf_stream_fill_writes(int i, int len, int capacity) { return i >= 0 && i < len && i >= len - capacity; }

// ---- extend: several tokens per track in one call, behind what the track holds ----------------------------------------
// Sequence b of the call is the next len tokens of its track, which holds pos0: the token at chunk row i takes position p = pos0 + i
// and attends to keys lo .. p, lo = tf_window_lo(p, W) (W = 0: a linear state, lo = 0).  Keys lo .. pos0 - 1 lie in the cache (rows j,
// or j % capacity of a ring), keys max(lo, pos0) .. p in the chunk's own packed qkv rows -- the query's own key among them.
// How many of query p's keys are cached ones, and the chunk row of its first key that is not
constexpr int tf_extend_cached(int pos0, int lo) { return lo < pos0 ? pos0 - lo : 0; }
constexpr int tf_extend_chunk0(int pos0, int lo) { return lo > pos0 ? lo - pos0 : 0; }
// ... and the largest visible key count of a sequence (its last query's), which sizes the score rows: tf_step_lds(smax - 1) bytes
constexpr int tf_extend_keys(int pos0, int len, int W) { return tf_window_keys(pos0 + len - 1, W); }

// tf_attn_extend: workgroup (sequence b, head h) x a slice of the queries, one query per wave and trip -- grid (n H, min(ceil(max_len
// / 4), 64)), so the four waves of a workgroup walk the same cache rows
constexpr int kTfExtendGridY = 64;
struct TfExtendLaunch { unsigned grid_x, grid_y, block; size_t lds; };
inline TfExtendLaunch tf_extend_launch(int n, int H, int max_len, int smax) {
  const int gy = (max_len + kTfStepWaves - 1) / kTfStepWaves;
  return {(unsigned)n * (unsigned)H, (unsigned)(gy < kTfExtendGridY ? gy : kTfExtendGridY), 64u * kTfStepWaves, tf_step_lds(smax - 1)};
}
// The append: the prefill's copy by its other name, and the same tokens
inline TfStreamLaunch tf_cache_append_launch(int n, int max_len, int units) { return tf_cache_fill_launch(n, max_len, units); }
constexpr bool tf_stream_append_writes(int i, int len, int capacity) { return tf_stream_fill_writes(i, len, capacity); }
// Where the tokens tf_stream_append_writes names go: token i of a chunk at pos0 to row
// (pos0 + i) % capacity; pos0 = 0 is the prefill.  A linear state writes every token, to row pos0 + i (the check below keeps that
// below capacity, where the two rules are one).
// THE APPEND RUNS BEHIND THE LAYER'S ATTENTION, never in front of it as the prefill's fill does: on a ring the chunk's token at p takes
// the row of key p - capacity, and query q < p of the same chunk still sees that key when p - capacity >= tf_window_lo(q, W) -- with
// q = pos0 and p = pos0 + len - 1 that is len >= capacity - W + 2, every chunk of two tokens at capacity == W.
constexpr int tf_stream_append_slot(int pos0, int i, int capacity) { return tf_stream_slot(pos0 + i, capacity); }

enum {
  kTfStreamRoom = -7        // extend, linear state: the track of sequence *bad holds pos and pos + lengths[*bad] > capacity
};

// extend: n sequences for n distinct tracks (tf_stream_check_rows as for prefill); lengths are 1 .. seq_len and sum to <= max_tokens
// by tf_varlen_plan, which the caller runs in front of this.  window = 0: every track has room for its chunk (kTfStreamRoom
// otherwise); a windowed state: pos + len stays an int (kTfStreamFull otherwise) -- a chunk may be longer than the capacity.
// *smax: the call's largest visible key count.  Writes nothing but *bad / *smax and the scratch.
inline int tf_stream_check_extend(const int* pos, int tracks, int capacity, int window, int n, const int* lengths, const int* rows, char* seen,
                                  int* bad, int* smax) {
  const int rc = tf_stream_check_rows(tracks, tracks, n, rows, seen, bad);
  if (rc) return rc;
  int mx = 0;
  for (int b = 0; b < n; ++b) {
    const int p = pos[tf_stream_track(rows, b)], len = lengths[b];
    if (window) { if (p > INT_MAX - len) { *bad = b; return kTfStreamFull; } }
    else if (p > capacity - len) { *bad = b; return kTfStreamRoom; }
    const int vis = tf_extend_keys(p, len, window);
    if (vis > mx) mx = vis;
  }
  *smax = mx;
  return kTfStreamOk;
}
// ... its device table is tf_stream_step_table's, (track, pos0) per sequence; the positions behind it
inline void tf_stream_extend_table(const int* pos, int n, const int* rows, int* tab) { tf_stream_step_table(pos, n, rows, tab); }
inline void tf_stream_extend_advance(int* pos, int n, const int* lengths, const int* rows) {
  for (int b = 0; b < n; ++b) pos[tf_stream_track(rows, b)] += lengths[b];
}

// ---- step_split: a token's visible keys split over the four waves of a workgroup (option "step_split") -----------------
// The visible key with index k, counted from the first visible key lo (k = 0 .. L - 1, the token's own key is k = L - 1), lies in block
// k / kTfSplitBlock; block b belongs to wave b % kTfSplitWaves, a wave walks its blocks in ascending order, and lane l of the wave scores
// key kTfSplitBlock b + l.  Counting from lo, not from the absolute position, is what makes a ring's capacity and the cached / chunk
// boundary of an extend invisible to the arithmetic.  tf_attn_split_row is built from these, and so is
// tests/host_harness/harness_tf_split.cpp (tests/test_tf_step_split_host.py holds them against brute force).
constexpr int kTfSplitWaves = 4;
constexpr int kTfSplitBlock = 64;
constexpr int tf_split_block(int k) { return k / kTfSplitBlock; }
constexpr int tf_split_lane(int k) { return k % kTfSplitBlock; }
constexpr int tf_split_wave(int block) { return block % kTfSplitWaves; }
// blocks of L visible keys, and how many of them wave w walks: blocks w, w + 4, .. (0: the wave has no part in the merge, by this rule)
constexpr int tf_split_blocks(int L) { return (L + kTfSplitBlock - 1) / kTfSplitBlock; }
constexpr int tf_split_wave_blocks(int L, int wave) { return (tf_split_blocks(L) - wave + kTfSplitWaves - 1) / kTfSplitWaves; }
// The value pass: a head slice is tf_split_lanes 16-byte vectors, one per lane; the wave's 64 lanes form 64 / tf_split_lanes groups,
// group g = lane / tf_split_lanes takes the block's keys g, g + groups, .. -- every lane loads
constexpr int tf_split_lanes(int head_dim, int esz) { return head_dim / tf_stream_vec(esz); }
// The rule: the head slice moves as whole 16-byte vectors (tf_step_vec_ok) and their count is a power of two <= 64
constexpr bool tf_step_split_ok(int head_dim, int esz) {
  return head_dim > 0 && tf_step_vec_ok(head_dim, esz) && tf_split_lanes(head_dim, esz) <= 64 &&
         (tf_split_lanes(head_dim, esz) & (tf_split_lanes(head_dim, esz) - 1)) == 0;
}
// LDS of a workgroup: per wave one block's probabilities, then the partial state m, l, o[head_dim].  No position, no smax.
constexpr size_t tf_split_lds(int head_dim) { return (size_t)kTfSplitWaves * (kTfSplitBlock + 2 + (size_t)head_dim) * sizeof(float); }
// tf_attn_step_split: one workgroup per (row, head)
inline TfStreamLaunch tf_step_split_launch(int n, int H, int head_dim) {
  return {(unsigned)n * (unsigned)H, 64u * kTfSplitWaves, tf_split_lds(head_dim)};
}
// tf_attn_extend_split: workgroup (sequence b, head h) x blockIdx.y takes queries blockIdx.y, blockIdx.y + grid_y, .. of the sequence
constexpr int kTfSplitGridY = 256;
inline TfExtendLaunch tf_extend_split_launch(int n, int H, int max_len, int head_dim) {
  return {(unsigned)n * (unsigned)H, (unsigned)(max_len < kTfSplitGridY ? max_len : kTfSplitGridY), 64u * kTfSplitWaves, tf_split_lds(head_dim)};
}
// Where visible key k of a query lies: the first nc keys are cached ones, cache row k (a ring: (slo + k) % capacity, slo = lo %
// capacity -- they wrap at most once), the others rows k - nc, .. behind the first own row (step: the token's qkv row; extend: chunk
// row tf_extend_chunk0 onwards)
constexpr int tf_split_cache_row(int k, int slo, int capacity) { return slo + k >= capacity ? slo + k - capacity : slo + k; }

// flope_tf_stream_attention: n sequences of a padded [n][seq_len] batch for tracks 0 .. n - 1; a length is 1 .. seq_len and, on a linear
// state (window = 0), at most capacity.  *max_pos: the largest visible key count - 1, as the step checks give it.
inline int tf_stream_check_attention(int tracks, int capacity, int window, int max_tokens, int n, int seq_len, const int* lengths, int* bad,
                                     int* max_pos) {
  if (n < 1 || n > tracks || n > max_tokens || seq_len < 1) return kTfStreamCount;
  int mx = 0;
  for (int b = 0; b < n; ++b) {
    const int len = lengths ? lengths[b] : seq_len;
    if (len < 1 || len > seq_len || (!window && len > capacity)) { *bad = b; return kTfStreamLength; }
    const int vis = tf_window_keys(len - 1, window) - 1;
    if (vis > mx) mx = vis;
  }
  *max_pos = mx;
  return kTfStreamOk;
}

// ---- extend_mfma: extend's attention on the 16-bit MFMA step (option "extend_mfma") -------------------------------------
// tf_attn16_extend: workgroup (sequence b, head h, query block y) takes chunk rows 128 y .. 128 y + 127 of its sequence, wave w the 32
// from 128 y + 32 w on; the query at chunk row i has the absolute position pos0 + i, and the wave's first query q0 = pos0 + 128 y + 32 w
// is NOT a multiple of 32.  Keys are walked in ABSOLUTE 64-key blocks (block t = keys 64 t .. 64 t + 63, two 32-key steps), the blocks
// and steps of tf_attn_tiled on the whole track: tf_causal_step_taken / tf_window_step_taken decide per wave, for any q0.
// A 16-bit dtype, a head_dim tf_attn_tiled has (32 / 64 / 96 / 128), and head slices that start on 16 bytes in a qkv row (3 model_dim
// elements) and in a cache row (2 model_dim elements)
inline bool tf_extend_mfma_ok(int dtype, int head_dim, int model_dim) {
  return (dtype == FLOPE_DT_F16 || dtype == FLOPE_DT_BF16) && tf_attn_tiled_ok(head_dim) && head_dim % 8 == 0 && model_dim > 0 && model_dim % 8 == 0;
}
// Positions the kernel's int arithmetic is written for: a wave's q0 + 31 and the block one behind the last stay ints while
// pos0 + len <= kTfExtendMfmaPosMax.  A call that passes it keeps the other kernels (tf_extend_mfma_positions_ok), and the kernel
// itself exits there.
constexpr int kTfExtendMfmaPosMax = INT_MAX - 2 * kTfAttnTiledQueries;
constexpr bool tf_extend_mfma_positions_ok(int pos0, int len) { return pos0 >= 0 && len >= 1 && pos0 <= kTfExtendMfmaPosMax - len; }
// the chunk rows of query block y, and whether it has any
constexpr bool tf_extend_mfma_block_live(int len, int y) { return y >= 0 && y < (len + kTfAttnTiledQueries - 1) / kTfAttnTiledQueries; }
// lo_wg: the first key any query of the workgroup sees -- its first query's (W = 0: key 0)
constexpr int tf_extend_mfma_lo(int pos0, int y, int W) { return tf_window_lo(pos0 + kTfAttnTiledQueries * y, W); }
// first and last 64-key block the workgroup loads: the one that holds lo_wg .. the one that holds its last query
constexpr int tf_extend_mfma_first_block(int pos0, int y, int W) { return tf_extend_mfma_lo(pos0, y, W) / kTfAttnTiledKB; }
constexpr int tf_extend_mfma_last_query(int pos0, int len, int y) {
  return pos0 + (kTfAttnTiledQueries * y + kTfAttnTiledQueries - 1 < len - 1 ? kTfAttnTiledQueries * y + kTfAttnTiledQueries - 1 : len - 1);
}
constexpr int tf_extend_mfma_last_block(int pos0, int len, int y) { return tf_extend_mfma_last_query(pos0, len, y) / kTfAttnTiledKB; }
// a wave's first absolute query
constexpr int tf_extend_mfma_q0(int pos0, int y, int wave) { return pos0 + kTfAttnTiledQueries * y + 32 * wave; }
// whether that wave takes the 32-key step that starts at key kb (a multiple of 32) of a sequence that ends at Labs = pos0 + len
constexpr bool tf_extend_mfma_step_taken(int q0, int kb, int Labs, int W) {
  return kb < Labs && (W > 0 ? tf_window_step_taken(q0, kb, W) : tf_causal_step_taken(q0, kb));
}
// Where the LDS row of key j comes from, for the workgroup y of a chunk (pos0, len):
//   j >= pos0 + len or j < lo_wg    zeros (never the contents of a row that holds no visible key: 0 x NaN is NaN in the PV product)
//   pos0 <= j                       the chunk's packed qkv row j - pos0 -- the token's own key among them, never its cache slot
//   lo_wg <= j < pos0               cache row j of the track, row j % capacity of a ring (lo_wg > pos0 - capacity: the ring holds it)
enum { kTfExtendKeyZero = 0, kTfExtendKeyCache = 1, kTfExtendKeyChunk = 2 };
struct TfExtendKey { int kind, row; };
constexpr TfExtendKey tf_extend_mfma_key(int j, int pos0, int len, int capacity, int W, int y) {
  if (j < tf_extend_mfma_lo(pos0, y, W) || j >= pos0 + len) return {kTfExtendKeyZero, 0};
  if (j >= pos0) return {kTfExtendKeyChunk, j - pos0};
  return {kTfExtendKeyCache, W > 0 ? tf_stream_slot(j, capacity) : j};
}
// the packed row of att the query at absolute position qi of sequence b (first packed row off_b) is stored to
constexpr long long tf_extend_mfma_out_row(int off_b, int pos0, int qi) { return (long long)off_b + (qi - pos0); }
// grid (n H, ceil(max_len / 128)), 256 threads, tf_attn_tiled's ring of two stages
inline TfExtendLaunch tf_extend_mfma_launch(int n, int H, int max_len, int head_dim) {
  return {(unsigned)n * (unsigned)H, (unsigned)((max_len + kTfAttnTiledQueries - 1) / kTfAttnTiledQueries), 256u, tf_attn_tiled_lds(head_dim)};
}

// flope_tf_stream_attention_extend: n sequences of a padded [n][seq_len] batch for tracks 0 .. n - 1; rows 0 .. cached[b] - 1 are the
// track's history, rows cached[b] .. lengths[b] - 1 the chunk.  A length is 1 .. seq_len and, on a linear state, at most capacity;
// cached[b] is 0 .. lengths[b] - 1; the chunks together are at most max_tokens rows.  *smax: the call's largest visible key count,
// *max_len the longest chunk, *total the chunks' rows.  kTfStreamCached names a cached[] outside its range, kTfStreamTokens the sum.
enum { kTfStreamCached = -8, kTfStreamTokens = -9 };
inline int tf_stream_check_attention_extend(int tracks, int capacity, int window, int max_tokens, int n, int seq_len, const int* lengths,
                                            const int* cached, int* bad, int* smax, int* max_len, int* total) {
  if (n < 1 || n > tracks || n > max_tokens || seq_len < 1 || !lengths || !cached) return kTfStreamCount;
  int mx = 0, ml = 0;
  long long sum = 0;
  for (int b = 0; b < n; ++b) {
    const int len = lengths[b];
    if (len < 1 || len > seq_len || (!window && len > capacity)) { *bad = b; return kTfStreamLength; }
    if (cached[b] < 0 || cached[b] > len - 1) { *bad = b; return kTfStreamCached; }
    const int vis = tf_extend_keys(cached[b], len - cached[b], window);
    if (vis > mx) mx = vis;
    if (len - cached[b] > ml) ml = len - cached[b];
    sum += len - cached[b];
  }
  if (sum > (long long)max_tokens) return kTfStreamTokens;
  *smax = mx; *max_len = ml; *total = (int)sum;
  return kTfStreamOk;
}

// ---- a distance table: a relative attention bias on a stream state (flope_tf_stream_open_bias) --------------------------
// rel: float32 [planes][D], planes = 1 (every head) or num_heads.  The query at position p scores key j (lo <= j <= p) as
// fl(fl(chain * scale) + rel[plane][p - j]).  A query never sees more than `capacity` keys of a linear state or W of a windowed one, so
// that is how many distances the table must hold -- exactly: a table of another length was made for another state.
constexpr int tf_stream_bias_distances(int capacity, int window) { return window ? window : capacity; }
constexpr bool tf_stream_bias_planes_ok(int planes, int H) { return planes == 1 || (H >= 1 && planes == H); }
// The entry of the visible key with index j counted from lo (as the score row counts, j = 0 .. L - 1; the query's own key is L - 1):
// its distance p - (lo + j) = L - 1 - j
constexpr int tf_stream_bias_index(int L, int j) { return L - 1 - j; }
// What tf_attn_step / tf_attn_extend test beside smax before their first load: `keys` visible keys index a table of D distances
constexpr bool tf_stream_bias_keys_ok(int keys, int D) { return keys <= D; }
// The first entry that is not finite, in (plane, distance) order: -inf is no way to mask here (visibility stays with the window), so
// every non-finite value counts.  By bits: the test holds under any floating-point option of the compiler.
inline bool tf_stream_bias_nonfinite(const float* rel, int planes, int D, int* plane, int* dist) {
  for (int h = 0; h < planes; ++h)
    for (int t = 0; t < D; ++t) {
      uint32_t u;
      memcpy(&u, rel + (size_t)h * D + t, sizeof(u));
      if ((u & 0x7f800000u) == 0x7f800000u) { *plane = h; *dist = t; return true; }
    }
  return false;
}
// open: the refusals of a table in the order the call makes them.  *bad_plane / *bad_dist: the entry kTfStreamBiasValue names
enum {
  kTfStreamBiasPlanes = -10,      // planes is neither 1 nor num_heads
  kTfStreamBiasDistances = -11,   // distances != tf_stream_bias_distances(capacity, window)
  kTfStreamBiasNull = -12,        // no table
  kTfStreamBiasValue = -13        // rel[*bad_plane][*bad_dist] is NaN or +-inf
};
inline int tf_stream_check_open_bias(int capacity, int window, int H, int planes, int distances, const float* rel, int* bad_plane, int* bad_dist) {
  if (!tf_stream_bias_planes_ok(planes, H)) return kTfStreamBiasPlanes;
  if (distances != tf_stream_bias_distances(capacity, window)) return kTfStreamBiasDistances;
  if (!rel) return kTfStreamBiasNull;
  return tf_stream_bias_nonfinite(rel, planes, distances, bad_plane, bad_dist) ? (int)kTfStreamBiasValue : (int)kTfStreamOk;
}
constexpr size_t tf_stream_bias_bytes(int planes, int D) { return (size_t)planes * (size_t)D * sizeof(float); }

}  // namespace flope_tf_plan
