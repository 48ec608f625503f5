// A compiled [L, L] attention mask (flope_tf_mask_*): the set of (query i, key j) pairs that may attend, as bits, and
// what the host derives from them -- plain integer arithmetic, no HIP, shared by tf_encoder.hip (flope_tf_mask_create and the masked
// entry points) and tests/host_harness/harness_tf_mask.cpp (tests/test_tf_mask_host.py holds every function against brute force).
// Layout: uint32 words [L][tf_mask_words(L)], bit j % 32 of word j / 32 of row i set = query i may attend to key j; the padding bits
// (columns L .. 32 * words - 1) are zero.  first[i] / last[i]: the first and last allowed key of row i; a row without a key has
// first = L and last = -1.  Below them the mask's tile map for option mask_mfma: which 64-key blocks a 128-row query block
// loads and which 32-key steps a wave takes, tf_attn_pick_masked and the launch of tf_attn_tiled_masked
// (tests/host_harness/harness_tf_mask16.cpp, tests/test_tf_mask16_host.py).  At the end the host side of a compiled additive bias
// (flope_tf_bias_create): float32 planes [planes][L][L], -inf = masked, from which the same bit words are derived, and the
// two validators a bias adds (tests/host_harness/harness_tf_bias.cpp, tests/test_tf_bias_host.py).
#pragma once

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "tf_attn_plan.h"

namespace flope_tf_plan {

constexpr int tf_mask_words(int L) { return (L + 31) / 32; }
inline bool tf_mask_bit(const uint32_t* bits, int L, int i, int j) { return (bits[(size_t)i * tf_mask_words(L) + (j >> 5)] >> (j & 31)) & 1u; }

// allow: row-major [L][L], non-zero = allowed -> bits [L][tf_mask_words(L)], padding bits zero
inline void tf_mask_pack(const unsigned char* allow, int L, uint32_t* bits) {
  const int nw = tf_mask_words(L);
  for (int i = 0; i < L; ++i)
    for (int w = 0; w < nw; ++w) {
      uint32_t m = 0;
      for (int j = w * 32; j < L && j < w * 32 + 32; ++j)
        if (allow[(size_t)i * L + j]) m |= 1u << (j & 31);
      bits[(size_t)i * nw + w] = m;
    }
}

inline int tf_mask_ctz(uint32_t m) { int n = 0; while (!(m & 1u)) { m >>= 1; ++n; } return n; }
inline int tf_mask_popc(uint32_t m) { int n = 0; for (; m; m &= m - 1) ++n; return n; }

// first[i], last[i] of every row (L, -1 for a row without a key); only the columns below L are looked at
inline void tf_mask_first_last(const uint32_t* bits, int L, int* first, int* last) {
  const int nw = tf_mask_words(L);
  for (int i = 0; i < L; ++i) {
    first[i] = L;
    last[i] = -1;
    for (int w = 0; w < nw; ++w) {
      uint32_t m = bits[(size_t)i * nw + w];
      if (w == nw - 1 && (L & 31)) m &= (1u << (L & 31)) - 1u;
      if (!m) continue;
      if (first[i] == L) first[i] = w * 32 + tf_mask_ctz(m);
      int hi = 31;
      while (!((m >> hi) & 1u)) --hi;
      last[i] = w * 32 + hi;
    }
  }
}

// The first row without an allowed key, -1: none
inline int tf_mask_empty_row(const uint32_t* bits, int L) {
  const int nw = tf_mask_words(L);
  for (int i = 0; i < L; ++i) {
    uint32_t any = 0;
    for (int w = 0; w < nw; ++w) {
      uint32_t m = bits[(size_t)i * nw + w];
      if (w == nw - 1 && (L & 31)) m &= (1u << (L & 31)) - 1u;
      any |= m;
    }
    if (!any) return i;
  }
  return -1;
}

// The first set padding bit in row order: its column (>= L) with *row written, -1: none
inline int tf_mask_padding_bit(const uint32_t* bits, int L, int* row) {
  if (!(L & 31)) return -1;
  const int nw = tf_mask_words(L);
  for (int i = 0; i < L; ++i) {
    const uint32_t m = bits[(size_t)i * nw + nw - 1] & ~((1u << (L & 31)) - 1u);
    if (m) {
      if (row) *row = i;
      return (nw - 1) * 32 + tf_mask_ctz(m);
    }
  }
  return -1;
}

// A sequence of n <= L tokens is encoded under the top-left n x n corner: the first row i < n with no allowed key below n, -1: none.
// Row i has a key below n exactly when first[i] < n.
inline int tf_mask_length_row(const int* first, int L, int n) {
  for (int i = 0; i < n && i < L; ++i)
    if (first[i] >= n) return i;
  return -1;
}

// Allowed pairs of the n x n corner (n = L: of the whole mask)
inline long long tf_mask_pairs_len(const uint32_t* bits, int L, int n) {
  const int nw = tf_mask_words(L);
  if (n > L) n = L;
  long long cnt = 0;
  for (int i = 0; i < n; ++i)
    for (int w = 0; w * 32 < n; ++w) {
      uint32_t m = bits[(size_t)i * nw + w];
      if (n - w * 32 < 32) m &= (1u << (n - w * 32)) - 1u;
      cnt += tf_mask_popc(m);
    }
  return cnt;
}
inline long long tf_mask_pairs(const uint32_t* bits, int L) { return tf_mask_pairs_len(bits, L, L); }

// Grid, block and LDS of tf_attn_masked: launched as the generic kernel always is (tf_attn_varlen_launch's default case, sized by the
// longest sequence max_len <= L), its LDS the four score rows [4][max_len] floats and behind them the four waves' mask rows
// [4][tf_mask_words(L)] words.
inline size_t tf_mask_lds_words_at(int max_len) { return (size_t)4 * max_len; }      // in 4-byte units: where the mask rows start
inline TfAttnLaunch tf_mask_launch(int head_dim, int B, int H, int max_len, int L) {
  TfAttnLaunch l = tf_attn_varlen_launch(FLOPE_TF_ATTN_GENERIC, head_dim, B, H, max_len);
  l.lds = (tf_mask_lds_words_at(max_len) + (size_t)4 * tf_mask_words(L)) * 4;
  return l;
}

// ---- the tile map of a mask (option "mask_mfma") ------------------------------------------------------------------------
// tf_attn_tiled_masked walks a mask in the units of tf_attn_tiled: query blocks of kTfAttnTiledQueries = 128 rows (four waves of 32),
// key blocks of kTfAttnTiledKB = 64 keys (two 32-key steps).  Query block qb owns the ascending list of the key blocks that hold at
// least one allowed pair with one of its rows, entries start[qb] .. start[qb + 1] - 1 (CSR; nqb = tf_mask_query_blocks(L) lists, every
// one non-empty: every row has a key).  An entry is 16 bytes:
//   kblock      the key block: keys 64 kblock .. 64 kblock + 63
//   colany      bit r: key 64 kblock + r is allowed by some row of the query block (lo: r < 32, hi: r - 32)
//   cls         two bits per (wave w = 0 .. 3, step s = 0 .. 1) at bit 2 (2 w + s): the tile of rows 128 qb + 32 w .. + 31 below L and keys
//               64 kblock + 32 s .. + 31 below L holds no allowed pair (kTfMaskNone; also a tile without a row or a key below L), some
//               (kTfMaskSome) or only allowed pairs (kTfMaskAll)
// A sequence of n < L tokens is encoded under the n x n corner: its query blocks are the first ceil(n / 128), of each list the entries
// with 64 kblock < n, a prefix (tf_mask_tiles_corner).  The classes stay those of the whole mask: "none" and "all" stay true of the
// corner, "some" may have become either, which costs a word load or a step over nothing and no bit.
struct TfMaskTile { int32_t kblock; uint32_t colany_lo, colany_hi, cls; };
static_assert(sizeof(TfMaskTile) == 16, "an entry is one 16-byte load");
enum { kTfMaskNone = 0, kTfMaskSome = 1, kTfMaskAll = 2 };

constexpr int tf_mask_query_blocks(int L) { return (L + kTfAttnTiledQueries - 1) / kTfAttnTiledQueries; }
constexpr int tf_mask_key_blocks(int L) { return (L + kTfAttnTiledKB - 1) / kTfAttnTiledKB; }
constexpr int tf_mask_tile_class(uint32_t cls, int wave, int step) { return (int)((cls >> (2 * (2 * wave + step))) & 3u); }

// The entry of (qb, kblock) into *t; false: the block holds no allowed pair with a row of qb and is not listed
inline bool tf_mask_tile_of(const uint32_t* bits, int L, int qb, int kblock, TfMaskTile* t) {
  const int nw = tf_mask_words(L);
  t->kblock = kblock; t->colany_lo = t->colany_hi = t->cls = 0;
  for (int w = 0; w < kTfAttnTiledQueries / 32; ++w)
    for (int s = 0; s < kTfAttnTiledKB / 32; ++s) {
      const int word = 2 * kblock + s, r0 = qb * kTfAttnTiledQueries + 32 * w;
      if (word >= nw || r0 >= L) continue;                                   // no key or no row below L: none
      const uint32_t valid = word == nw - 1 && (L & 31) ? (1u << (L & 31)) - 1u : ~0u;
      uint32_t any = 0, all = ~0u;
      for (int r = r0; r < r0 + 32 && r < L; ++r) { const uint32_t m = bits[(size_t)r * nw + word] & valid; any |= m; all &= m; }
      (s ? t->colany_hi : t->colany_lo) |= any;
      t->cls |= (uint32_t)(!any ? kTfMaskNone : all == valid ? kTfMaskAll : kTfMaskSome) << (2 * (2 * w + s));
    }
  return (t->colany_lo | t->colany_hi) != 0;
}

// start: nqb + 1 ints, written always; tiles: the entries, or NULL to count them.  Returns start[nqb], the number of entries.
inline long long tf_mask_tiles_build(const uint32_t* bits, int L, int* start, TfMaskTile* tiles) {
  const int nqb = tf_mask_query_blocks(L), nkb = tf_mask_key_blocks(L);
  int n = 0;
  for (int qb = 0; qb < nqb; ++qb) {
    start[qb] = n;
    for (int kblock = 0; kblock < nkb; ++kblock) {
      TfMaskTile t;
      if (!tf_mask_tile_of(bits, L, qb, kblock, &t)) continue;
      if (tiles) tiles[n] = t;
      ++n;
    }
  }
  start[nqb] = n;
  return n;
}

// Entries of the list tiles[begin .. end - 1] a sequence of n tokens walks: those with 64 kblock < n, a prefix of the ascending list
inline int tf_mask_tiles_corner(const TfMaskTile* tiles, int begin, int end, int n) {
  int c = 0;
  while (begin + c < end && (long long)tiles[begin + c].kblock * kTfAttnTiledKB < n) ++c;
  return c;
}

// The mask word a lane of tf_attn_tiled_masked loads in a "some" step: row min(query, n - 1) of the sequence of n <= L tokens, the
// word of the step that starts at key kb < n (a multiple of 32) -- an index into bits [L][tf_mask_words(L)]
inline size_t tf_mask_lane_word(int L, int n, int query, int kb) { return (size_t)(query < n ? query : n - 1) * tf_mask_words(L) + (size_t)(kb >> 5); }
// ... and the bit of that word that belongs to the key of accumulator element q = 0 .. 3 of S^T tile u = 0 .. 1 in lane group g = 0 .. 3:
// key kb + 16 u + 4 g + q (tf_attn16_step)
constexpr int tf_mask_lane_bit(int u, int g, int q) { return u * 16 + g * 4 + q; }

// What flope_tf_mask_tiles reports: the lists' total, and the 8 (wave, step) tiles of every listed entry by class
struct TfMaskTileStats { int query_blocks; long long blocks_listed, steps_none, steps_some, steps_all; };
inline TfMaskTileStats tf_mask_tile_stats(int L, const int* start, const TfMaskTile* tiles) {
  TfMaskTileStats st = {tf_mask_query_blocks(L), 0, 0, 0, 0};
  st.blocks_listed = start[st.query_blocks];
  for (long long i = 0; i < st.blocks_listed; ++i)
    for (int k = 0; k < 8; ++k) {
      const int c = tf_mask_tile_class(tiles[i].cls, k >> 1, k & 1);
      ++(c == kTfMaskNone ? st.steps_none : c == kTfMaskSome ? st.steps_some : st.steps_all);
    }
  return st;
}

// One device allocation holds bits | first | last | start | tiles; the entries start on a 16-byte boundary
inline size_t tf_mask_dev_start_at(int L) { return ((size_t)L * tf_mask_words(L) + 2 * (size_t)L) * 4; }
inline size_t tf_mask_dev_tiles_at(int L) { return (tf_mask_dev_start_at(L) + ((size_t)tf_mask_query_blocks(L) + 1) * 4 + 15) / 16 * 16; }
inline size_t tf_mask_dev_bytes(int L, long long entries) { return tf_mask_dev_tiles_at(L) + (size_t)entries * sizeof(TfMaskTile); }

// The kernel a masked 16-bit launch takes: tf_attn_tiled_masked for a 16-bit handle under option mask_mfma = 1 (generic = 0) at every
// head_dim tf_attn_tiled serves, whatever option attn_tiled says (head_dim 64 at L <= 512 included); tf_attn_masked otherwise.
inline int tf_attn_pick_masked(int dtype, int head_dim, int opt_generic, int opt_mask_mfma, int aligned16) {
  if (dtype != FLOPE_DT_F32 && opt_mask_mfma == 1 && !opt_generic && tf_attn_tiled_ok(head_dim) && aligned16) return FLOPE_TF_ATTN_MASKED16;
  return FLOPE_TF_ATTN_MASKED;
}
// Grid, block and LDS of tf_attn_tiled_masked: tf_attn_tiled's, sized by the longest sequence; no mask rows in LDS
inline TfAttnLaunch tf_mask16_launch(int head_dim, int B, int H, int max_len) {
  return tf_attn_varlen_launch(FLOPE_TF_ATTN_TILED, head_dim, B, H, max_len);
}

// ---- a compiled additive bias (flope_tf_bias_create) --------------------------------------------------------------------------
// bias: float32 [planes][L][L], planes = 1 (one plane for every head) or the handle's num_heads.  -inf = the pair is masked, a finite
// value = allowed with that value added to its score; +inf and NaN have no meaning and are refused.  The allowed set is one for all
// heads (the kernel walks one set of bit words), so every plane must hold its -inf where plane 0 does.  The launch is tf_mask_launch.

// The first entry in (plane, row, col) order that is +inf or NaN: true with its index written, false: none
inline bool tf_bias_nonfinite(const float* bias, int L, int planes, int* plane, int* row, int* col) {
  const size_t LL = (size_t)L * L;
  for (size_t t = 0; t < (size_t)planes * LL; ++t) {
    const float b = bias[t];
    if (isnan(b) || (isinf(b) && b > 0.f)) {
      if (plane) *plane = (int)(t / LL);
      if (row) *row = (int)(t % LL / (size_t)L);
      if (col) *col = (int)(t % (size_t)L);
      return true;
    }
  }
  return false;
}

// The first entry in (plane >= 1, row, col) order whose masked-or-not differs from plane 0's: true with its index written, false: none
inline bool tf_bias_plane_differs(const float* bias, int L, int planes, int* plane, int* row, int* col) {
  const size_t LL = (size_t)L * L;
  for (int p = 1; p < planes; ++p)
    for (size_t t = 0; t < LL; ++t)
      if ((bias[t] == -INFINITY) != (bias[(size_t)p * LL + t] == -INFINITY)) {
        if (plane) *plane = p;
        if (row) *row = (int)(t / (size_t)L);
        if (col) *col = (int)(t % (size_t)L);
        return true;
      }
  return false;
}

// Plane 0's allowed set as bits [L][tf_mask_words(L)]: the words tf_mask_pack gives for allow[i][j] = (bias[0][i][j] != -inf)
inline void tf_bias_pack(const float* bias, int L, uint32_t* bits) {
  const int nw = tf_mask_words(L);
  for (int i = 0; i < L; ++i)
    for (int w = 0; w < nw; ++w) {
      uint32_t m = 0;
      for (int j = w * 32; j < L && j < w * 32 + 32; ++j)
        if (bias[(size_t)i * L + j] != -INFINITY) m |= 1u << (j & 31);
      bits[(size_t)i * nw + w] = m;
    }
}

// One device allocation holds bits | first | last | bias: the planes start behind the two tables, 4-byte aligned as everything in it
inline size_t tf_bias_dev_bias_at(int L) { return tf_mask_dev_start_at(L); }
inline size_t tf_bias_dev_bytes(int L, int planes) { return tf_bias_dev_bias_at(L) + (size_t)planes * L * L * 4; }
// The bias entry the lane that owns key j of query i of head h loads: an index into the float32 planes (plane 0 for every head when
// planes == 1).  i and j are positions in the mask's L x L planes whatever the length of the sequence (the corner's rows keep stride L).
inline size_t tf_bias_index(int L, int planes, int h, int i, int j) { return ((size_t)(planes > 1 ? h : 0) * L + (size_t)i) * L + (size_t)j; }

// ---- a compiled bias on the 16-bit MFMA attention (option "bias_mfma") ----------------------------------------------------
// tf_attn_tiled_masked's BIASED instantiation walks the tile map of the bias's allowed set (the -inf entries of plane 0) and so needs it on
// the device: a bias handle's allocation is bits | first | last | bias | start | tiles, the map BEHIND the planes, so that
// tf_bias_dev_bias_at and tf_bias_dev_bytes (the end of the planes) keep their values; the entries start on a 16-byte boundary.  Uploaded
// for every bias: the option may be flipped between forwards.
inline size_t tf_bias_dev_start_at(int L, int planes) { return tf_bias_dev_bytes(L, planes); }
inline size_t tf_bias_dev_tiles_at(int L, int planes) { return (tf_bias_dev_start_at(L, planes) + ((size_t)tf_mask_query_blocks(L) + 1) * 4 + 15) / 16 * 16; }
inline size_t tf_bias_dev_bytes_tiled(int L, int planes, long long entries) { return tf_bias_dev_tiles_at(L, planes) + (size_t)entries * sizeof(TfMaskTile); }

// The head_dims whose BIASED instantiation of tf_attn_tiled_masked was built without scratch (all four that
// tf_attn_tiled_ok admits); a head_dim that is not listed here keeps tf_attn_masked under a bias.
constexpr bool tf_attn_biased16_built(int head_dim) { return head_dim == 32 || head_dim == 64 || head_dim == 96 || head_dim == 128; }

// The kernel a launch under a compiled bias takes: tf_attn_tiled_masked's BIASED instantiation for a 16-bit handle under option
// bias_mfma = 1 (generic = 0) at every head_dim tf_attn_tiled serves and that instantiation was built for without scratch, 16-byte aligned
// buffers; tf_attn_masked's otherwise.  Option mask_mfma has no say: it is the plain masks' option.
inline int tf_attn_pick_biased(int dtype, int head_dim, int opt_generic, int opt_bias_mfma, int aligned16) {
  if (dtype != FLOPE_DT_F32 && opt_bias_mfma == 1 && !opt_generic && tf_attn_tiled_ok(head_dim) && tf_attn_biased16_built(head_dim) && aligned16)
    return FLOPE_TF_ATTN_BIASED16;
  return FLOPE_TF_ATTN_BIASED;
}

// The bias entry a lane of the BIASED tf_attn_tiled_masked loads for accumulator element q = 0 .. 3 of S^T tile u = 0 .. 1 in lane group
// g = 0 .. 3 in the step that starts at key kb < n (a multiple of 32): row min(query, n - 1) of the sequence of n <= L tokens in plane h
// (plane 0 when planes == 1), the column of the key kb + 16 u + 4 g + q itself, clamped to L - 1 -- a key at or past L is never seen, and
// no address outside [0, L) of the row is formed.  An index into the float32 planes.
inline size_t tf_bias16_lane_index(int L, int planes, int n, int h, int query, int kb, int u, int g, int q) {
  const int col = kb + 16 * u + 4 * g + q;
  return tf_bias_index(L, planes, h, query < n ? query : n - 1, col < L ? col : L - 1);
}
// ... and whether the lanes of that step take one 16-byte load per (query tile, u) in place of four clamped dword loads: the plane rows
// start on 16-byte boundaries (L a multiple of 4; tf_bias_dev_bias_at(L) then is a multiple of 16) and the step's 32 columns lie inside the row
constexpr bool tf_bias16_step_vec(int L, int kb) { return !(L & 3) && kb + 32 <= L; }

}  // namespace flope_tf_plan
