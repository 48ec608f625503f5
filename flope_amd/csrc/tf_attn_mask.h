// A compiled [L, L] attention mask (flope_tf_mask_*): the set of (query i, key j) pairs that may attend, as bits, and
// what the host derives from them -- plain integer arithmetic, no HIP, shared by tf_encoder.hip (flope_tf_mask_create and the masked
// entry points) and tests/host_harness/harness_tf_mask.cpp (tests/test_tf_mask_host.py holds every function against brute force).
// Layout: uint32 words [L][tf_mask_words(L)], bit j % 32 of word j / 32 of row i set = query i may attend to key j; the padding bits
// (columns L .. 32 * words - 1) are zero.  first[i] / last[i]: the first and last allowed key of row i; a row without a key has
// first = L and last = -1.
#pragma once

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

}  // namespace flope_tf_plan
