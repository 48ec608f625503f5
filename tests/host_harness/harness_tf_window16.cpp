// CPU-only test harness of the window on the 16-bit MFMA attention kernels (flope_amd/csrc/tf_attn_plan.h, option "window_mfma";
// DESIGN.md 28): the constexpr functions tf_attn_mfma's and tf_attn_tiled's WINDOW instantiations call, their loops restated, and
// tf_attn_pick_window.  tests/test_tf_window16_host.py holds them against brute force without a GPU and runs tfw16_selfcheck once in a
// stand-alone program built with -DTF_WINDOW16_MAIN under AddressSanitizer + UBSan.  Not part of the product.
#include "tf_attn_plan.h"

#include <vector>

extern "C" {

int tfw16_first_step(int q0, int W) { return flope_tf_plan::tf_window_first_step(q0, W); }
int tfw16_step_taken(int q0, int kb, int W) { return flope_tf_plan::tf_window_step_taken(q0, kb, W) ? 1 : 0; }
int tfw16_tiled_first_block(int qblock, int W) { return flope_tf_plan::tf_window_tiled_first_block(qblock, W); }
int tfw16_pick(int dtype, int head_dim, int seq_len, int opt_generic, int opt_f32m, int opt_tiled, int opt_window_mfma, int aligned16) {
  return flope_tf_plan::tf_attn_pick_window(dtype, head_dim, seq_len, opt_generic, opt_f32m, opt_tiled, opt_window_mfma, aligned16);
}

// The 32-key steps wave `wave` (0 .. 3) of tf_attn_tiled's workgroup `qblock` runs for a sequence of seq_len tokens under window W, in
// order, as the kernel's loop decides them: blocks tf_window_tiled_first_block <= t < tf_causal_tiled_blocks, steps st of a block,
// kb < seq_len, tf_window_step_taken.  steps: room for cap first keys; *first, *end: the blocks the workgroup loads, first .. end - 1.
// Returns the number of steps (may exceed cap: only cap are written).
int tfw16_tiled_walk(int qblock, int wave, int seq_len, int W, int* steps, int cap, int* first, int* end) {
  using namespace flope_tf_plan;
  const int q0 = qblock * kTfAttnTiledQueries + wave * 32, nb = tf_causal_tiled_blocks(qblock, seq_len);
  const int t0 = tf_window_tiled_first_block(qblock, W);
  int n = 0;
  for (int t = t0; t < nb; ++t)
    for (int st = 0; st < kTfAttnTiledKB / 32; ++st) {
      const int kb = t * kTfAttnTiledKB + st * 32;
      if (kb >= seq_len) continue;
      if (!tf_window_step_taken(q0, kb, W)) continue;
      if (n < cap) steps[n] = kb;
      ++n;
    }
  if (first) *first = t0;
  if (end) *end = nb;
  return n;
}

// ... and of wave `wave` of tf_attn_mfma (one workgroup per head, pad32(seq_len) / 32 waves): tf_window_first_step <= kb < min(Lp, q0 + 32)
int tfw16_mfma_walk(int wave, int seq_len, int W, int* steps, int cap) {
  using namespace flope_tf_plan;
  const int q0 = wave * 32, end = tf_causal_keys(q0, 32, tf_attn_pad32(seq_len));
  int n = 0;
  for (int kb = tf_window_first_step(q0, W); kb < end; kb += 32) {
    if (n < cap) steps[n] = kb;
    ++n;
  }
  return n;
}

// Every property tests/test_tf_window16_host.py states, for every seq_len <= max_len, every W <= seq_len + 2 and every wave, on heap
// arrays sized exactly (the sanitizer's business): 0, or a code that names the first property that failed.
int tfw16_selfcheck(int max_len) {
  using namespace flope_tf_plan;
  for (int L = 1; L <= max_len; ++L) {
    const int nsteps = tf_attn_pad32(L) / 32;
    std::vector<int> steps((size_t)nsteps), causal((size_t)nsteps);
    std::vector<char> covered((size_t)L);
    for (int W = 0; W <= L + 2; ++W) {
      for (int qb = 0; qb * kTfAttnTiledQueries < L; ++qb) {
        int first0 = -1, end0 = -1;
        for (int w = 0; w < 4; ++w) {
          int first = -1, end = -1;
          const int q0 = qb * kTfAttnTiledQueries + w * 32;
          const int n = tfw16_tiled_walk(qb, w, L, W, steps.data(), nsteps, &first, &end);
          if (n > nsteps) return 1;
          if (w == 0) { first0 = first; end0 = end; } else if (first != first0 || end != end0) return 2;     // one trip count for the four waves
          if (first < 0 || first >= end || end != tf_causal_tiled_blocks(qb, L)) return 3;                 // a contiguous range that ends where causal ends
          for (int i = 0; i < n; ++i)
            if (steps[i] / kTfAttnTiledKB < first || steps[i] / kTfAttnTiledKB >= end) return 4;            // a taken step lies in a loaded block
          if (q0 >= L) continue;                                     // a wave of clamped queries: nothing of it is stored
          covered.assign((size_t)L, 0);
          for (int i = 0; i < n; ++i) {
            bool any = false;                                        // some query below L of the wave sees some key of the step
            for (int q = q0; q < q0 + 32 && q < L && !any; ++q)
              for (int k = steps[i]; k < steps[i] + 32 && k < L; ++k)
                if (k <= q && k >= tf_window_lo(q, W)) { any = true; break; }
            if (!any) return 5;
            for (int k = steps[i]; k < steps[i] + 32 && k < L; ++k) covered[(size_t)k] = 1;
          }
          for (int q = q0; q < q0 + 32 && q < L; ++q)
            for (int k = tf_window_lo(q, W); k <= q; ++k)
              if (!covered[(size_t)k]) return 6;                     // every visible pair lies in a taken step
          if (W == 0 || W >= L) {                                    // the causal walk
            const int nc = tf_causal_tiled_blocks(qb, L);
            int m = 0;
            for (int t = 0; t < nc; ++t)
              for (int st = 0; st < kTfAttnTiledKB / 32; ++st) {
                const int kb = t * kTfAttnTiledKB + st * 32;
                if (kb < L && tf_causal_step_taken(q0, kb)) causal[(size_t)m++] = kb;
              }
            if (first != 0 || m != n) return 7;
            for (int i = 0; i < n; ++i)
              if (steps[i] != causal[(size_t)i]) return 7;
          }
        }
      }
      for (int w = 0; w * 32 < L; ++w) {
        const int q0 = w * 32, n = tfw16_mfma_walk(w, L, W, steps.data(), nsteps);
        if (n > nsteps || n < 1) return 8;
        if (steps[0] != (tf_window_lo(q0, W) & ~31) || steps[n - 1] != q0) return 9;
        for (int i = 0; i < n; ++i)
          if (steps[i] != steps[0] + 32 * i || !tf_window_step_taken(q0, steps[i], W)) return 10;          // the same steps as the streamed walk
        if ((W == 0 || W >= L) && steps[0] != 0) return 11;
      }
    }
  }
  return 0;
}

}  // extern "C"

#ifdef TF_WINDOW16_MAIN
#include <stdio.h>
int main() {
  const int rc = tfw16_selfcheck(300);
  printf("tfw16_selfcheck(300) = %d\n", rc);
  return rc;
}
#endif
