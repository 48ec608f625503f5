// CPU-only test harness of causal attention's planner (flope_amd/csrc/tf_attn_plan.h): the constexpr functions that say how far a
// query group walks the keys under option "causal" -- the ones tf_attn_generic, tf_attn_mfma, tf_attn_tiled and tf_attn_f32m call.
// tests/test_tf_causal_host.py holds them against brute force without a GPU and runs tfc_selfcheck once in a stand-alone
// program built with -DTF_CAUSAL_MAIN under AddressSanitizer + UBSan.  Not part of the product.
#include "tf_attn_plan.h"

#include <vector>

extern "C" {

int tfc_keys(int q_first, int nq, int seq_len) { return flope_tf_plan::tf_causal_keys(q_first, nq, seq_len); }
int tfc_tiled_blocks(int qblock, int seq_len) { return flope_tf_plan::tf_causal_tiled_blocks(qblock, seq_len); }
int tfc_step_taken(int q0, int kb) { return flope_tf_plan::tf_causal_step_taken(q0, kb) ? 1 : 0; }
int tfc_f32m_tiles(int q0, int seq_len) { return flope_tf_plan::tf_causal_f32m_tiles(q0, seq_len); }

// The 32-key steps wave `wave` (0 .. 3) of tf_attn_tiled's workgroup `qblock` runs for a sequence of seq_len tokens, in order, as the
// kernel's loop decides them: blocks t < tf_causal_tiled_blocks, steps st of a block, kb < seq_len, tf_causal_step_taken.  steps: room
// for cap first keys; *trips: the barrier-loop trip count.  Returns the number of steps (may exceed cap: only cap are written).
int tfc_tiled_walk(int qblock, int wave, int seq_len, int* steps, int cap, int* trips) {
  using namespace flope_tf_plan;
  const int q0 = qblock * kTfAttnTiledQueries + wave * 32, nb = tf_causal_tiled_blocks(qblock, seq_len);
  int n = 0;
  for (int t = 0; t < nb; ++t)
    for (int st = 0; st < kTfAttnTiledKB / 32; ++st) {
      const int kb = t * kTfAttnTiledKB + st * 32;
      if (kb >= seq_len) continue;
      if (!tf_causal_step_taken(q0, kb)) continue;
      if (n < cap) steps[n] = kb;
      ++n;
    }
  if (trips) *trips = nb;
  return n;
}

// ... and of wave `wave` of tf_attn_mfma (one workgroup per head, pad32(seq_len) / 32 waves): steps kb < min(Lp, q0 + 32)
int tfc_mfma_walk(int wave, int seq_len, int* steps, int cap) {
  using namespace flope_tf_plan;
  const int q0 = wave * 32, end = tf_causal_keys(q0, 32, tf_attn_pad32(seq_len));
  int n = 0;
  for (int kb = 0; kb < end; kb += 32) {
    if (n < cap) steps[n] = kb;
    ++n;
  }
  return n;
}

// Every property tests/test_tf_causal_host.py states, for every seq_len <= max_len, on heap arrays sized exactly (the sanitizer's
// business): 0, or a code that names the first property that failed.
int tfc_selfcheck(int max_len) {
  using namespace flope_tf_plan;
  for (int L = 1; L <= max_len; ++L) {
    const int nsteps = tf_attn_pad32(L) / 32;
    std::vector<int> steps((size_t)nsteps);
    std::vector<char> covered((size_t)L);
    for (int qb = 0; qb * kTfAttnTiledQueries < L; ++qb) {
      int trips0 = -1;
      for (int w = 0; w < 4; ++w) {
        int trips = -1;
        const int q0 = qb * kTfAttnTiledQueries + w * 32;
        const int n = tfc_tiled_walk(qb, w, L, steps.data(), nsteps, &trips);
        if (n > nsteps) return 1;
        if (w == 0) trips0 = trips; else if (trips != trips0) return 2;
        if (q0 >= L) continue;                                     // a wave of clamped queries: nothing of it is stored
        covered.assign((size_t)L, 0);
        for (int i = 0; i < n; ++i) {
          if (steps[i] > (q0 + 31 < L - 1 ? q0 + 31 : L - 1)) return 3;          // a step wholly above the wave's last query
          for (int k = steps[i]; k < steps[i] + 32 && k < L; ++k) covered[(size_t)k] = 1;
        }
        if (n < 1 || steps[0] != 0) return 4;                       // a wave starts at step 0
        for (int q = q0; q < q0 + 32 && q < L; ++q)
          for (int k = 0; k <= q; ++k)
            if (!covered[(size_t)k]) return 5;
      }
    }
    for (int w = 0; w * 32 < L; ++w) {
      const int n = tfc_mfma_walk(w, L, steps.data(), nsteps);
      if (n > nsteps || n < 1 || steps[0] != 0) return 6;
      if (steps[n - 1] > (w * 32 + 31 < L - 1 ? w * 32 + 31 : L - 1)) return 7;
      if (steps[n - 1] + 32 < tf_causal_keys(w * 32, 32, L)) return 8;
    }
    for (int q0 = 0; q0 < L; q0 += 16) {
      const int nt = tf_causal_f32m_tiles(q0, L), last = q0 + 15 < L - 1 ? q0 + 15 : L - 1;
      if (nt * 16 <= last) return 9;                               // the last query's own key lies in a walked tile
      if ((nt - 1) * 16 > last) return 10;                         // no tile wholly above it
      if (nt * 16 > ((L + 15) & ~15)) return 11;                   // inside the score rows the launch allocates
    }
    for (int i = 0; i < L; ++i)
      if (tf_causal_keys(i, 1, L) != i + 1) return 12;
  }
  return 0;
}

}  // extern "C"

#ifdef TF_CAUSAL_MAIN
#include <stdio.h>
int main() {
  const int rc = tfc_selfcheck(300);
  printf("tfc_selfcheck(300) = %d\n", rc);
  return rc;
}
#endif
