// CPU-only test harness of the encoder's attention launch planner (flope_amd/csrc/tf_attn_plan.h): the selection function that
// flope_tf_forward and flope_tf_attention go through, the LDS bytes of each launch and the constants of tf_attn_tiled's ring, so
// that tests/test_tf_attn_plan_host.py checks the table without a GPU and tests/test_gpu_tf_attn_tiled.py derives its ring-reuse
// shapes from what the kernel was built with.  Not part of the product.
#include "tf_attn_plan.h"

extern "C" {

int tf_attn_pick(int dtype, int head_dim, int seq_len, int opt_generic, int opt_f32m, int opt_tiled, int aligned16) {
  return flope_tf_plan::tf_attn_pick(dtype, head_dim, seq_len, opt_generic, opt_f32m, opt_tiled, aligned16);
}

// which: FLOPE_TF_ATTN_* id; bytes of dynamic LDS that kernel is launched with at this shape (generic: four waves of seq_len floats)
long tf_attn_lds_bytes(int which, int head_dim, int seq_len) {
  switch (which) {
    case FLOPE_TF_ATTN_GENERIC: return (long)4 * seq_len * 4;
    case FLOPE_TF_ATTN_MFMA64: return (long)flope_tf_plan::tf_attn_mfma64_lds(seq_len);
    case FLOPE_TF_ATTN_TILED: return (long)flope_tf_plan::tf_attn_tiled_lds(head_dim);
    case FLOPE_TF_ATTN_F32M: return (long)flope_tf_plan::tf_attn_f32m_lds(head_dim, seq_len);
  }
  return -1;
}

int tf_attn_tiled_kb(void) { return flope_tf_plan::kTfAttnTiledKB; }
int tf_attn_tiled_ring(void) { return flope_tf_plan::kTfAttnTiledRing; }
int tf_attn_tiled_queries(void) { return flope_tf_plan::kTfAttnTiledQueries; }
int tf_attn_id(int i) {
  const int ids[4] = {FLOPE_TF_ATTN_GENERIC, FLOPE_TF_ATTN_MFMA64, FLOPE_TF_ATTN_TILED, FLOPE_TF_ATTN_F32M};
  return i >= 0 && i < 4 ? ids[i] : -1;
}

}  // extern "C"
