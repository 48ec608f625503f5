// CPU-only test harness of the encoder's ragged-batch planner (flope_amd/csrc/tf_attn_plan.h): the function that validates a
// batch of per-sequence lengths and lays it out as packed rows, and the grid / block / LDS figures of the variable-length attention
// launches -- what flope_tf_forward_varlen and flope_tf_attention_varlen go through.  tests/test_tf_varlen_host.py checks both
// without a GPU, tests/test_gpu_tf_varlen.py compares the device's kernel ids with it.  Not part of the product.
#include "tf_attn_plan.h"

extern "C" {

// off: batch + 1 ints; out3: {T, max_len, index of the offending length or -1}.  Returns 0 or the planner's error code.
int tf_varlen_plan(const int* lengths, int batch, int seq_len, int max_tokens, int* off, int* out3) {
  int T = -1, mx = -1, bad = -1;
  const int rc = flope_tf_plan::tf_varlen_plan(lengths, batch, seq_len, max_tokens, off, &T, &mx, &bad);
  if (out3) { out3[0] = T; out3[1] = mx; out3[2] = bad; }
  return rc;
}

int tf_varlen_err(int i) {
  const int codes[5] = {flope_tf_plan::kTfVarlenOk, flope_tf_plan::kTfVarlenBatch, flope_tf_plan::kTfVarlenLength,
                        flope_tf_plan::kTfVarlenTokens, flope_tf_plan::kTfVarlenOverflow};
  return i >= 0 && i < 5 ? codes[i] : 1;
}

// out4: {grid_x, grid_y, block, lds bytes} of the variable-length launch of kernel `which`
void tf_varlen_launch(int which, int head_dim, int batch, int heads, int max_len, long* out4) {
  const flope_tf_plan::TfAttnLaunch l = flope_tf_plan::tf_attn_varlen_launch(which, head_dim, batch, heads, max_len);
  out4[0] = l.grid_x; out4[1] = l.grid_y; out4[2] = l.block; out4[3] = (long)l.lds;
}

// the kernel a ragged batch runs: tf_attn_pick at the longest sequence (a pass-through: what launch_attention hands it for a ragged batch is
// checked on the device, tests/test_gpu_tf_varlen.py)
int tf_varlen_pick(int dtype, int head_dim, int max_len, int opt_generic, int opt_f32m, int opt_tiled, int aligned16) {
  return flope_tf_plan::tf_attn_pick(dtype, head_dim, max_len, opt_generic, opt_f32m, opt_tiled, aligned16);
}

}  // extern "C"
