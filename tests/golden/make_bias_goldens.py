"""Regenerates tests/golden/tf_bias_fixture.npz from the reference tree: its TransformerEncoder (scripts/tf_encoder.py) run in eval
mode on the CPU with nn.TransformerEncoder's float mask = four additive biases:
  alibi      causal ALiBi, slope 0.5, one [L, L] plane
  alibi_h    causal ALiBi, slopes 2^-(h + 1), one plane per head (torch's [B * H, L, L] form: the H planes repeated batch-major)
  rand       2 randn with 40 % -inf off the diagonal (generator seed 5), one plane
  rand_h     the same allowed set with an independent 2 randn per head
Data only: x, the biases (float32, -inf = masked), the outputs and the state dict.

    python tests/golden/make_bias_goldens.py [path of the reference tree]     (default: $FLOPE_REFERENCE)

Same settings as make_mask_goldens.py (toy dims, seed 11, x [6, 15, 16]).

The reference runs with torch.backends.mha.set_fastpath_enabled(False).  With torch 2.10 the eval / no-grad fast path of
nn.TransformerEncoder on the CPU treats every non-zero entry of a float mask as masked: an ALiBi mask comes back 1.09 away from the
fp64 restatement (only the diagonal's 0 survives, so the per-head and 2-D forms even agree), a random finite bias gives NaN.  With the
fast path off the module agrees with fp64 to 5.2e-7.  The assertion below (1e-5 against tests/tf_attn_bias_bound.py's biased_forward)
fails with the fast path on; the -inf / 0 fixtures of make_mask_goldens.py are not affected.
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import tf_attn_bias_bound as BB  # noqa: E402

DIMS = (16, 32, 9, 4, 2, 64)
H = DIMS[3]
L = 15
BATCH = 6


def biases():
    """name -> float32 [L, L] or [H, L, L]"""
    g = torch.Generator().manual_seed(5)
    masked = torch.rand(L, L, generator=g) < 0.4
    masked[torch.arange(L), torch.arange(L)] = False
    rand = 2 * torch.randn(L, L, generator=g)
    rand_h = 2 * torch.randn(H, L, L, generator=g)
    return {"alibi": BB.alibi(L, [0.5])[0],
            "alibi_h": BB.alibi(L, [2.0 ** -(h + 1) for h in range(H)]),
            "rand": rand.masked_fill(masked, float("-inf")),
            "rand_h": rand_h.masked_fill(masked[None], float("-inf"))}


def bias_fixture(ref):
    spec = importlib.util.spec_from_file_location("ref_tf", os.path.join(ref, "scripts/tf_encoder.py"))
    ref_tf = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref_tf)
    torch.manual_seed(11)
    enc = ref_tf.TransformerEncoder(*DIMS, 0.1).eval()
    x = torch.randn(BATCH, L, 16)
    out = {"x": x.numpy()}
    sd = {k: v.numpy() for k, v in enc.state_dict().items()}
    torch.backends.mha.set_fastpath_enabled(False)          # the fast path masks every non-zero entry of a float mask (see above)
    with torch.no_grad():
        h = enc.embedding(x)
        for name, b in biases().items():
            m = b if b.dim() == 2 else b.repeat(BATCH, 1, 1)                   # [B * H, L, L], batch-major
            y = enc.out_layer(enc.transformer_encoder(h, mask=m)).numpy()
            worst = float(np.abs(BB.biased_forward(sd, out["x"], b.numpy(), num_heads=H) - y).max())
            print(f"{name}: reference vs the fp64 restatement {worst:.2e}")
            assert worst < 1e-5, (name, worst)
            out["bias_" + name] = b.numpy()
            out["y_" + name] = y
    for k, v in sd.items():
        out["sd::" + k] = v
    path = os.path.join(HERE, "tf_bias_fixture.npz")
    np.savez_compressed(path, **out)
    print("tf_bias_fixture.npz:", len(out), "arrays; y", tuple(out["y_alibi"].shape), os.path.getsize(path), "bytes")


if __name__ == "__main__":
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("FLOPE_REFERENCE", "")
    if not os.path.isdir(ref):
        sys.exit("reference tree not given: pass its path or set FLOPE_REFERENCE")
    bias_fixture(ref)
