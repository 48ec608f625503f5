"""Regenerates tests/golden/tf_window_fixture.npz from the reference tree: its TransformerEncoder (scripts/tf_encoder.py) run in eval
mode on the CPU with nn.TransformerEncoder's mask = the banded causal mask of window W (masked where col > row or col <= row - W),
once as torch's float mask (-inf / 0) and once as its bool mask (True = masked), and once more with W = L, which is the causal
mask of make_causal_goldens.py.  Data only: x, W, the outputs and the state dict.

    python tests/golden/make_window_goldens.py [path of the reference tree]     (default: $FLOPE_REFERENCE)

Same settings as make_causal_goldens.py (toy dims, seed 11, x [6, 15, 16]); W = 4.
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
DIMS = (16, 32, 9, 4, 2, 64)
L, W = 15, 4


def band(L, W, dtype):
    i, j = torch.arange(L)[:, None], torch.arange(L)[None, :]
    masked = (j > i) | (j <= i - W)
    return masked if dtype == torch.bool else torch.zeros(L, L).masked_fill(masked, float("-inf"))


def window_fixture(ref):
    spec = importlib.util.spec_from_file_location("ref_tf", os.path.join(ref, "scripts/tf_encoder.py"))
    ref_tf = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref_tf)
    torch.manual_seed(11)
    enc = ref_tf.TransformerEncoder(*DIMS, 0.1).eval()
    x = torch.randn(6, L, 16)
    with torch.no_grad():
        h = enc.embedding(x)
        y = enc.out_layer(enc.transformer_encoder(h, mask=band(L, W, torch.float32)))
        yb = enc.out_layer(enc.transformer_encoder(h, mask=band(L, W, torch.bool)))
        yl = enc.out_layer(enc.transformer_encoder(h, mask=band(L, L, torch.float32)))
    out = {"x": x.numpy(), "W": np.int32(W), "y_window": y.numpy(), "y_window_bool": yb.numpy(), "y_window_L": yl.numpy()}
    for k, v in enc.state_dict().items():
        out["sd::" + k] = v.numpy()
    path = os.path.join(HERE, "tf_window_fixture.npz")
    np.savez_compressed(path, **out)
    print("tf_window_fixture.npz:", len(out), "arrays; y", tuple(y.shape), os.path.getsize(path), "bytes")


if __name__ == "__main__":
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("FLOPE_REFERENCE", "")
    if not os.path.isdir(ref):
        sys.exit("reference tree not given: pass its path or set FLOPE_REFERENCE")
    window_fixture(ref)
