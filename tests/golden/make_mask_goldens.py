"""Regenerates tests/golden/tf_mask_fixture.npz from the reference tree: its TransformerEncoder (scripts/tf_encoder.py) run in eval
mode on the CPU with nn.TransformerEncoder's mask = three [L, L] masks none of which is causal or a band:
  random   rand < 0.4 masked (generator seed 5), diagonal forced on; once as torch's bool mask (True = masked), once as its float
           mask (-inf / 0)
  blocks   block-diagonal over the lengths [4, 1, 7, 3]: a query sees the keys of its own block
  prefix   prefix-LM: the first 5 keys visible to every query, causal behind them
Data only: x, the masks (bool, True = masked), the outputs and the state dict.

    python tests/golden/make_mask_goldens.py [path of the reference tree]     (default: $FLOPE_REFERENCE)

Same settings as make_window_goldens.py (toy dims, seed 11, x [6, 15, 16]).
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
DIMS = (16, 32, 9, 4, 2, 64)
L = 15
BLOCKS = [4, 1, 7, 3]
PREFIX = 5


def masks():
    """name -> bool [L, L], True = masked"""
    g = torch.Generator().manual_seed(5)
    rnd = torch.rand(L, L, generator=g) < 0.4
    rnd[torch.arange(L), torch.arange(L)] = False
    blk = torch.ones(L, L, dtype=torch.bool)
    o = 0
    for n in BLOCKS:
        blk[o:o + n, o:o + n] = False
        o += n
    i, j = torch.arange(L)[:, None], torch.arange(L)[None, :]
    pre = (j > i) & (j >= PREFIX)
    return {"random": rnd, "blocks": blk, "prefix": pre}


def mask_fixture(ref):
    spec = importlib.util.spec_from_file_location("ref_tf", os.path.join(ref, "scripts/tf_encoder.py"))
    ref_tf = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref_tf)
    torch.manual_seed(11)
    enc = ref_tf.TransformerEncoder(*DIMS, 0.1).eval()
    x = torch.randn(6, L, 16)
    out = {"x": x.numpy()}
    with torch.no_grad():
        h = enc.embedding(x)
        for name, m in masks().items():
            out["mask_" + name] = m.numpy()
            out["y_" + name] = enc.out_layer(enc.transformer_encoder(h, mask=m)).numpy()
        fm = torch.zeros(L, L).masked_fill(masks()["random"], float("-inf"))
        out["y_random_float"] = enc.out_layer(enc.transformer_encoder(h, mask=fm)).numpy()
    for k, v in enc.state_dict().items():
        out["sd::" + k] = v.numpy()
    path = os.path.join(HERE, "tf_mask_fixture.npz")
    np.savez_compressed(path, **out)
    print("tf_mask_fixture.npz:", len(out), "arrays; y", tuple(out["y_random"].shape), os.path.getsize(path), "bytes")


if __name__ == "__main__":
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("FLOPE_REFERENCE", "")
    if not os.path.isdir(ref):
        sys.exit("reference tree not given: pass its path or set FLOPE_REFERENCE")
    mask_fixture(ref)
