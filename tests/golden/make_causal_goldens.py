"""Regenerates tests/golden/tf_causal_fixture.npz from the reference tree: its TransformerEncoder (scripts/tf_encoder.py) run in eval
mode with nn.TransformerEncoder's mask = generate_square_subsequent_mask(L), once on the full batch and once with the right-padding
src_key_padding_mask of a ragged batch on top of it.  Data only: x, lengths, the two outputs and the state dict.

    python tests/golden/make_causal_goldens.py [path of the reference tree]     (default: $FLOPE_REFERENCE)

Same settings as make_varlen_goldens.py (toy dims, seed 11, x [6, 15, 16]).  With a mask torch leaves its nested-tensor path: the
rows behind a sequence of y_causal_padded hold what torch computes there, not out_layer.bias -- only the valid rows are meaningful.
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
DIMS = (16, 32, 9, 4, 2, 64)
LENGTHS = [15, 1, 7, 12, 3, 15]


def causal_fixture(ref):
    spec = importlib.util.spec_from_file_location("ref_tf", os.path.join(ref, "scripts/tf_encoder.py"))
    ref_tf = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref_tf)
    torch.manual_seed(11)
    enc = ref_tf.TransformerEncoder(*DIMS, 0.1).eval()
    x = torch.randn(6, 15, 16)
    lengths = torch.tensor(LENGTHS)
    pad = torch.arange(15)[None, :] >= lengths[:, None]               # True = padding
    causal = torch.nn.Transformer.generate_square_subsequent_mask(15)
    with torch.no_grad():
        h = enc.embedding(x)
        y = enc.out_layer(enc.transformer_encoder(h, mask=causal))
        yp = enc.out_layer(enc.transformer_encoder(h, mask=causal, src_key_padding_mask=pad))
    out = {"x": x.numpy(), "lengths": lengths.numpy().astype(np.int32), "y_causal": y.numpy(), "y_causal_padded": yp.numpy()}
    for k, v in enc.state_dict().items():
        out["sd::" + k] = v.numpy()
    path = os.path.join(HERE, "tf_causal_fixture.npz")
    np.savez_compressed(path, **out)
    print("tf_causal_fixture.npz:", len(out), "arrays; y", tuple(y.shape), os.path.getsize(path), "bytes")


if __name__ == "__main__":
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("FLOPE_REFERENCE", "")
    if not os.path.isdir(ref):
        sys.exit("reference tree not given: pass its path or set FLOPE_REFERENCE")
    causal_fixture(ref)
