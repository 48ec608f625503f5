"""Regenerates tests/golden/tf_varlen_fixture.npz from the reference tree: its TransformerEncoder (scripts/tf_encoder.py) run in eval
mode on a right-padded ragged batch with nn.TransformerEncoder's src_key_padding_mask.  Data only: x, lengths, y and the state dict.

    python tests/golden/make_varlen_goldens.py [path of the reference tree]     (default: $FLOPE_REFERENCE)

L = 15 is the padded flower count of the reference's dataset (sunflower/dataset/flower_attn_dataset.py:277-288).
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
DIMS = (16, 32, 9, 4, 2, 64)
LENGTHS = [15, 1, 7, 12, 3, 15]


def varlen_fixture(ref):
    spec = importlib.util.spec_from_file_location("ref_tf", os.path.join(ref, "scripts/tf_encoder.py"))
    ref_tf = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref_tf)
    torch.manual_seed(11)
    enc = ref_tf.TransformerEncoder(*DIMS, 0.1).eval()
    x = torch.randn(6, 15, 16)
    lengths = torch.tensor(LENGTHS)
    mask = torch.arange(15)[None, :] >= lengths[:, None]              # True = padding
    with torch.no_grad():
        y = enc.out_layer(enc.transformer_encoder(enc.embedding(x), src_key_padding_mask=mask))
    out = {"x": x.numpy(), "lengths": lengths.numpy().astype(np.int32), "y": y.numpy()}
    for k, v in enc.state_dict().items():
        out["sd::" + k] = v.numpy()
    path = os.path.join(HERE, "tf_varlen_fixture.npz")
    np.savez_compressed(path, **out)
    print("tf_varlen_fixture.npz:", len(out), "arrays; y", tuple(y.shape), os.path.getsize(path), "bytes")


if __name__ == "__main__":
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("FLOPE_REFERENCE", "")
    if not os.path.isdir(ref):
        sys.exit("reference tree not given: pass its path or set FLOPE_REFERENCE")
    varlen_fixture(ref)
