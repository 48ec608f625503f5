"""The cases of the encoder's architecture tests, shared by tests/golden/make_arch_goldens.py, tests/test_tf_arch_ref.py
and tests/test_gpu_tf_arch.py: the eight (norm_first, activation, final_norm) combinations, the two shapes, the weights, and the fp64
reference -- torch's own nn.TransformerEncoderLayer / nn.TransformerEncoder in float64 on the CPU.

Weights: oracle.tf_encoder_ref.synthetic_state_dict(seed 5) rounded to float32, as load_state_dict rounds them; the final norm
weight = 1 + 0.1 N(0, 1), bias = 0.1 N(0, 1) from a fixed seed.  Inputs: standard normal float32 from a fixed seed.
"""
import itertools
import os

import numpy as np
import torch

from oracle import tf_encoder_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "tf_arch_fixture.npz")

SHAPES = {"a": (16, 128, 9, 2, 2, 256), "b": (24, 384, 9, 6, 2, 1536)}       # (input_dim, model_dim, out_dim, heads, layers, ff_dim)
BL = ((5, 50), (2, 33))
ARCHS = [{"norm_first": nf, "activation": act, "final_norm": fn}
         for nf, act, fn in itertools.product((False, True), ("relu", "gelu"), (False, True))]
DEFAULT = ARCHS[0]
NON_DEFAULT = ARCHS[1:]
TOL = {"f32": 2e-4, "f32m": 2e-4, "f16": 1.5e-2, "bf16": 1.2e-1}             # tests/test_gpu_tf_encoder.py's, for these weights and shapes


def arch_id(a):
    return ("pre" if a["norm_first"] else "post") + "-" + a["activation"] + ("-fn" if a["final_norm"] else "")


def state_dict(dims, final_norm):
    sd = T.synthetic_state_dict(dims[0], dims[1], dims[2], dims[4], dims[5], seed=5)
    sd = {k: torch.from_numpy(np.asarray(v, dtype=np.float32)) for k, v in sd.items()}
    if final_norm:
        g = torch.Generator().manual_seed(50)
        sd["transformer_encoder.norm.weight"] = 1.0 + 0.1 * torch.randn(dims[1], generator=g)
        sd["transformer_encoder.norm.bias"] = 0.1 * torch.randn(dims[1], generator=g)
    return sd


def inputs(dims, B, L):
    g = torch.Generator().manual_seed(9000 + dims[1] + 13 * B + L)
    return torch.randn(B, L, dims[0], generator=g)


class TorchEncoder(torch.nn.Module):
    """the reference script's module shape, with torch's architecture keywords"""

    def __init__(self, dims, norm_first=False, activation="relu", final_norm=False, **layer_kw):
        super().__init__()
        i, d, o, h, nl, ff = dims
        self.embedding = torch.nn.Linear(i, d)
        layer = torch.nn.TransformerEncoderLayer(d, h, ff, dropout=0.0, activation=activation, batch_first=True, norm_first=norm_first, **layer_kw)
        self.transformer_encoder = torch.nn.TransformerEncoder(layer, nl, norm=torch.nn.LayerNorm(d) if final_norm else None,
                                                               enable_nested_tensor=False)
        self.out_layer = torch.nn.Linear(d, o)

    def forward(self, x):
        return self.out_layer(self.transformer_encoder(self.embedding(x)))


def torch_reference(dims, arch, x):
    """fp64 [B, L, out_dim] of torch's own module under `arch`"""
    m = TorchEncoder(dims, **arch).double().eval()
    m.load_state_dict({k: v.double() for k, v in state_dict(dims, arch["final_norm"]).items()})
    with torch.no_grad():
        return m(x.double())


def key(shape, arch, B, L):
    return f"y_{shape}_{arch_id(arch)}_{B}x{L}"
