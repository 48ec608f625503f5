"""Writes tests/golden/tf_arch_fixture.npz: for the two shapes and the two (B, L) of tests/tf_arch_cases.py the float32
inputs, the final-norm parameters, and the fp64 outputs of torch's own nn.TransformerEncoder for the seven non-default architectures.
tests/test_tf_arch_ref.py recomputes every array with torch and compares; the GPU tests read the file only.

    python tests/golden/make_arch_goldens.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import tf_arch_cases as AC  # noqa: E402


def build():
    out = {}
    for s, dims in AC.SHAPES.items():
        sd = AC.state_dict(dims, True)
        out[f"fnw_{s}"] = sd["transformer_encoder.norm.weight"].numpy()
        out[f"fnb_{s}"] = sd["transformer_encoder.norm.bias"].numpy()
        for B, L in AC.BL:
            x = AC.inputs(dims, B, L)
            out[f"x_{s}_{B}x{L}"] = x.numpy()
            for arch in AC.NON_DEFAULT:
                out[AC.key(s, arch, B, L)] = AC.torch_reference(dims, arch, x).numpy()
    return out


if __name__ == "__main__":
    arrays = build()
    np.savez_compressed(AC.FIXTURE, **arrays)
    print(AC.FIXTURE, os.path.getsize(AC.FIXTURE), "bytes,", len(arrays), "arrays")
