"""Writes tests/golden/pose_cases.npz: the input classes of tests/pose_cases.py with their references (float64 SVD where
gap / |M|_F >= 1e-6, mpmath at 60 digits below), so that the GPU tests need no mpmath.  Deterministic; run from the repository root:
    python tests/golden/make_pose_goldens.py
tests/test_pose_bound.py regenerates a sample per class and compares it with the file."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import pose_cases as PC  # noqa: E402


def build():
    out = {}
    for c in PC.PROCRUSTES_CLASSES:
        M = PC.procrustes_class(c)
        out[f"M/{c}"] = M
        if c != "nonfinite":
            R, gap, fro, used_mp = PC.procrustes_reference(M)
            out[f"R/{c}"], out[f"gap/{c}"], out[f"fro/{c}"], out[f"mp/{c}"] = R, gap, fro, used_mp
    for c in PC.YAW_CLASSES:
        R = PC.yaw_class(c)
        out[f"yawR/{c}"], out[f"yawO/{c}"] = R, PC.yaw_reference(R)
    return out


if __name__ == "__main__":
    np.savez_compressed(PC.GOLDEN, **build())
    print("wrote", PC.GOLDEN, os.path.getsize(PC.GOLDEN), "bytes")
