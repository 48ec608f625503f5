"""The planner of option "skinny" without a device (flope_amd/csrc/tf_skinny_plan.h, which tf_gemm_skinny calls per lane, through
tests/host_harness/harness_tf_skinny.cpp).

  1. tf_skinny_ok against a brute-force statement of the rule: every M in 0 .. 40, every combination of the options, packed or not;
     the token-tile count; the constants;
  2. for N in {128, 256, 384, 1152, 1536}, K in {64, 128, 256, 384, 1536}, MT in {1, 2}: the grid's waves cover every (feature tile,
     token tile) and their lanes every output element exactly once, every weight load lies inside the packed image and every token
     load inside 16 MT rows, and the fragments are the ones tf_gemm_mfma's LDS read addresses select from the chunk's image (the harness
     restates both address computations, and the packer's row order and swizzle);
  3. copies broken the way the kernel can break are noticed;
  4. the same once more as a stand-alone program under -fsanitize=address,undefined (nothing is loaded into Python under a sanitizer);
  5. the new entry point is declared, bound and exported; the Python surface that needs no device.
"""
import ctypes as C
import itertools
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NS = (128, 256, 384, 1152, 1536)
KS = (64, 128, 256, 384, 1536)


@pytest.fixture(scope="module")
def H():
    path = os.path.join(ROOT, "tests", "host_harness", "libflope_host_tf_skinny.so")
    if not os.path.exists(path):
        subprocess.check_call(["make", "-C", ROOT, "tests/host_harness/libflope_host_tf_skinny.so"])
    lib = C.CDLL(path)
    lib.tf_skinny_h_ok.argtypes = [C.c_int] * 6
    lib.tf_skinny_h_mt.argtypes = [C.c_int]
    lib.tf_skinny_h_consts.argtypes = [C.c_void_p]
    lib.tf_skinny_h_launch.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    lib.tf_skinny_h_shape.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
    return lib


def shape(H, N, K, MT, broken=0):
    fails = (C.c_longlong * 4)()
    rc = H.tf_skinny_h_shape(N, K, MT, broken, fails)
    got = dict(zip(("cover", "bounds", "gemm", "meaning"), list(fails)))
    assert rc == int(any(got.values()))
    return got


# ---- 1. the rule ---------------------------------------------------------------------------------------------------------------------------
def test_ok_against_the_rule_by_brute_force(H):
    """true exactly where launch_linear would run tf_gemm_mfma (16-bit handle, packed image, 16-bit result, generic off), skinny == 1
    and 1 <= M <= 32"""
    taken = 0
    for M in range(0, 41):
        for d16, sk, gen, pk, yf in itertools.product((0, 1), repeat=5):
            mfma = bool(d16 and pk and not yf and not gen)
            want = mfma and sk == 1 and 1 <= M <= 32
            assert bool(H.tf_skinny_h_ok(d16, sk, gen, pk, yf, M)) == want, (M, d16, sk, gen, pk, yf)
            taken += want
    assert taken == 32
    for sk in (-1, 2, 3):                                             # only the value 1 turns it on
        assert not H.tf_skinny_h_ok(1, sk, 0, 1, 0, 8)


def test_token_tiles_and_constants(H):
    for M in range(1, 33):
        assert H.tf_skinny_h_mt(M) == (1 if M <= 16 else 2)
    c = (C.c_int * 3)()
    H.tf_skinny_h_consts(c)
    rows, waves, depth = list(c)
    assert rows == 32 and waves in (1, 2, 4, 8) and depth >= 2
    for N in NS:
        for MT in (1, 2):
            g, b = C.c_uint(), C.c_uint()
            H.tf_skinny_h_launch(N, MT, C.byref(g), C.byref(b))
            assert b.value == 64 * waves and g.value * waves == N // 16    # one wave per 16-row feature tile: N / 16 waves


# ---- 2. the shapes -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("MT", (1, 2))
@pytest.mark.parametrize("N", NS)
def test_cover_bounds_and_fragments(H, N, MT):
    for K in KS:
        assert shape(H, N, K, MT) == {"cover": 0, "bounds": 0, "gemm": 0, "meaning": 0}, (N, K, MT)


# ---- 3. broken copies ------------------------------------------------------------------------------------------------------------------------
def test_broken_copies_are_noticed(H):
    """the weight swizzle dropped; token tile 1 read eight rows early; the feature order of an unpermuted image"""
    for N, K in ((128, 64), (384, 384), (1536, 1536)):
        got = shape(H, N, K, 2, 1)
        assert got["gemm"] > 0 and got["meaning"] > 0 and got["cover"] == 0, got
        got = shape(H, N, K, 2, 2)
        assert got["gemm"] > 0 and got["meaning"] > 0 and got["bounds"] == 0, got
        assert shape(H, N, K, 1, 2) == {"cover": 0, "bounds": 0, "gemm": 0, "meaning": 0}        # (there is no tile 1 at MT = 1)
        got = shape(H, N, K, 1, 4)
        assert got["meaning"] > 0 and got["gemm"] == 0, got


# ---- 4. the same under AddressSanitizer + UBSan, as a program of its own ---------------------------------------------------------------------
def test_stand_alone_program_under_sanitizers(tmp_path):
    """every shape once in a stand-alone program of its own (host code only, nothing loaded into python): the loads are made from
    buffers of exactly N K 2 and 16 MT K 2 bytes"""
    exe = str(tmp_path / "tf_skinny_selfcheck")
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DTF_SKINNY_MAIN", "-std=c++17",
                           "-I" + os.path.join(ROOT, "flope_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "host_harness", "harness_tf_skinny.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "50 shapes, 0 failures" in r.stdout


# ---- 5. the surface ----------------------------------------------------------------------------------------------------------------------------
def test_linear_plan_is_declared_bound_and_exported():
    from flope_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "flope_amd.h")).read()
    assert re.search(r"\bint flope_tf_linear_plan\(", header)
    assert "flope_tf_linear_plan" in _lib.SIGNATURES and hasattr(lib, "flope_tf_linear_plan")
    assert re.search(r"#define FLOPE_TF_LIN_SKINNY\s+5\b", header) and _lib.TF_LIN_SKINNY == 5
    assert '"skinny"' in header


def test_python_surface_without_a_device():
    import inspect
    from flope_amd.tf_encoder import TransformerEncoder
    assert inspect.signature(TransformerEncoder.__init__).parameters["skinny"].default == 0
    assert list(inspect.signature(TransformerEncoder.linear_plan).parameters) == ["self", "name", "rows"]
