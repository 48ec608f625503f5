"""The encoder's architecture list and its GELU without a device (flope_amd/csrc/tf_arch_plan.h, which run_forward_with walks, and
flope_amd/csrc/tf_act.h, which every linear kernel applies, through tests/host_harness/harness_tf_arch.cpp).

  1. the op list of all eight architectures x layers in {0, 1, 2, 3} against a brute-force statement of the two orders: an interpreter
     runs the list on symbolic buffers and must arrive at the expression the order states; no op's output is its input or residual;
  2. the default architecture's list is the sequence of before, op for op;
  3. the skinny_ln fold rule and the counts flope_tf_last_ln reports;
  4. broken copies of the list are noticed;
  5. tf_gelu_f32 against fp64 on a strided walk of at least 2^24 float32 values of [-16, 16] and the neighbourhoods of 0 and +-2^-20:
     the worst error in units of 2^-23 |x| is what tests/tf_act_bound.py's G comes from; special values;
  6. the same once more as a stand-alone program under -fsanitize=address,undefined (nothing is loaded into Python under a sanitizer);
  7. the new entry points are declared, bound and exported; the Python surface that needs no device.
"""
import ctypes as C
import itertools
import math
import os
import re
import subprocess

import numpy as np
import pytest

import tf_act_bound as AB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIN, LN, ATT = 0, 1, 2
EMB, INP, OUTP, L1, L2, OUTL, N1, N2, NF, AT = range(10)
NONE, X, H, H2, QKV, ATTB, FFB, Y = range(8)
ARCHS = list(itertools.product((0, 1), (1, 2), (0, 1)))
LAYERS = (0, 1, 2, 3)


@pytest.fixture(scope="module")
def Hn():
    path = os.path.join(ROOT, "tests", "host_harness", "libflope_host_tf_arch.so")
    if not os.path.exists(path):
        subprocess.check_call(["make", "-C", ROOT, "tests/host_harness/libflope_host_tf_arch.so"])
    lib = C.CDLL(path)
    lib.tf_arch_h_ops.argtypes = [C.c_int] * 5 + [C.c_void_p, C.c_int]
    lib.tf_arch_h_ln.argtypes = [C.c_int] * 4 + [C.POINTER(C.c_int)] * 2
    lib.tf_arch_h_gelu.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong]
    lib.tf_arch_h_gelu_walk.restype = C.c_double
    lib.tf_arch_h_gelu_walk.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_longlong), C.POINTER(C.c_float)]
    return lib


def ops(Hn, nf, act, fn, nl, broken=0):
    cap = 2 + 7 * nl + 1
    buf = (C.c_int * (8 * cap))()
    n = Hn.tf_arch_h_ops(nf, act, fn, nl, broken, buf, cap)
    assert n <= cap
    return [tuple(buf[8 * i:8 * i + 8]) for i in range(n)]


# ---- 1. the orders, by brute force ---------------------------------------------------------------------------------------------------------
def stated(nf, act, fn, nl):
    """the forward as an expression, straight from the two orders"""
    a = {1: "relu", 2: "gelu"}[act]
    s = "emb(x)"
    for l in range(nl):
        if nf:
            s = f"({s} + out_proj{l}(att{l}(in_proj{l}(ln1_{l}({s})))))"
            s = f"({s} + linear2_{l}({a}(linear1_{l}(ln2_{l}({s})))))"
        else:
            s = f"ln1_{l}(({s} + out_proj{l}(att{l}(in_proj{l}({s})))))"
            s = f"ln2_{l}(({s} + linear2_{l}({a}(linear1_{l}({s})))))"
    if fn:
        s = f"lnf({s})"
    return f"out({s})"


def interpret(oplist):
    """runs an op list on symbolic buffers; checks on the way that no output is the op's input or residual and that nothing unwritten is read"""
    buf = {X: "x"}
    for kind, name, layer, i, r, o, act, fold in oplist:
        assert o not in (i, r) and o != NONE, (kind, name, layer)
        assert i in buf and (r == NONE or r in buf), ("reads an unwritten buffer", kind, name, layer)
        src = buf[i]
        if kind == ATT:
            v = f"att{layer}({src})"
        elif kind == LN:
            v = {N1: f"ln1_{layer}", N2: f"ln2_{layer}", NF: "lnf"}[name] + f"({src})"
            assert r == NONE and act == 0
        else:
            fnm = {EMB: "emb", INP: f"in_proj{layer}", OUTP: f"out_proj{layer}", L1: f"linear1_{layer}", L2: f"linear2_{layer}", OUTL: "out"}[name]
            v = f"{fnm}({src})"
            assert not (act == 2 and r != NONE), "GELU with a residual"
            if r != NONE:
                v = f"({buf[r]} + {v})"
            if act:
                v = {1: "relu", 2: "gelu"}[act] + f"({v})"
        buf[o] = v
    return buf[Y]


@pytest.mark.parametrize("nl", LAYERS)
@pytest.mark.parametrize("arch", ARCHS)
def test_op_list_is_the_stated_order(Hn, arch, nl):
    nf, act, fn = arch
    lst = ops(Hn, nf, act, fn, nl)
    assert len(lst) == Hn.tf_arch_h_count(nf, act, fn, nl) == 2 + 7 * nl + fn
    assert interpret(lst) == stated(nf, act, fn, nl)
    assert [o[6] for o in lst if o[1] == L1] == [act] * nl and all(o[6] == 0 for o in lst if o[1] != L1)
    assert [o[2] for o in lst if o[0] == ATT] == list(range(nl))
    # buffer roles: the wide buffers hold one thing each, the stream lives in h / h2 only
    for kind, name, layer, i, r, o, a, fold in lst:
        if name == INP: assert o == QKV
        if name == AT: assert (i, o) == (QKV, ATTB)
        if name == OUTP: assert i == ATTB
        if name == L1: assert o == FFB
        if name == L2: assert i == FFB
        if kind == LN or name in (OUTP, L2): assert {i, r, o} - {NONE, ATTB, FFB} <= {H, H2}
    assert bool(Hn.tf_arch_h_valid(nf, act, fn)) and bool(Hn.tf_arch_h_default(nf, act, fn)) == (arch == (0, 1, 0))


def test_other_values_are_not_an_architecture(Hn):
    for bad in ((2, 1, 0), (-1, 1, 0), (0, 0, 0), (0, 3, 0), (0, 1, 2), (0, 1, -1)):
        assert not Hn.tf_arch_h_valid(*bad), bad


# ---- 2. the default architecture is the sequence of before ---------------------------------------------------------------------------------
def parent_sequence(nl):
    """run_forward_with as it stood: embedding; per layer in_proj (behind the previous layer's LN2 h2 -> h), attention, out_proj (+ h)
    -> h2, LN1 h2 -> h, linear1 ReLU, linear2 (+ h) -> h2; the last LN2; out_layer"""
    seq = [(LIN, EMB, -1, X, NONE, H, 0)]
    for l in range(nl):
        if l:
            seq.append((LN, N2, l - 1, H2, NONE, H, 0))
        seq += [(LIN, INP, l, H, NONE, QKV, 0), (ATT, AT, l, QKV, NONE, ATTB, 0), (LIN, OUTP, l, ATTB, H, H2, 0), (LN, N1, l, H2, NONE, H, 0),
                (LIN, L1, l, H, NONE, FFB, 1), (LIN, L2, l, FFB, H, H2, 0)]
    if nl:
        seq.append((LN, N2, nl - 1, H2, NONE, H, 0))
    return seq + [(LIN, OUTL, -1, H, NONE, Y, 0)]


@pytest.mark.parametrize("nl", LAYERS)
def test_default_list_is_the_parent_sequence(Hn, nl):
    lst = ops(Hn, 0, 1, 0, nl)
    assert [o[:7] for o in lst] == parent_sequence(nl)
    # ... and the pairs tf_ln_then_linear took: every LN1 with its linear1, every LN2 but the last with the next in_proj
    assert [(o[1], o[2]) for o in lst if o[7]] == sorted([(N1, l) for l in range(nl)] + [(N2, l) for l in range(nl - 1)], key=lambda t: (t[1], t[0]))


# ---- 3. the fold rule ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arch", ARCHS)
def test_fold_rule_and_last_ln_counts(Hn, arch):
    nf, act, fn = arch
    for nl in LAYERS:
        lst = ops(Hn, nf, act, fn, nl)
        for k, o in enumerate(lst):
            if o[7]:                                                     # a folded LayerNorm: a linear with no residual reads its output next
                n = lst[k + 1]
                assert o[0] == LN and n[0] == LIN and n[3] == o[5] and n[4] == NONE and n[1] in (INP, L1) and o[1] != NF
            if o[0] == LN and not o[7]:
                assert o[1] == NF or (not nf and o[1] == N2 and o[2] == nl - 1)
        folded, launched = C.c_int(), C.c_int()
        Hn.tf_arch_h_ln(nf, act, fn, nl, C.byref(folded), C.byref(launched))
        want_folded = 2 * nl if nf else max(2 * nl - 1, 0)
        assert (launched.value, folded.value) == (2 * nl + fn - want_folded, want_folded)
        if nf:
            assert (launched.value, folded.value) == (1 if fn else 0, 2 * nl)      # enc.last_ln under pre-norm and skinny_ln = 1


# ---- 4. broken copies ----------------------------------------------------------------------------------------------------------------------
def test_broken_lists_are_noticed(Hn):
    for nf, act, fn in ARCHS:
        for nl in (1, 2, 3):
            for broken in (1, 2, 3):
                applies = {1: nf, 2: nf, 3: fn}[broken]            # LN2 stands directly in front of linear1 in pre-norm only
                lst = ops(Hn, nf, act, fn, nl, broken)
                try:
                    same = interpret(lst) == stated(nf, act, fn, nl)
                except AssertionError:
                    same = False
                assert same == (not applies), (nf, act, fn, nl, broken)


# ---- 5. the GELU ---------------------------------------------------------------------------------------------------------------------------
def walk(Hn, lo, hi, stride):
    n, wx = C.c_longlong(), C.c_float()
    w = Hn.tf_arch_h_gelu_walk(lo, hi, stride, C.byref(n), C.byref(wx))
    return w, n.value, wx.value


def test_gelu_measured_against_fp64(Hn):
    bits16 = int(np.float32(16.0).view(np.uint32))
    worst, n, wx = walk(Hn, 1, bits16, 128)                              # every 128th float32 of (0, 16], both signs
    assert n >= 2 ** 24
    w0, n0, _ = walk(Hn, 1, 1 << 16, 1)                                  # the 2^16 values next to zero, both signs
    b20 = int(np.float32(2.0 ** -20).view(np.uint32))
    w20, n20, _ = walk(Hn, b20 - 4096, b20 + 4096, 1)                    # ... and around +-2^-20 (the function has no break points)
    worst = max(worst, w0, w20)
    print(f"tf_gelu_f32: worst error {worst:.4f} x 2^-23 |x| at x = {wx!r} over {n + n0 + n20} points; G_WORST = {AB.G_WORST}, G = {AB.G}")
    assert worst <= AB.G_WORST and math.ceil(worst) == math.ceil(AB.G_WORST) and AB.G == 2 * math.ceil(worst)


def test_the_harness_reference_is_math_erf(Hn):
    """the walk's fp64 reference against math.erf, and the harness's function against the emulation tests/tf_act_bound.py uses"""
    import torch
    Hn.tf_arch_h_gelu64.restype, Hn.tf_arch_h_gelu64.argtypes = C.c_double, [C.c_double]
    rng = np.random.default_rng(3)
    x = np.concatenate([rng.uniform(-16, 16, 20000), rng.standard_normal(20000) * 1e-3]).astype(np.float32)
    for v in x[:4000]:
        ref = 0.5 * float(v) * (1.0 + math.erf(float(v) / math.sqrt(2.0)))
        assert abs(Hn.tf_arch_h_gelu64(float(v)) - ref) <= 4e-16 * abs(float(v))
    y = np.empty_like(x)
    Hn.tf_arch_h_gelu(x.ctypes.data, y.ctypes.data, x.size)
    emu = AB.gelu_f32(torch.from_numpy(x)).numpy()
    ref = AB.gelu64(torch.from_numpy(x)).numpy()
    assert (np.abs(emu.astype(np.float64) - y) <= 2.0 ** -23 * np.abs(x)).all()          # the two differ by the fma's double rounding at most
    assert (np.abs(y - ref) <= AB.G_WORST * 2.0 ** -23 * np.abs(x) + 2.0 ** -149).all()


def test_gelu_special_values(Hn):
    x = np.array([0.0, -0.0, np.nan, np.inf, -np.inf, 3e38, -3e38, 20.0, -20.0, 1e-45, -1e-45, 1.0], dtype=np.float32)
    y = np.empty_like(x)
    Hn.tf_arch_h_gelu(x.ctypes.data, y.ctypes.data, x.size)
    assert y[0] == 0 and y[1] == 0 and np.isnan(y[2]) and y[3] == np.inf
    assert not (np.isfinite(y[4]) and y[4] != 0)                         # no finite non-zero result from a non-finite argument
    assert y[5] == x[5] and y[6] == 0 and y[7] == 20.0 and y[8] == 0 and abs(y[11] - 0.8413447) < 1e-6
    assert abs(float(y[9])) <= 1.5e-45 and abs(float(y[10])) <= 1.5e-45


# ---- 6. the same under AddressSanitizer + UBSan, as a program of its own ---------------------------------------------------------------------
def test_stand_alone_program_under_sanitizers(tmp_path):
    exe = str(tmp_path / "tf_arch_selfcheck")
    subprocess.check_call(["g++", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DTF_ARCH_MAIN",
                           "-std=c++17", "-I" + os.path.join(ROOT, "flope_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "host_harness", "harness_tf_arch.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "128 lists" in r.stdout and " 0 failures" in r.stdout


# ---- 7. the surface --------------------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_bound_and_exported():
    from flope_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "flope_amd.h")).read()
    for name in ("flope_tf_linear_act", "flope_tf_linear_ln_act"):
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert re.search(r"#define FLOPE_TF_ACT_RELU\s+1\b", header) and re.search(r"#define FLOPE_TF_ACT_GELU\s+2\b", header)
    assert (_lib.TF_ACT_RELU, _lib.TF_ACT_GELU) == (1, 2)
    for opt in ('"norm_first"', '"activation"', '"final_norm"'):
        assert opt in header, opt


def test_python_surface_without_a_device():
    import inspect
    from flope_amd.tf_encoder import TransformerEncoder, check_arch, expected_keys
    p = inspect.signature(TransformerEncoder.__init__).parameters
    assert (p["norm_first"].default, p["activation"].default, p["final_norm"].default, p["layer_norm_eps"].default) == (False, "relu", False, 1e-5)
    assert inspect.signature(TransformerEncoder.linear).parameters["act"].default is None
    assert "act" in inspect.signature(TransformerEncoder.linear_ln_act).parameters
    assert check_arch() == {"norm_first": False, "activation": "relu", "final_norm": False}
    import torch.nn.functional as F
    for kw in ({"activation": "gelu_tanh"}, {"activation": "tanh"}, {"activation": F.gelu}, {"activation": None}, {"layer_norm_eps": 1e-6},
               {"layer_norm_eps": 1e-12}, {"norm_first": 2}, {"final_norm": "yes"}):
        with pytest.raises(ValueError):
            check_arch(**kw)
        with pytest.raises(ValueError):                                  # the constructor refuses them before it looks for a device
            TransformerEncoder(16, 128, 9, 2, 1, 256, **kw)
    assert expected_keys(2) == expected_keys(2, False) and len(expected_keys(2, True)) == len(expected_keys(2)) + 2
    assert TransformerEncoder._act_id(False, None) == 0 and TransformerEncoder._act_id(True, None) == 1 and TransformerEncoder._act_id(True, "relu") == 1
    assert TransformerEncoder._act_id(False, "gelu") == 2
    for bad in ((True, "gelu"), (False, "tanh"), (False, 2)):
        with pytest.raises(ValueError):
            TransformerEncoder._act_id(*bad)
