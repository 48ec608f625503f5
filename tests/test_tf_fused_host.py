"""The encoder's single-launch forward (option fused) without a device: the planner of flope_amd/csrc/tf_fused_plan.h
through tests/host_harness/harness_tf_fused.cpp --

  1. eligibility over the table of shapes the GPU test runs (eight fit 64 KiB of LDS, `big` does not), and its three switches;
  2. the LDS layout: total non-decreasing in L, no two buffers that are live in one phase overlap, every buffer inside total;
  3. the rule that sends a linear to the rowwave summation order;
  4. the scalar walk of the kernel through that layout, every LDS and global index checked, against the fp64 oracle per sequence
     at 1e-5 (the project's bound for float32 against the reference fixture; the oracle's own float32 evaluation is within 2.3e-7 of
     its fp64 one at these shapes).  The walk is a rehearsal of offsets and aliasing, not a bit oracle: libm's exp is not the device's.
"""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT_BF16, DT_F16, DT_F32 = 0, 1, 2
LDS = 64 * 1024

# name: ((in, d, out, heads, layers, ff), B, L, eligible)
CASES = {
    "toy": ((16, 32, 9, 4, 2, 64), 8, 10, True),
    "one": ((16, 32, 9, 4, 2, 64), 1, 1, True),
    "long": ((8, 16, 9, 2, 2, 32), 2, 70, True),
    "wide": ((12, 80, 7, 5, 1, 96), 3, 5, True),
    "odd": ((5, 21, 3, 3, 2, 13), 4, 9, True),
    "tiny": ((3, 4, 2, 2, 1, 8), 3, 7, True),
    "nolayer": ((6, 8, 5, 2, 0, 8), 2, 4, True),
    "many": ((16, 32, 9, 4, 1, 64), 600, 3, True),
    "big": ((16, 128, 9, 2, 1, 128), 2, 300, False),
}
ELIGIBLE = [k for k, v in CASES.items() if v[3]]
TOY_LENGTHS = [10, 1, 3, 7, 10, 2, 9, 5]
BUFFERS = ["h", "h2", "x", "qkv", "att", "sc", "ffb"]


def case_data(name):
    """(dims, state dict, x [B, L, in]) of a case: the toy on the reference fixture's weights, every other on synthetic ones"""
    from oracle import tf_encoder_ref as T
    dims, B, L, _ = CASES[name]
    if name == "toy":
        f = np.load(os.path.join(ROOT, "tests", "golden", "reference_fixtures.npz"))
        sd = {k[len("tf_sd::"):]: f[k] for k in f.files if k.startswith("tf_sd::")}
    else:
        sd = T.synthetic_state_dict(dims[0], dims[1], dims[2], dims[4], dims[5], seed=5)
    x = np.random.default_rng(1).standard_normal((B, L, dims[0])).astype(np.float32)
    return dims, sd, x


@pytest.fixture(scope="module")
def hz():
    path = os.path.join(ROOT, "tests", "host_harness", "libflope_host_tf_fused.so")
    if not os.path.exists(path):
        subprocess.check_call(["make", "-C", ROOT, "tests/host_harness/libflope_host_tf_fused.so"])
    lib = C.CDLL(path)
    lib.tf_fused_lds_limit.restype = C.c_long
    lib.tf_fused_walk.restype = C.c_long
    return lib


def layout(hz, in_dim, d, ff, L):
    o = (C.c_long * 10)()
    hz.tf_fused_layout(in_dim, d, ff, L, o)
    v = list(o)
    return dict(zip(BUFFERS, v[:7])), v[7], v[8], v[9]


def sizes(hz, in_dim, d, ff, L):
    o = (C.c_long * 7)()
    hz.tf_fused_buffer_bytes(in_dim, d, ff, L, o)
    return dict(zip(BUFFERS, list(o)))


# ---- 1. eligibility ---------------------------------------------------------------------------------------------------------------
def test_limit_is_64_kib(hz):
    assert hz.tf_fused_lds_limit() == LDS and hz.tf_fused_waves() == 4


@pytest.mark.parametrize("name", list(CASES))
def test_eligibility_over_the_table(hz, name):
    (i, d, _, _, _, ff), _, L, want = CASES[name]
    assert bool(hz.tf_fused_ok(DT_F32, 1, 0, i, d, ff, L)) is want
    total = layout(hz, i, d, ff, L)[3]
    assert (total <= LDS) is want
    naive = 4 * L * (i + 3 * d + 3 * d + ff + 4)            # no aliasing at all: x, h, h2, qkv, att, ffb, four score rows
    print(f"{name}: layout {total} B, without aliasing {naive} B")
    assert total <= naive + 4 * L                          # (at most one pad float per qkv row on top)
    if want:
        assert naive < 40 * 1024
    else:
        assert naive > 800 * 1024


def test_eligibility_switches(hz):
    (i, d, _, _, _, ff), _, L, _ = CASES["toy"]
    assert hz.tf_fused_ok(DT_F32, 1, 0, i, d, ff, L) == 1
    assert hz.tf_fused_ok(DT_F16, 1, 0, i, d, ff, L) == 0
    assert hz.tf_fused_ok(DT_BF16, 1, 0, i, d, ff, L) == 0
    assert hz.tf_fused_ok(DT_F32, 0, 0, i, d, ff, L) == 0
    assert hz.tf_fused_ok(DT_F32, 1, 1, i, d, ff, L) == 0
    assert hz.tf_fused_ok(DT_F32, 2, 0, i, d, ff, L) == 0           # the option is 0 or 1
    assert hz.tf_fused_ok(DT_F32, 1, 0, i, d, ff, 0) == 0           # no sequence
    # the threshold is the layout's total, exactly
    fits = [L for L in range(1, 400) if hz.tf_fused_ok(DT_F32, 1, 0, i, d, ff, L)]
    assert fits == list(range(1, fits[-1] + 1))
    assert layout(hz, i, d, ff, fits[-1])[3] <= LDS < layout(hz, i, d, ff, fits[-1] + 1)[3]


# ---- 2. the layout ----------------------------------------------------------------------------------------------------------------
DIMS = sorted({(v[0][0], v[0][1], v[0][5]) for v in CASES.values()} | {(1, 1, 1), (64, 64, 256), (7, 384, 1536)})


@pytest.mark.parametrize("dims", DIMS, ids=str)
def test_total_is_non_decreasing_in_length(hz, dims):
    prev = -1
    for L in list(range(0, 130)) + [255, 256, 257, 1000, 4096, 100000, 2 ** 31 - 1]:
        total = layout(hz, *dims, L)[3]
        assert total >= prev, (dims, L)
        prev = total


@pytest.mark.parametrize("dims", DIMS, ids=str)
def test_live_buffers_never_overlap(hz, dims):
    nph = hz.tf_fused_phases()
    assert nph == 10
    live = [hz.tf_fused_live(p) for p in range(nph)]
    assert all(m > 0 for m in live) and hz.tf_fused_live(nph) == -1
    seen = 0
    for m in live:
        seen |= m
    assert seen == (1 << len(BUFFERS)) - 1, "a buffer no phase uses"
    for L in (1, 2, 7, 10, 64, 65, 70):
        off, qld, scfl, total = layout(hz, *dims, L)
        if total > LDS:
            continue
        sz = sizes(hz, *dims, L)
        assert qld >= 3 * dims[1] and qld % 2 == 1 and scfl >= L and sz["sc"] == 4 * hz.tf_fused_waves() * scfl     # one score row per wave
        for name in BUFFERS:
            assert off[name] % 4 == 0 and off[name] + sz[name] <= total, (name, L)
        for p, m in enumerate(live):
            names = [n for i, n in enumerate(BUFFERS) if m >> i & 1]
            for a, b in itertools.combinations(names, 2):
                assert off[a] + sz[a] <= off[b] or off[b] + sz[b] <= off[a], f"phase {p}: {a} and {b} overlap at L = {L}"
    # the aliasing the layout exists for: the three tenants of the shared region do share it
    off = layout(hz, *dims, 10)[0]
    assert off["x"] == off["qkv"] == off["ffb"]


# ---- 3. the order rule ------------------------------------------------------------------------------------------------------------
def test_rowwave_order_rule(hz):
    assert [hz.tf_fused_rowwave_order(n, r) for n, r in ((9, 0), (16, 0), (17, 0), (4, 1))] == [1, 1, 0, 0]


# ---- 4. the walk ------------------------------------------------------------------------------------------------------------------
def run_walk(hz, dims, sd, x, lengths=None):
    from flope_amd.tf_encoder import expected_keys
    i, d, o, H, nl, ff = dims
    B, L = x.shape[0], x.shape[1]
    keys = expected_keys(nl)
    order = keys[:2] + keys[-2:]
    for l in range(nl):
        p = f"transformer_encoder.layers.{l}."
        order += [p + s for s in ("self_attn.in_proj_weight", "self_attn.in_proj_bias", "self_attn.out_proj.weight", "self_attn.out_proj.bias",
                                  "linear1.weight", "linear1.bias", "linear2.weight", "linear2.bias", "norm1.weight", "norm1.bias",
                                  "norm2.weight", "norm2.bias")]
    arrs = [np.ascontiguousarray(sd[k], dtype=np.float32) for k in order]
    tab = (C.c_void_p * len(arrs))(*[a.ctypes.data for a in arrs])
    tab_n = (C.c_long * len(arrs))(*[a.size for a in arrs])
    xc = np.ascontiguousarray(x, dtype=np.float32)
    y = np.full((B, L, o), np.nan, dtype=np.float32)
    lh = None if lengths is None else (C.c_int * B)(*lengths)
    bad = hz.tf_fused_walk(xc.ctypes.data_as(C.c_void_p), y.ctypes.data_as(C.c_void_p), lh, B, L, i, d, o, H, nl, ff, tab, tab_n)
    return bad, y


@pytest.mark.parametrize("name", ELIGIBLE)
def test_walk_matches_the_oracle_with_every_index_checked(hz, name):
    from oracle import tf_encoder_ref as T
    dims, sd, x = case_data(name)
    bad, y = run_walk(hz, dims, sd, x)
    assert bad == 0, f"{bad} accesses outside the layout or an array"
    ref = T.forward(sd, x, num_heads=dims[3])
    err = np.abs(y - ref).reshape(x.shape[0], -1).max(axis=1)
    print(f"{name}: walk vs fp64 oracle, worst sequence {err.max():.2e}")
    assert np.isfinite(y).all() and (err < 1e-5).all()
    # the rowwave rule as this shape meets it (what the GPU test's table says each case trips)
    rw = lambda n, r: bool(hz.tf_fused_rowwave_order(n, r))
    if name == "tiny":
        assert rw(dims[1], 0) and rw(3 * dims[1], 0) and rw(dims[5], 0) and not rw(dims[1], 1)
    if name == "odd":
        assert rw(dims[5], 0) and not rw(dims[1], 0)


def test_walk_of_a_ragged_toy_batch(hz):
    from oracle import tf_encoder_ref as T
    dims, sd, x = case_data("toy")
    xn = x.copy()
    for b, n in enumerate(TOY_LENGTHS):
        xn[b, n:] = np.nan                                   # padding is never read
    bad, y = run_walk(hz, dims, sd, xn, TOY_LENGTHS)
    assert bad == 0
    bias = np.asarray(sd["out_layer.bias"], dtype=np.float32)
    worst = 0.0
    for b, n in enumerate(TOY_LENGTHS):
        ref = T.forward(sd, x[b:b + 1, :n], num_heads=dims[3])[0]
        e = float(np.abs(y[b, :n] - ref).max())
        assert e < 1e-5, (b, n, e)
        worst = max(worst, e)
        assert np.array_equal(y[b, n:].view(np.int32), np.broadcast_to(bias, (x.shape[1] - n, bias.size)).view(np.int32))
    print(f"ragged toy: walk vs fp64 oracle per sequence {worst:.2e}")
    # equal lengths are the fixed-length walk
    assert np.array_equal(run_walk(hz, dims, sd, x, [x.shape[1]] * x.shape[0])[1].view(np.int32), run_walk(hz, dims, sd, x)[1].view(np.int32))


def test_walk_refuses_what_the_kernel_is_never_given(hz):
    dims, sd, x = case_data("toy")
    assert run_walk(hz, dims, sd, x, [10, 0, 3, 7, 10, 2, 9, 5])[0] == -2
    assert run_walk(hz, dims, sd, x, [10, 11, 3, 7, 10, 2, 9, 5])[0] == -2
    from oracle import tf_encoder_ref as T
    bdims, B, L, _ = CASES["big"]
    bsd = T.synthetic_state_dict(bdims[0], bdims[1], bdims[2], bdims[4], bdims[5], seed=5)
    assert run_walk(hz, bdims, bsd, np.zeros((B, L, bdims[0]), dtype=np.float32))[0] == -1


# ---- the C-ABI ---------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_and_exported():
    import re
    from flope_amd import _lib
    header = open(os.path.join(ROOT, "include", "flope_amd.h")).read()
    assert "flope_tf_forward_plan" in set(re.findall(r"\b(flope_[a-z0-9_]+)\s*\(", header))
    assert re.search(r"#define\s+FLOPE_TF_FWD_LAUNCHES\s+0\b", header) and re.search(r"#define\s+FLOPE_TF_FWD_FUSED\s+1\b", header)
    assert (_lib.TF_FWD_LAUNCHES, _lib.TF_FWD_FUSED) == (0, 1)
    for name in ("flope_tf_forward_plan", "flope_tf_last_forward"):
        assert name in set(re.findall(r"\b(flope_[a-z0-9_]+)\s*\(", header)), name
        assert name in _lib.SIGNATURES and hasattr(_lib.load(), name), name
