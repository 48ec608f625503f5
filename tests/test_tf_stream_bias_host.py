"""A stream state's distance table without a device (flope_amd/csrc/tf_encoder_stream.h through
tests/host_harness/harness_tf_stream_bias.cpp, flope_amd/tf_encoder.py):

  1. the header's helpers against brute force in numpy on random (capacity, window, planes, D): the distances a state needs, the
     planes check, the first non-finite entry and the open's refusals with the named (plane, distance), the entry of every (L, j), the
     keys <= D test the kernels make;
  2. every refusal by hand, and NULL arguments;
  3. the two new symbols in _lib.SIGNATURES and the new defines in the header;
  4. distance_bias against a triple loop, against alibi_bias in bits, and its windowed allowed set against what _mask_window
     recognises as a causal band;
  5. an independent fp64 restatement of a biased stream -- one token at a time, a k / v list per layer, a ring of `capacity` rows at
     p % capacity, distance p - j -- against tf_attn_bias_bound.biased_forward on the expanded bias, to 1e-12 relative;
  6. the helper properties once more in a stand-alone program with its own main under -fsanitize=address,undefined, compiled and run
     here as a child process (nothing is loaded into Python under a sanitizer).
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import tf_attn_bias_bound as BB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
i32p, f32p = C.POINTER(C.c_int), C.POINTER(C.c_float)
OK, PLANES, DISTANCES, NULL, VALUE = 0, -10, -11, -12, -13
BAD = [np.float32(np.nan), np.float32(np.inf), np.float32(-np.inf)]


@pytest.fixture(scope="module")
def H():
    path = os.path.join(ROOT, "tests", "host_harness", "libflope_host_tf_stream_bias.so")
    if not os.path.exists(path):
        subprocess.check_call(["make", "-C", ROOT, "tests/host_harness/libflope_host_tf_stream_bias.so"])
    lib = C.CDLL(path)
    lib.tf_sbias_bytes.restype = C.c_long
    return lib


def fp(a):
    return a.ctypes.data_as(f32p)


def found(H, rel):
    out = (C.c_int * 2)(-7, -7)
    return H.tf_sbias_nonfinite(fp(rel), rel.shape[0], rel.shape[1], out), tuple(out)


def check_open(H, capacity, window, heads, planes, distances, rel):
    out = (C.c_int * 2)(-7, -7)
    return H.tf_sbias_check_open(capacity, window, heads, planes, distances, None if rel is None else fp(rel), out), tuple(out)


# ---- 1. against brute force -----------------------------------------------------------------------------------------------------------
def test_helpers_against_brute_force(H):
    assert [H.tf_sbias_code(i) for i in range(5)] == [OK, PLANES, DISTANCES, NULL, VALUE]
    rng = np.random.default_rng(8)
    n = 0
    for rep in range(1500):
        capacity = int(rng.integers(1, 300))
        window = int(rng.integers(1, capacity + 1)) if rep % 3 else 0
        heads = int(rng.integers(1, 9))
        planes = heads if rep % 2 else 1
        D = window if window else capacity
        assert H.tf_sbias_distances(capacity, window) == D
        for p in range(-1, 11):
            assert H.tf_sbias_planes_ok(p, heads) == int(p == 1 or p == heads), (p, heads)
        rel = np.ascontiguousarray((2 * rng.standard_normal((planes, D))).astype(np.float32))
        assert H.tf_sbias_bytes(planes, D) == rel.nbytes
        assert found(H, rel) == (0, (-7, -7))
        assert check_open(H, capacity, window, heads, planes, D, rel) == (OK, (-7, -7))
        # a few non-finite entries anywhere: the first in (plane, distance) order is named
        wrong = rng.random(rel.shape) < 2.0 / rel.size
        wrong.reshape(-1)[rng.integers(rel.size)] = True
        bad = rel.copy()
        bad[wrong] = rng.choice(BAD, size=int(wrong.sum()))
        first = tuple(int(v) for v in np.unravel_index(np.flatnonzero(wrong.reshape(-1))[0], wrong.shape))
        assert found(H, bad) == (1, first)
        assert check_open(H, capacity, window, heads, planes, D, bad) == (VALUE, first)
        # the refusals in front of the values, in their order, name nothing
        other = int(rng.choice([p for p in range(-1, 12) if p != 1 and p != heads]))
        assert check_open(H, capacity, window, heads, other, D + 1, None) == (PLANES, (-7, -7))
        wrong_d = int(rng.choice([d for d in (D - 1, D + 1, capacity + 1, 0, window + capacity) if d != D]))
        assert check_open(H, capacity, window, heads, planes, wrong_d, None) == (DISTANCES, (-7, -7))
        assert check_open(H, capacity, window, heads, planes, D, None) == (NULL, (-7, -7))
        # the entry of every (L, j) a query of this state can have, and the test in front of the kernels' first load
        for pos in {0, D - 1, D, capacity - 1, int(rng.integers(0, 10 * capacity))}:
            if not window and pos >= capacity:
                continue
            lo = max(0, pos + 1 - window) if window else 0
            L = pos - lo + 1
            assert H.tf_sbias_step_keys(pos, window) == L and H.tf_sbias_keys_ok(L, D) == 1
            idx = np.array([H.tf_sbias_index(L, j) for j in range(L)])
            assert np.array_equal(idx, pos - (lo + np.arange(L))) and idx.min() == 0 and idx.max() == L - 1 <= D - 1
            ln = int(rng.integers(1, 9))
            if window or pos + ln <= capacity:
                keys = H.tf_sbias_extend_keys(pos, ln, window)
                assert keys == (min(pos + ln, window) if window else pos + ln) and H.tf_sbias_keys_ok(keys, D) == 1
        for keys in (0, 1, D - 1, D, D + 1, 2 * D + 3):
            assert H.tf_sbias_keys_ok(keys, D) == int(keys <= D)
        n += 1
    assert n == 1500


# ---- 2. by hand -----------------------------------------------------------------------------------------------------------------------
def test_each_refusal_by_hand(H):
    t = np.zeros((4, 36), dtype=np.float32)
    assert check_open(H, 40, 36, 4, 4, 36, t) == (OK, (-7, -7)) and check_open(H, 36, 0, 4, 4, 36, t) == (OK, (-7, -7))
    assert check_open(H, 40, 36, 4, 1, 36, t[:1].copy()) == (OK, (-7, -7))
    assert check_open(H, 40, 36, 4, 2, 36, t)[0] == PLANES and check_open(H, 40, 36, 4, 0, 36, t)[0] == PLANES
    assert check_open(H, 40, 36, 4, 4, 40, t)[0] == DISTANCES                       # a windowed state needs its window, not its capacity
    assert check_open(H, 40, 0, 4, 4, 36, t)[0] == DISTANCES                        # ... and a linear one its capacity
    assert check_open(H, 40, 36, 4, 4, 36, None)[0] == NULL
    for v in BAD:                                                                   # -inf is no way to mask here
        c = t.copy(); c[2, 7] = v
        assert check_open(H, 40, 36, 4, 4, 36, c) == (VALUE, (2, 7)) and found(H, c) == (1, (2, 7))
        c[1, 35] = np.nan                                                           # an earlier plane wins
        assert found(H, c) == (1, (1, 35))
        c[1, 0] = np.inf                                                            # an earlier distance of it wins
        assert found(H, c) == (1, (1, 0))
    big = np.full((1, 5), np.float32(-3.0e38))                                      # a huge finite value is a value
    big[0, 1] = np.float32(1e-45); big[0, 2] = -0.0                                 # and so are a denormal and a signed zero
    assert found(H, big) == (0, (-7, -7))
    assert [H.tf_sbias_index(5, j) for j in range(5)] == [4, 3, 2, 1, 0]            # the query's own key has distance 0
    assert H.tf_sbias_keys_ok(36, 36) == 1 and H.tf_sbias_keys_ok(37, 36) == 0
    assert H.tf_sbias_step_id() == 2 and H.tf_sbias_extend_id() == 3


def test_null_arguments(H):
    out = (C.c_int * 2)(-7, -7)
    t = np.zeros((1, 2), dtype=np.float32)
    assert H.tf_sbias_nonfinite(None, 1, 2, out) == -1 and H.tf_sbias_nonfinite(fp(t), 1, 2, None) == -1
    assert H.tf_sbias_check_open(4, 2, 1, 1, 2, fp(t), None) == 1
    assert tuple(out) == (-7, -7)


# ---- 3. the binding ---------------------------------------------------------------------------------------------------------------------
def test_signatures_and_defines():
    from flope_amd import _lib
    sig = _lib.SIGNATURES["flope_tf_stream_open_bias"]
    assert sig[0] is C.c_int and len(sig[1]) == 8 and sig[1][6] == f32p
    assert _lib.SIGNATURES["flope_tf_stream_bias_planes"] == (C.c_int, [C.c_void_p])
    assert (_lib.TF_STEP_BIASED, _lib.TF_EXTEND_BIASED) == (2, 3)
    header = open(os.path.join(ROOT, "include", "flope_amd.h")).read()
    assert "int flope_tf_stream_open_bias(flope_tf_handle h, int tracks, int capacity, int window, int planes, int distances, const float* table_host," in header
    assert "int flope_tf_stream_bias_planes(flope_tf_stream s);" in header
    assert "#define FLOPE_TF_STEP_BIASED      2" in header and "#define FLOPE_TF_EXTEND_BIASED    3" in header
    # the ids that were there stay as they were
    assert "#define FLOPE_TF_STEP_ROW         0" in header and "#define FLOPE_TF_STEP_SPLIT       1" in header
    assert "#define FLOPE_TF_EXTEND_ROW       0" in header and "#define FLOPE_TF_EXTEND_MFMA      2" in header


# ---- 4. distance_bias -------------------------------------------------------------------------------------------------------------------
def test_distance_bias_against_a_triple_loop():
    import torch
    from flope_amd.tf_encoder import distance_bias
    g = torch.Generator().manual_seed(3)
    for L, W, D, planes in ((1, 0, 1, 1), (7, 0, 7, 4), (7, 0, 12, 1), (9, 4, 4, 2), (9, 4, 9, 1), (6, 9, 6, 3), (15, 1, 1, 1)):
        table = torch.randn(planes, D, generator=g)
        b = distance_bias(table, L, window=W)
        assert b.dtype == torch.float32 and tuple(b.shape) == (planes, L, L) and b.is_contiguous()
        for h in range(planes):
            for i in range(L):
                for j in range(L):
                    seen = j <= i and (not W or i - j < W)
                    assert b[h, i, j].item() == (table[h, i - j].item() if seen else float("-inf")), (L, W, h, i, j)
    assert tuple(distance_bias(torch.zeros(5), 5).shape) == (1, 5, 5)                # a [D] table is one plane
    assert distance_bias(torch.zeros(2, 5, dtype=torch.float64), 3).dtype == torch.float32
    for call, msg in ((lambda: distance_bias(torch.zeros(2, 4), 5), "table has 4 distances, a forward of L = 5 needs 5"),
                      (lambda: distance_bias(torch.zeros(2, 3), 9, window=4), "under window = 4 needs 4"),
                      (lambda: distance_bias(torch.zeros(2, 3, 3), 3), "table must be a floating tensor"),
                      (lambda: distance_bias(torch.zeros(3, dtype=torch.int64), 3), "table must be a floating tensor"),
                      (lambda: distance_bias(torch.zeros(3), 0), "L must be positive"),
                      (lambda: distance_bias(torch.zeros(3), 3, window=-1), "L must be positive")):
        with pytest.raises(ValueError, match=msg):
            call()


def test_alibi_distances_expand_to_alibi_bias_in_bits():
    import torch
    from flope_amd.tf_encoder import alibi_bias, alibi_distances, distance_bias
    slopes = [2.0 ** -(h + 1) for h in range(4)] + [0.3, 1e-3]
    for L in (1, 2, 15, 33, 130):
        t = alibi_distances(L, slopes)
        assert t.dtype == torch.float32 and tuple(t.shape) == (len(slopes), L)
        for h, s in enumerate(slopes):
            assert np.array_equal(t[h].numpy(), -np.float32(s) * np.arange(L, dtype=np.float32))
        got, want = distance_bias(t, L), alibi_bias(L, slopes)
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), L
    assert tuple(alibi_distances(7, [0.5]).shape) == (1, 7) and tuple(alibi_distances(7, torch.tensor([0.5, 0.25])).shape) == (2, 7)


def test_windowed_allowed_set_is_the_causal_band():
    import torch
    from flope_amd.tf_encoder import _mask_window, distance_bias
    for L in (2, 9, 33):
        for W in range(1, L + 3):
            b = distance_bias(torch.zeros(1, max(L, W)), L, window=W)[0]
            # the float mask torch would take: 0 where allowed, -inf elsewhere; a window that covers the sequence is the causal mask
            assert _mask_window(b, L) == (True, W if W < L else 0), (L, W)
        assert _mask_window(distance_bias(torch.zeros(L), L)[0], L) == (True, 0)


# ---- 5. an independent restatement of the stream ----------------------------------------------------------------------------------------
def _ln(x, w, b):
    mu = x.mean()
    return (x - mu) / np.sqrt(((x - mu) ** 2).mean() + 1e-5) * w + b


def stream64(sd, x, table, capacity, window, num_heads):
    """One track, one token at a time, in fp64: per layer a ring of `capacity` (k, v) rows at p % capacity; the query at p scores the
    keys lo .. p (lo = max(0, p + 1 - window), 0 without a window) as q . k / sqrt(hd) + table[h or 0][p - j].  Written from the
    semantics, not from tf_attn_bias_bound.biased_forward: no [L, L] matrix, no mask."""
    g = lambda k: np.asarray(sd[k], dtype=np.float64)
    table = np.asarray(table, dtype=np.float64)
    nl = 0
    while f"transformer_encoder.layers.{nl}.norm1.weight" in sd:
        nl += 1
    ring = [[None] * capacity for _ in range(nl)]
    out = []
    for p in range(x.shape[0]):
        assert window or p < capacity
        h = g("embedding.weight") @ np.asarray(x[p], dtype=np.float64) + g("embedding.bias")
        d = h.shape[0]
        hd = d // num_heads
        lo = max(0, p + 1 - window) if window else 0
        for i in range(nl):
            pre = f"transformer_encoder.layers.{i}."
            qkv = g(pre + "self_attn.in_proj_weight") @ h + g(pre + "self_attn.in_proj_bias")
            q, k, v = qkv[:d], qkv[d:2 * d], qkv[2 * d:]
            ring[i][p % capacity] = (k, v)
            att = np.zeros(d)
            for hh in range(num_heads):
                sl = slice(hh * hd, (hh + 1) * hd)
                plane = table[hh if table.shape[0] > 1 else 0]
                s = np.array([q[sl] @ ring[i][j % capacity][0][sl] / np.sqrt(hd) + plane[p - j] for j in range(lo, p + 1)])
                w = np.exp(s - s.max())
                w /= w.sum()
                for wj, j in zip(w, range(lo, p + 1)):
                    att[sl] += wj * ring[i][j % capacity][1][sl]
            a = g(pre + "self_attn.out_proj.weight") @ att + g(pre + "self_attn.out_proj.bias")
            h = _ln(h + a, g(pre + "norm1.weight"), g(pre + "norm1.bias"))
            f = g(pre + "linear2.weight") @ np.maximum(g(pre + "linear1.weight") @ h + g(pre + "linear1.bias"), 0) + g(pre + "linear2.bias")
            h = _ln(h + f, g(pre + "norm2.weight"), g(pre + "norm2.bias"))
        out.append(g("out_layer.weight") @ h + g("out_layer.bias"))
    return np.stack(out)


@pytest.mark.parametrize("capacity,window", [(15, 0), (8, 5)])
def test_stream_restatement_against_the_biased_forward(capacity, window):
    import torch
    from flope_amd.tf_encoder import alibi_distances, distance_bias
    f = np.load(os.path.join(ROOT, "tests", "golden", "tf_bias_fixture.npz"))
    sd = {k[4:]: f[k] for k in f.files if k.startswith("sd::")}
    x = f["x"][:3]
    L, heads = x.shape[1], 4
    D = window or capacity
    tables = {"alibi_h": alibi_distances(D, [2.0 ** -(h + 1) for h in range(heads)]),
              "rand_1": 2 * torch.randn(1, D, generator=torch.Generator().manual_seed(5)),
              "rand_h": 2 * torch.randn(heads, D, generator=torch.Generator().manual_seed(6))}
    for name, table in tables.items():
        want = BB.biased_forward(sd, x, distance_bias(table, L, window=window).numpy(), num_heads=heads)
        for b in range(x.shape[0]):
            got = stream64(sd, x[b], table.numpy(), capacity, window, heads)
            rel = float(np.abs(got - want[b]).max() / np.abs(want[b]).max())
            assert rel < 1e-12, (name, b, rel)
    # the fixture's own ALiBi output: the restated stream is the reference module's causal forward under that float mask
    if not window:
        assert np.array_equal(distance_bias(tables["alibi_h"], L).numpy(), f["bias_alibi_h"])
        got = stream64(sd, x[0], tables["alibi_h"].numpy(), capacity, window, heads)
        assert float(np.abs(got - f["y_alibi_h"][0]).max()) < 1e-5


# ---- 6. the same under AddressSanitizer + UBSan, as a program of its own --------------------------------------------------------------
def test_stand_alone_program_under_sanitizers(tmp_path):
    """the host functions once in a stand-alone program of its own (host code only, nothing loaded into python)"""
    exe = str(tmp_path / "tf_stream_bias_selfcheck")
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DTF_STREAM_BIAS_MAIN", "-std=c++17",
                           "-I" + os.path.join(ROOT, "flope_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "host_harness", "harness_tf_stream_bias.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "400 tables, 0 failures" in r.stdout
