"""The element-wise checker of the encoder's linears and LayerNorms (tests/tf_linear_bound.py) must bite: it passes an honest
float32 emulation of each operation, in three summation orders, on every case the device test uses, and fails copies of that
emulation broken the way kernels break, one defect at a time, on at least one of those cases.  CPU only; the same references and
bounds judge the device in tests/test_gpu_tf_ops.py.  Every test prints its figures (-s).

Big cases are walked on their first rows only (tf_linear_bound.cpu_rows): the rows of a linear are independent.
"""
import pytest
import torch

import tf_linear_bound as LB

DTYPES = ["f16", "bf16", "f32", "f32m"]
KNAME = {LB.GENERIC: "generic", LB.ROWWAVE: "rowwave", LB.ROWWAVE_VEC: "rowwave_vec", LB.MFMA: "mfma", LB.F32M: "f32m"}


def _unique(cases):
    seen, out = set(), []
    for c in cases:
        k = LB.case_id(c)
        if k not in seen:
            seen.add(k)
            out.append(c)
    return out


def _cut(c, dtype):
    """inputs, weights, reference and bound of the rows of case c the CPU walks"""
    n = LB.cpu_rows(c)
    sd = LB.state_dict(c["dims"])
    wk, bk = LB.weight_keys(c["name"])
    x, r = LB.linear_inputs(c["dims"], c["name"], c["rows"], dtype, c["x_f32"], c["res"])
    ref, bound = LB.case_reference(c, dtype)
    x = LB.fed(x, dtype, c["kernel"])[:n]
    return x, LB.kernel_weight(sd[wk], dtype, c["kernel"]), sd[bk], (None if r is None else r[:n]), ref[:n], bound[:n], n


def test_the_cases_cover_what_the_kernels_can_get_wrong():
    for dt in ("f16", "bf16"):
        cs = LB.linear_cases(dt)
        assert {c["kernel"] for c in cs} == {LB.GENERIC, LB.ROWWAVE, LB.ROWWAVE_VEC, LB.MFMA}
        mf = [c for c in cs if c["kernel"] == LB.MFMA]
        assert {(c["relu"], c["res"]) for c in mf} == {(False, False), (True, False), (False, True), (True, True)}
        assert {c["rows"] for c in mf} >= {1, 127, 128, 129, 250, 1100}
        assert any(c["rows"] > 32768 and c["kernel"] == LB.ROWWAVE for c in cs)
        assert any(c["rows"] > 2 * 16384 and c["kernel"] == LB.ROWWAVE_VEC for c in cs)
    assert {c["kernel"] for c in LB.linear_cases("f32m")} == {LB.F32M}
    assert {c["kernel"] for c in LB.linear_cases("f32")} == {LB.GENERIC, LB.ROWWAVE}
    # the LDS edge between the two row-wave kernels
    assert 9 * 1360 * 4 <= 48 * 1024 < 9 * 1368 * 4 and 16 * 768 * 4 == 48 * 1024
    for mut in LB.LINEAR_MUTATIONS:
        assert all(any(LB.mutation_applies(mut, c) for c in LB.linear_cases(dt)) for dt in ("f16", "bf16", "f32")), mut


WORST = {}


@pytest.mark.parametrize("dtype", DTYPES)
def test_honest_linear_emulation_is_within_the_bound(dtype):
    worst = {}
    for c in _unique(LB.linear_cases(dtype)):
        x, W, b, r, ref, bound, n = _cut(c, dtype)
        out = LB.out_key(c, dtype)
        for order in LB.ORDERS:
            q, where = LB.ratio(LB.emulate_linear(x, W, b, r, c["relu"], out, order), ref, bound)
            assert q <= 1.0, (LB.case_id(c), order, q, where)
            k = (KNAME[c["kernel"]], out)
            if q > worst.get(k, (0.0,))[0]:
                worst[k] = (q, LB.case_id(c), order)
    for k, (q, cid, order) in sorted(worst.items()):
        print(f"{dtype} {k[0]:12s} stored as {k[1]:5s}: worst err / bound of the emulation {q:.3f} ({cid}, {order})")
    WORST[dtype] = worst


@pytest.mark.parametrize("dtype", ["f16", "bf16", "f32"])
@pytest.mark.parametrize("mutation", LB.LINEAR_MUTATIONS)
def test_broken_linear_emulations_fail_the_bound(dtype, mutation):
    """Judged on the device test's own cases; a float32 handle's "16-bit" defects (bias16, acc16) use bf16."""
    caught, tried = [], 0
    cases = _unique(LB.linear_cases(dtype) + (LB.linear_cases("f32m") if dtype == "f32" else []))
    for c in cases:
        if not LB.mutation_applies(mutation, c) or c["rows"] > 2000:
            continue                              # (the grid-stride cases add nothing here; the honest emulation walks them above)
        x, W, b, r, ref, bound, n = _cut(c, dtype)
        if mutation == "lastrow" and (n % 128 == 0 or n < 2):
            continue
        tried += 1
        d16 = dtype if dtype in ("f16", "bf16") else "bf16"
        q, where = LB.ratio(LB.emulate_linear(x, W, b, r, c["relu"], LB.out_key(c, dtype), "seq", mutation, d16), ref, bound)
        if q > 1.0:
            caught.append((LB.case_id(c), q))
    assert tried
    best = max(caught, key=lambda t: t[1]) if caught else None
    print(f"{mutation:10s} {dtype}: over the bound on {len(caught)} of {tried} cases" + (f", worst err / bound {best[1]:.3g} at {best[0]}" if best else ""))
    assert caught, f"no case shows the defect {mutation}"


LN_CASES = [(f, r, d) for d in LB.LN_DIMS for r in LB.LN_ROWS for f in LB.LN_FAMILIES]


@pytest.mark.parametrize("dtype", ["f16", "bf16", "f32"])
def test_honest_layernorm_emulation_is_within_the_bound(dtype):
    worst = {}
    for f, r, d in LN_CASES:
        x, w, b = LB.ln_inputs(f, r, d, dtype)
        ref, bound = LB.ln_reference(x, w, b, dtype)
        for order in LB.ORDERS:
            q, where = LB.ratio(LB.emulate_ln(x, w, b, dtype, order), ref, bound)
            assert q <= 1.0, (f, r, d, order, q, where)
            if q > worst.get(f, (0.0,))[0]:
                worst[f] = (q, d, r, order)
    for f, (q, d, r, order) in worst.items():
        print(f"{dtype} layernorm {f:9s}: worst err / bound of the emulation {q:.3f} (d = {d}, rows = {r}, {order})")


# where each LayerNorm defect has to show (the issue's wording): (families, dims, dtypes)
LN_MUST = {"unbiased": (LB.LN_FAMILIES, (8, 72), ("f16", "bf16", "f32")),
           "noeps": (("lowvar",), LB.LN_DIMS, ("f16", "bf16", "f32")),
           "onepass": (("offset",), LB.LN_DIMS, ("f32",)),
           "swap": (LB.LN_FAMILIES, LB.LN_DIMS, ("f16", "bf16", "f32")),
           "padmean": (LB.LN_FAMILIES, LB.LN_DIMS, ("f16", "bf16", "f32"))}


@pytest.mark.parametrize("mutation", LB.LN_MUTATIONS)
def test_broken_layernorm_emulations_fail_the_bound(mutation):
    fams, dims, dtypes = LN_MUST[mutation]
    for dtype in dtypes:
        caught = []
        for f, r, d in LN_CASES:
            if f not in fams or d not in dims:
                continue
            x, w, b = LB.ln_inputs(f, r, d, dtype)
            ref, bound = LB.ln_reference(x, w, b, dtype)
            q, _ = LB.ratio(LB.emulate_ln(x, w, b, dtype, "seq", mutation), ref, bound)
            if q > 1.0:
                caught.append(((f, r, d), q))
        best = max(caught, key=lambda t: t[1]) if caught else None
        print(f"{mutation:9s} {dtype}: over the bound on {len(caught)} cases" + (f", worst err / bound {best[1]:.3g} at (family, rows, d) = {best[0]}" if best else ""))
        assert caught, f"{dtype}: no case shows the defect {mutation}"
        if mutation == "unbiased":
            assert {c[0][2] for c in caught} == {8, 72}, "the unbiased variance must fail at d = 8 and at d = 72"


def test_a_non_finite_output_is_infinitely_wrong():
    x, w, b = LB.ln_inputs("normal", 5, 72, "f16")
    ref, bound = LB.ln_reference(x, w, b, "f16")
    got = LB.emulate_ln(x, w, b, "f16").clone()
    got[2, 7] = float("nan")
    q, where = LB.ratio(got, ref, bound)
    assert q == float("inf") and where == (2, 7)
