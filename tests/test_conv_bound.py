"""The element-wise conv checker (oracle/conv_bound.py) must bite: it passes the emulating oracle's own tensors and fails
copies of them broken the way kernels break, one defect at a time.  CPU only; the same checker judges the device in
tests/test_gpu_conv_elementwise.py.

Each broken copy is also put to the criterion the stage tests of tests/test_gpu_parity.py use, relL2 <= 2e-3 (f16) /
1e-2 (bf16) on the whole tensor at B = 64 (the two images replicated 32 times, ONE copy broken: the error norm stays,
the reference norm grows by sqrt(32)) -- generously, as if those tests could read the broken conv's output directly.
What that criterion does with each defect (224 x 224, seed 11; relL2 range over the convs broken; every test prints
its own figures with -s):

  defect                                          checker   whole-stage norm at B = 64 (tolerance f16 2e-3, bf16 1e-2)
  one product dropped on a border column, layer 1 fails     ACCEPTS all  (7e-5 .. 5e-4)
  one element off by 8 ulp (L1) / 2 x bound (L3+) fails     ACCEPTS all  (2e-6 .. 9e-5)
  bias of one channel off by 1 % of its RMS, L1   fails     ACCEPTS all  (7e-5 .. 9e-4)
  store rounded toward zero                       fails     ACCEPTS all  (f16 5e-4, bf16 4e-3: one u, under 4 u / 2.6 u)
  one tap dropped on a border column              fails     f16 catches (2.5e-3 .. 1.7e-2); bf16 ACCEPTS 12 of 16 convs
  one row taken from the row above                fails     f16 catches (4e-3 .. 1.3e-2); bf16 ACCEPTS 13 of 19
  ReLU skipped on 256 pixels                      fails     catches, except bf16 layer1.{0,1}.conv2 (5e-3)
  residual from the neighbouring image            fails     catches (3e-2)
  two images swapped                              fails     catches (0.2 .. 0.4)
"""
import functools

import pytest
import torch
import torch.nn.functional as F

from oracle import conv_bound as CB
from oracle import posenet_ref as O

TDT = {"f16": torch.float16, "bf16": torch.bfloat16}
OLD_TOL = {"f16": 2e-3, "bf16": 1e-2}
REPLICAS = 32           # B = 64 from the two distinct images


@functools.lru_cache(maxsize=None)
def _sd():
    from flope_amd.weights import synthetic_state_dict
    return synthetic_state_dict(0)


@functools.lru_cache(maxsize=4)
def _case(dtype, H, W):
    """The emulating oracle in the device's place: every conv's input / residual / output taps and its reference."""
    dt = TDT[dtype]
    torch.manual_seed(11)
    x = torch.rand(2, 3, H, W)
    taps = O.forward_stages_emulated(_sd(), x, dt)
    specs = CB.trunk_specs(_sd(), dt)
    rows = []
    for name, xin, rin, xds, out in CB.trunk_io(specs):
        spec = specs[name]
        xt, rt = taps[xin], (taps[rin] if rin else None)
        ref, bound = CB.reference(spec, xt, dt, rt)
        pre = CB.preactivation(spec, xt, rt)
        emu_rel = CB.rel_l2(CB.finish(spec, pre, dt), ref)
        rows.append(dict(name=name, spec=spec, x=xt, r=rt, got=taps[out], ref=ref, bound=bound, pre=pre, emu_rel=emu_rel))
    stem = specs["stem"]
    xin = CB.store(x, dt)
    ref, bound = CB.reference(stem, xin, dt)
    front = dict(stem=(taps["stem"], ref, bound, CB.rel_l2(CB.emulate(stem, xin, dt), ref)),
                 pool=(taps["pool"], CB.maxpool(ref), CB.maxpool(bound), CB.rel_l2(CB.maxpool(CB.emulate(stem, xin, dt)), CB.maxpool(ref))))
    return rows, front, dt


def _judge(row, got, dt):
    rep = CB.check(row["name"], got, row["ref"], row["bound"])
    return rep, CB.verdict(rep, row["emu_rel"], dt)


def _old_criterion(row, got):
    """relL2 of the whole tensor at B = 64 against the emulating oracle's tensor, one replica broken."""
    return float((got - row["got"]).double().norm() / (REPLICAS ** 0.5 * row["got"].double().norm()))


def _layer(row):
    return int(row["name"][5])


@pytest.mark.parametrize("H,W", [(224, 224), (65, 71)])
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_unbroken_emulation_passes_every_conv(dtype, H, W):
    rows, front, dt = _case(dtype, H, W)
    assert len([r for r in rows if not r["name"].endswith(".ds")]) == 16
    worst = 0.0
    for row in rows:
        rep, fails = _judge(row, row["got"], dt)
        print(f"{dtype} {H}x{W} {row['name']:16s} max err/bound {rep.max_ratio:.3f}  relL2 {rep.rel_l2 / CB.UNIT_ROUNDOFF[dt]:.3f} u  "
              f"emu {row['emu_rel'] / CB.UNIT_ROUNDOFF[dt]:.3f} u  median bound / rms {float(row['bound'].median() / row['ref'].pow(2).mean().sqrt()):.2e}")
        assert not fails, fails
        worst = max(worst, rep.max_ratio)
    for name, (got, ref, bound, emu_rel) in front.items():
        rep = CB.check(name, got, ref, bound)
        assert not CB.verdict(rep, emu_rel, dt), CB.verdict(rep, emu_rel, dt)
        worst = max(worst, rep.max_ratio)
    assert worst <= 1.0


def test_store_toward_zero_is_exact_truncation():
    for dt in TDT.values():
        t = torch.randn(4096) * 3
        z = CB.store_toward_zero(t, dt)
        assert (z.abs() <= t.abs()).all() and (z.to(dt).float() == z).all()
        up = (z.to(dt).view(torch.int16) + 1).view(dt).float()          # the next storage value away from zero
        assert ((up.abs() > t.abs()) | (z == t)).all()


def _report(kind, dtype, row, rep, fails, old):
    print(f"{kind:14s} {dtype:4s} {row['name']:16s} checker: {len(fails)} failed assertion(s), {rep.count} elements, worst {rep.max_ratio:.3g} at {rep.worst}; "
          f"whole-stage relL2 at B=64 {old:.2e} ({'ACCEPTS' if old <= OLD_TOL[dtype] else 'catches'})")


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_dropped_tap_on_a_border_column(dtype):
    """A wrong edge mask: tap (ky, kx) = (1, 0), all input channels, missing at the last column of image 1."""
    rows, _, dt = _case(dtype, 224, 224)
    for row in rows:
        spec = row["spec"]
        if spec.w.shape[2] != 3:
            continue
        wt = torch.zeros_like(spec.w)
        wt[:, :, 1, 0] = spec.w[:, :, 1, 0]
        pre = row["pre"].clone()
        pre[1, :, :, -1] -= F.conv2d(row["x"][1:2], wt, None, stride=spec.stride, padding=1)[0, :, :, -1]
        got = CB.finish(spec, pre, dt)
        rep, fails = _judge(row, got, dt)
        old = _old_criterion(row, got)
        _report("border tap", dtype, row, rep, fails, old)
        assert any(f.startswith("assertion 1") for f in fails), row["name"]
        assert rep.worst[0] == 1 and rep.worst[3] == got.shape[3] - 1, rep.describe()


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_dropped_single_product_in_layer1(dtype):
    """One (ky, kx, ci) product of 576 missing at the first column of image 0."""
    rows, _, dt = _case(dtype, 224, 224)
    n = 0
    for row in rows:
        if _layer(row) != 1:
            continue
        spec = row["spec"]
        wt = torch.zeros_like(spec.w)
        wt[:, 5, 2, 1] = spec.w[:, 5, 2, 1]
        pre = row["pre"].clone()
        pre[0, :, :, 0] -= F.conv2d(row["x"][0:1], wt, None, stride=spec.stride, padding=1)[0, :, :, 0]
        got = CB.finish(spec, pre, dt)
        rep, fails = _judge(row, got, dt)
        old = _old_criterion(row, got)
        _report("one product", dtype, row, rep, fails, old)
        assert any(f.startswith("assertion 1") for f in fails), row["name"]
        assert rep.worst[0] == 0 and rep.worst[3] == 0, rep.describe()
        assert old <= OLD_TOL[dtype], "the whole-stage norm was expected to accept this defect"
        n += 1
    assert n == 4


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_row_from_the_row_above_and_swapped_images(dtype):
    rows, _, dt = _case(dtype, 224, 224)
    for row in rows:
        got = row["got"].clone()
        y = got.shape[2] // 2
        got[1, :, y, :] = got[1, :, y - 1, :]
        rep, fails = _judge(row, got, dt)
        _report("row above", dtype, row, rep, fails, _old_criterion(row, got))
        assert any(f.startswith("assertion 1") for f in fails), row["name"]
        assert rep.worst[0] == 1 and rep.worst[2] == y, rep.describe()
        got = row["got"][[1, 0]]
        rep, fails = _judge(row, got, dt)
        _report("images swapped", dtype, row, rep, fails, _old_criterion(row, got) * REPLICAS ** 0.5)   # every replica pair swapped
        assert any(f.startswith("assertion 1") for f in fails), row["name"]


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_residual_from_the_neighbouring_image(dtype):
    rows, _, dt = _case(dtype, 224, 224)
    n = 0
    for row in rows:
        if row["r"] is None:
            continue
        r = row["r"].clone()
        r[0] = row["r"][1]
        got = CB.finish(row["spec"], CB.preactivation(row["spec"], row["x"], r), dt)
        rep, fails = _judge(row, got, dt)
        _report("residual", dtype, row, rep, fails, _old_criterion(row, got))
        assert any(f.startswith("assertion 1") for f in fails), row["name"]
        assert rep.worst[0] == 0, rep.describe()
        n += 1
    assert n == 8


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_relu_skipped_on_one_tile(dtype):
    """The first 256 pixels of image 0 (the whole image where the map is smaller) stored without ReLU."""
    rows, _, dt = _case(dtype, 224, 224)
    for row in rows:
        if not row["spec"].relu:
            continue
        got = row["got"].clone()
        B, C, h, w = got.shape
        npx = min(256, h * w)
        got[0].view(C, h * w)[:, :npx] = CB.store(row["pre"][0].reshape(C, h * w)[:, :npx], dt)
        rep, fails = _judge(row, got, dt)
        _report("no ReLU", dtype, row, rep, fails, _old_criterion(row, got))
        assert any(f.startswith("assertion 1") for f in fails), row["name"]
        assert rep.worst[0] == 0 and rep.worst[2] * w + rep.worst[3] < npx, rep.describe()
        assert rep.got < 0.0


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_bias_of_one_channel_off_by_one_percent(dtype):
    rows, _, dt = _case(dtype, 224, 224)
    n = 0
    for row in rows:
        if _layer(row) != 1:
            continue
        c = int(row["ref"].pow(2).mean(dim=(0, 2, 3)).argsort()[32])     # the channel of median RMS (some are dead behind their ReLU)
        pre = row["pre"].clone()
        pre[:, c] += 0.01 * float(row["ref"][:, c].pow(2).mean().sqrt())
        got = CB.finish(row["spec"], pre, dt)
        rep, fails = _judge(row, got, dt)
        old = _old_criterion(row, got) * REPLICAS ** 0.5        # a wrong bias is wrong in every replica
        _report("bias 1 %", dtype, row, rep, fails, old)
        assert fails and rep.worst[1] == c, (row["name"], fails, rep.describe())
        assert old <= OLD_TOL[dtype], "the whole-stage norm was expected to accept this defect"
        n += 1
    assert n == 4


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_single_element_off(dtype):
    """Layer 1: one element off by 8 ulp of the storage type.  Layers 3 and 4 (accumulation term 10 to 100 times the rounding
    term): off by twice its own bound."""
    rows, _, dt = _case(dtype, 224, 224)
    n = 0
    for row in rows:
        li = _layer(row)
        if li == 2:
            continue
        got = row["got"].clone()
        idx = (1,) + tuple(int(v) for v in torch.unravel_index(row["ref"][1].argmax(), row["ref"][1].shape))
        if li == 1:
            v = got[idx].to(dt)
            ulp = abs(float((v.view(torch.int16) + 1).view(dt)) - float(v))
            got[idx] += 8 * ulp
        else:
            got[idx] = float(row["ref"][idx] + 2 * row["bound"][idx])
        rep, fails = _judge(row, got, dt)
        old = _old_criterion(row, got)
        _report("one element", dtype, row, rep, fails, old)
        assert any(f.startswith("assertion 1") for f in fails), row["name"]
        assert rep.count == 1 and rep.worst == idx, rep.describe()
        assert old <= OLD_TOL[dtype], "the whole-stage norm was expected to accept this defect"
        n += 1
    assert n >= 12


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_store_rounded_toward_zero(dtype):
    """Fails assertion 2 on every conv; in layer 1, where the accumulation term is small, assertion 1 as well."""
    rows, _, dt = _case(dtype, 224, 224)
    for row in rows:
        got = CB.finish(row["spec"], row["pre"], dt, rounding="toward_zero")
        rep, fails = _judge(row, got, dt)
        _report("toward zero", dtype, row, rep, fails, _old_criterion(row, got) * REPLICAS ** 0.5)
        assert any(f.startswith("assertion 2") for f in fails), (row["name"], rep.rel_l2, row["emu_rel"])
        if _layer(row) == 1:
            assert any(f.startswith("assertion 1") for f in fails), row["name"]


def test_fp32_throughout_uses_the_order_independent_statistic():
    """Strict fp32 mode stores in the accumulator's type: assertion 2 is relL2 <= || u |ref| + sqrt(K + 2) 2^-23 mag || / || ref ||
    (oracle/conv_bound.py).  The plain evaluation passes it; one product of 4608 missing at every pixel of a layer-4 conv
    (2e-2 of the output RMS against a statistic of 3e-4) fails it."""
    dt = torch.float32
    torch.manual_seed(11)
    x = torch.rand(2, 3, 65, 71)
    taps = O.forward_stages_emulated(_sd(), x, dt)
    specs = CB.trunk_specs(_sd(), dt)
    for name, xin, rin, _, out in CB.trunk_io(specs):
        spec = specs[name]
        xt, rt = taps[xin], (taps[rin] if rin else None)
        ref, bound = CB.reference(spec, xt, dt, rt)
        stat_rel = float(CB.statistical_bound(ref, bound, spec.K, dt).norm() / ref.norm())
        rep = CB.check(name, taps[out], ref, bound)
        print(f"f32 {name:16s} max err/bound {rep.max_ratio:.4f}  relL2 {rep.rel_l2:.3g}  statistic {stat_rel:.3g}")
        assert not CB.verdict(rep, 0.0, dt, stat_rel=stat_rel)
        if name == "layer4.1.conv1":
            wt = torch.zeros_like(spec.w)
            wt[:, 100, 1, 1] = spec.w[:, 100, 1, 1]
            got = CB.finish(spec, CB.preactivation(spec, xt, rt) - F.conv2d(xt, wt, None, stride=spec.stride, padding=1), dt)
            rep = CB.check(name, got, ref, bound)
            fails = CB.verdict(rep, 0.0, dt, stat_rel=stat_rel)
            print(f"    one product of {spec.K} missing everywhere: relL2 {rep.rel_l2:.3g}, {len(fails)} failed assertion(s)")
            assert any(f.startswith("assertion 2") for f in fails), fails
