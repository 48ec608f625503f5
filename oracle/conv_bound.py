"""Oracle: one convolution of the PoseResNet trunk on its own, in fp64, with a derived element-wise error bound.

TEST INFRASTRUCTURE ONLY -- see oracle/__init__.py.

The whole-stage checks of tests/test_gpu_parity.py compare norms against an oracle that runs the network from its
input, so their tolerance has to absorb what earlier layers did and a handful of wrong elements disappears in the
norm.  Here every convolution is judged alone: from the tensor the device itself fed it (16-bit values widened, hence
exact), the folded and 16-bit-rounded weights (posenet_ref.fold_bn, then one rounding, as the engine packs them), the
fp32 bias, an optional residual and the ReLU flag,

    acc   = conv64(x, w) + b + r                      float64
    ref   = relu(acc) or acc
    mag   = conv64(|x|, |w|) + |b| + |r|              float64, same geometry
    bound = u |ref|  +  (K + 2) 2^-23 mag  +  tiny

  u |ref|            the single round-to-nearest of the epilogue's store; u = 2^-11 (f16), 2^-8 (bf16), 2^-24 (fp32 mode).
  (K + 2) 2^-23 mag  fp32 accumulation of K products plus bias and residual IN ANY ORDER.  The textbook figure for a sum
                     of n terms is (n - 1) 2^-24 sum|t_i| to first order whatever the order of the additions; the factor 2
                     makes it independent of whether the matrix unit's accumulator rounds to nearest or truncates (one ulp
                     instead of half an ulp per addition).  Products of two 16-bit values are exact in fp32 (11 + 11 or
                     8 + 8 significand bits); in fp32 mode a fused multiply-add rounds once per term, which the same count
                     covers.  K is the number of taps really summed: kh kw Cin, + Cin of the shortcut when it is folded in.
  tiny               one smallest subnormal of the storage type: a ReLU'd value next to zero may land on either side.

A 1x1 shortcut folded into conv2 (engine option dsfuse) enters `acc` as the fp64 1x1 conv of the block input plus its
bias, NOT rounded to the storage type (the device keeps it in the accumulator), and `mag` gets its magnitudes.  The
rounding of relu(acc + d) against relu(acc) + ... needs no extra term: |relu(a) - relu(b)| <= |a - b|.

`emulate` is the plain fp32 evaluation (F.conv2d in float32, as posenet_ref.forward_stages_emulated does) of the same
conv on the same input, rounded once to the storage type: the yardstick of the second assertion
relL2(got, ref) <= 1.25 relL2(emu, ref).  For 16-bit storage that statistic is the storage rounding itself
(u / sqrt(3) ~ 0.4 u on average); accumulation order only decides near-ties.

Where that derivation does NOT hold: an operation that is fp32 throughout (the strict fp32 mode's convs, the average
pool, fc.0, fc_rot) stores in the accumulator's own type, so relL2(x, ref) IS the accumulation error and depends on the
order of the additions.  Measured on an MI355X against this CPU's F.conv2d / F.linear: the strict mode's plain
sequential fused-multiply-add loop 1.0 (K = 64) .. 4.5 (K = 4608) times the CPU's blocked sum, fc.0 on the fp32 matrix
unit 1.2 .. 1.5 times, fc_rot 0.3 .. 0.55 times -- all within 0.14 of assertion 1's bound (convs and fc within 0.04).  Two correct orders differ
there by more than any fixed margin near 1, so for these operations assertion 2 is the order-independent statistic

    relL2(got, ref) <= || u |ref| + sqrt(K + 2) 2^-23 mag ||_2 / || ref ||_2                  (`statistical_bound`)

i.e. the same terms as `bound` with the accumulation term growing as the square root of the number of additions: the
rounding errors of a sum are bounded by one ulp of a partial sum each (|partial sum| <= mag) and, rounding to nearest,
have no common sign, so their sum over n additions has a root mean square of at most sqrt(n) ulp(mag) (the
probabilistic error model of Higham & Mary, SIAM J. Sci. Comput. 41 (2019)); the factor 2 of assertion 1 is kept.
It still catches an error that is small everywhere: one tap of 4608 missing is 1.5e-2 of the output RMS, the statistic
allows 3e-4 there (layer4.1.conv1; 2e-5 .. 2e-4 on the other convs).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import torch
import torch.nn.functional as F

from . import posenet_ref as O

UNIT_ROUNDOFF = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8, torch.float32: 2.0 ** -24}
TINY = {torch.float16: 2.0 ** -24, torch.bfloat16: 2.0 ** -133, torch.float32: 2.0 ** -149}
REL_L2_MARGIN = 1.25
F16_MAX_REF = 6.0e4        # the synthetic weights keep f16 far from saturation: asserted, never masked


def store(t: torch.Tensor, act_dtype) -> torch.Tensor:
    """One round-to-nearest-even to the storage type, widened again (float32)."""
    return t.float().to(act_dtype).float()


@dataclass
class ConvSpec:
    name: str                       # "stem", "layer2.0.conv1", "layer2.0.ds", ...
    w: torch.Tensor                 # [Cout,Cin,k,k] float32, already rounded to the storage type
    b: torch.Tensor                 # [Cout] float32
    stride: int
    padding: int
    relu: bool
    ds_w: Optional[torch.Tensor] = None   # folded 1x1 shortcut (conv2 of layer{2,3,4}.0 only): [Cout,Cin0,1,1]
    ds_b: Optional[torch.Tensor] = None
    ds_stride: int = 2

    @property
    def K(self) -> int:
        k = self.w.shape[1] * self.w.shape[2] * self.w.shape[3]
        return k + (self.ds_w.shape[1] if self.ds_w is not None else 0)


def trunk_specs(sd: dict, act_dtype, fold_shortcut=()) -> dict:
    """ConvSpec of the stem, the 16 block convs and the 3 shortcut convs.  `fold_shortcut`: layer indices (2..4) whose
    shortcut is computed inside conv2; their "layerN.0.conv2" spec carries ds_w / ds_b and "layerN.0.ds" is omitted."""
    sd = {k: v.float() for k, v in sd.items() if v.is_floating_point()}
    specs = {}
    w, b = O.fold_bn(sd["base.conv1.weight"], sd, "base.bn1")
    specs["stem"] = ConvSpec("stem", store(w, act_dtype), b, 2, 3, True)
    for li, _cin, _cout, stride in O.LAYER_CFG:
        for bi in range(2):
            p = f"base.layer{li}.{bi}"
            s = stride if bi == 0 else 1
            w, b = O.fold_bn(sd[p + ".conv1.weight"], sd, p + ".bn1")
            specs[f"layer{li}.{bi}.conv1"] = ConvSpec(f"layer{li}.{bi}.conv1", store(w, act_dtype), b, s, 1, True)
            w, b = O.fold_bn(sd[p + ".conv2.weight"], sd, p + ".bn2")
            c2 = ConvSpec(f"layer{li}.{bi}.conv2", store(w, act_dtype), b, 1, 1, True)
            if (p + ".downsample.0.weight") in sd:
                wd, bd = O.fold_bn(sd[p + ".downsample.0.weight"], sd, p + ".downsample.1")
                if li in fold_shortcut:
                    c2.ds_w, c2.ds_b, c2.ds_stride = store(wd, act_dtype), bd, s
                else:
                    specs[f"layer{li}.{bi}.ds"] = ConvSpec(f"layer{li}.{bi}.ds", store(wd, act_dtype), bd, s, 0, False)
            specs[c2.name] = c2
    return specs


def _conv64(x, w, stride, padding):
    return F.conv2d(x.double(), w.double(), None, stride=stride, padding=padding)


def reference(spec: ConvSpec, x: torch.Tensor, act_dtype, r: Optional[torch.Tensor] = None,
              x_ds: Optional[torch.Tensor] = None):
    """-> (ref, bound), float64 [B,Cout,h,w].  x: the conv's input as stored; r: residual tensor as stored (or None);
    x_ds: the block input, when spec carries a folded shortcut."""
    acc = _conv64(x, spec.w, spec.stride, spec.padding) + spec.b.double().view(1, -1, 1, 1)
    mag = _conv64(x.abs(), spec.w.abs(), spec.stride, spec.padding) + spec.b.double().abs().view(1, -1, 1, 1)
    if spec.ds_w is not None:
        assert x_ds is not None and r is None, "a folded shortcut takes the block input, not a residual tensor"
        acc = acc + _conv64(x_ds, spec.ds_w, spec.ds_stride, 0) + spec.ds_b.double().view(1, -1, 1, 1)
        mag = mag + _conv64(x_ds.abs(), spec.ds_w.abs(), spec.ds_stride, 0) + spec.ds_b.double().abs().view(1, -1, 1, 1)
    if r is not None:
        acc = acc + r.double()
        mag = mag + r.double().abs()
    ref = F.relu(acc) if spec.relu else acc
    bound = UNIT_ROUNDOFF[act_dtype] * ref.abs() + (spec.K + 2) * 2.0 ** -23 * mag + TINY[act_dtype]
    return ref, bound


def statistical_bound(ref, bound, K: int, act_dtype):
    """Assertion 2 of an operation that is fp32 throughout (see the module docstring): u |ref| + sqrt(K + 2) 2^-23 mag + tiny,
    recovered from `bound` = u |ref| + (K + 2) 2^-23 mag + tiny."""
    round_term = UNIT_ROUNDOFF[act_dtype] * ref.abs()
    return round_term + (bound - round_term - TINY[act_dtype]).clamp_min(0.0) / (K + 2) ** 0.5 + TINY[act_dtype]


def preactivation(spec: ConvSpec, x, r=None, x_ds=None):
    """fp32 accumulator of the plain CPU evaluation: conv + bias (+ folded shortcut) (+ residual), before ReLU and store."""
    y = F.conv2d(x.float(), spec.w, spec.b, stride=spec.stride, padding=spec.padding)
    if spec.ds_w is not None:
        y = y + F.conv2d(x_ds.float(), spec.ds_w, spec.ds_b, stride=spec.ds_stride, padding=0)
    if r is not None:
        y = y + r.float()
    return y


def finish(spec: ConvSpec, y, act_dtype, rounding="nearest"):
    """Epilogue: ReLU where the conv has one, then ONE store.  rounding="toward_zero" is the broken store of
    tests/test_conv_bound.py (never the yardstick)."""
    if spec.relu:
        y = F.relu(y)
    return store(y, act_dtype) if rounding == "nearest" else store_toward_zero(y, act_dtype)


def emulate(spec: ConvSpec, x, act_dtype, r=None, x_ds=None):
    """Plain CPU fp32 evaluation of the same conv, stored once -> float32 (the yardstick of assertion 2)."""
    return finish(spec, preactivation(spec, x, r, x_ds), act_dtype)


def trunk_io(specs: dict):
    """[(spec name, input tap, residual tap | None, folded-shortcut input tap | None, output tap)] of the 16 block convs
    and of every shortcut conv that `specs` holds on its own, in launch order.  Tap names are PoseEngine.read_stage's."""
    rows, cur = [], "pool"
    for li in range(1, 5):
        for bi in range(2):
            blk = f"layer{li}.{bi}"
            rows.append((blk + ".conv1", cur, None, None, blk + ".mid"))
            if blk + ".ds" in specs:
                rows.append((blk + ".ds", cur, None, None, blk + ".ds"))
                rows.append((blk + ".conv2", blk + ".mid", blk + ".ds", None, blk))
            elif specs[blk + ".conv2"].ds_w is not None:
                rows.append((blk + ".conv2", blk + ".mid", None, cur, blk))
            else:
                rows.append((blk + ".conv2", blk + ".mid", cur, None, blk))
            cur = blk
    return rows


def store_toward_zero(t: torch.Tensor, act_dtype) -> torch.Tensor:
    """Truncating store (what a conversion by bit-shift does)."""
    t = t.float()
    n = store(t, act_dtype)
    if act_dtype == torch.float32:
        return n
    over = n.abs() > t.abs()                 # rounded away from zero: step one storage ulp back
    bits = n.to(act_dtype).view(torch.int16)
    back = (bits - 1).view(act_dtype).float()     # sign-magnitude encoding: magnitude - 1 ulp for either sign
    return torch.where(over, back, n)


def linear_reference(x, w, b, relu: bool):
    """Head: y = x W^T + b in fp32 throughout -> (ref, bound) with u = 2^-24, K = in_features."""
    acc = x.double() @ w.double().t() + b.double()
    mag = x.double().abs() @ w.double().abs().t() + b.double().abs()
    ref = F.relu(acc) if relu else acc
    return ref, 2.0 ** -24 * ref.abs() + (w.shape[1] + 2) * 2.0 ** -23 * mag + TINY[torch.float32]


def avgpool_reference(x):
    """Global average pool of the stored last stage, fp32 sum then one scaling: K = pixels."""
    n = x.shape[2] * x.shape[3]
    ref = x.double().mean(dim=(2, 3))
    mag = x.double().abs().mean(dim=(2, 3))
    return ref, 2.0 ** -24 * ref.abs() + (n + 2) * 2.0 ** -23 * mag + TINY[torch.float32]


def maxpool(t):
    """3x3 stride-2 pad-1 max-pool.  |max a - max b| <= max |a - b|, so maxpool(bound) bounds maxpool(got) - maxpool(ref)."""
    return F.max_pool2d(t, 3, 2, 1)


def rel_l2(a, ref) -> float:
    ref = ref.double()
    return float((a.double() - ref).norm() / ref.norm().clamp_min(1e-300))


@dataclass
class Report:
    name: str
    count: int            # elements over the bound or not finite
    total: int
    max_ratio: float      # max err / bound
    worst: tuple          # (image, channel, y, x) of that maximum (or of the first non-finite element)
    got: float
    ref: float
    bound: float
    err2: float           # sum (got - ref)^2
    ref2: float           # sum ref^2
    ref_absmax: float

    @property
    def rel_l2(self) -> float:
        return (self.err2 / max(self.ref2, 1e-300)) ** 0.5

    @property
    def ok(self) -> bool:
        return self.count == 0

    def describe(self, kernel: str = "") -> str:
        return (f"{self.name}{' [' + kernel + ']' if kernel else ''}: {self.count} of {self.total} elements over the bound; worst err/bound "
                f"{self.max_ratio:.3g} at (image, channel, y, x) = {self.worst}: got {self.got!r} ref {self.ref!r} bound {self.bound:.3g}")


def check(name: str, got: torch.Tensor, ref: torch.Tensor, bound: torch.Tensor) -> Report:
    """Assertion 1 on every element: |got - ref| <= bound and got finite.  Tensors of one shape on one device."""
    assert got.shape == ref.shape == bound.shape, (name, tuple(got.shape), tuple(ref.shape), tuple(bound.shape))
    g = got.double()
    finite = torch.isfinite(g)
    err = torch.where(finite, (g - ref).abs(), torch.full_like(g, float("inf")))
    ratio = err / bound
    bad = ~(err <= bound)
    flat = int(ratio.argmax())
    idx = []
    for n in reversed(got.shape):
        idx.append(flat % n)
        flat //= n
    idx = tuple(reversed(idx))
    e2 = torch.where(finite, err, torch.zeros_like(err))
    return Report(name, int(bad.sum()), got.numel(), float(ratio.max()), idx, float(g[idx]), float(ref[idx]), float(bound[idx]),
                  float((e2 * e2).sum()), float((ref * ref).sum()), float(ref.abs().max()))


def verdict(rep: Report, emu_rel: float, act_dtype, kernel: str = "", stat_rel: Optional[float] = None):
    """-> list of failure messages (empty: both assertions hold).  16-bit storage: assertion 2 against the emulation;
    fp32 throughout: against stat_rel = || statistical_bound || / || ref || (required then)."""
    out = []
    if act_dtype == torch.float16 and not rep.ref_absmax < F16_MAX_REF:
        out.append(f"{rep.name}: |ref| reaches {rep.ref_absmax:.3g}, too close to the float16 range for this check")
    if not rep.ok:
        out.append("assertion 1: " + rep.describe(kernel))
    if act_dtype == torch.float32:
        if not rep.rel_l2 <= stat_rel:
            out.append(f"assertion 2 (fp32 throughout): {rep.name}{' [' + kernel + ']' if kernel else ''}: relL2(got, ref) = {rep.rel_l2:.4g} > "
                       f"|| u |ref| + sqrt(K + 2) 2^-23 mag || / || ref || = {stat_rel:.4g}")
    elif not rep.rel_l2 <= REL_L2_MARGIN * emu_rel:
        out.append(f"assertion 2: {rep.name}{' [' + kernel + ']' if kernel else ''}: relL2(got, ref) = {rep.rel_l2:.4g} > {REL_L2_MARGIN} x "
                   f"relL2(emu, ref) = {emu_rel:.4g}")
    return out
