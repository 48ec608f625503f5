"""Oracle: one op of the YOLO11-seg detector on its own, in fp64, with a derived element-wise error bound.

TEST INFRASTRUCTURE ONLY -- see oracle/__init__.py.  Plain torch in float64 / float32; reuses oracle/conv_bound.py's `store`,
`check`, `Report`, `rel_l2`, `UNIT_ROUNDOFF`, `TINY`, `REL_L2_MARGIN` and its two assertions:

    1.  |got - ref| <= bound at every element, got finite
    2.  16-bit storage:      relL2(got, ref) <= 1.25 relL2(emu, ref),  emu = the plain CPU float32 evaluation stored once
        float32 throughout:  relL2(got, ref) <= || stat || / || ref ||,  stat = bound with sqrt(count) for every count
                             (conv_bound.statistical_bound's form; float32 maps of the strict mode and the float32 prediction rows)

Inputs are always the tensors the device fed the op: 16-bit values widened (or float32), hence exact.  Weights are folded as the
builder folds them (yolo_engine.hip Builder::conv): s = g / sqrt(var + 1e-3) in double, w s and b - mu s in double, then float32,
then ONE rounding of the conv weights to the storage type; depthwise weights and every bias stay float32.

u = UNIT_ROUNDOFF of the storage type (2^-11 f16, 2^-8 bf16, 2^-24 float32); u32 = 2^-24.

conv / plain / deconv  (`conv_reference`)
    acc = conv64(x, w) + b                     mag = conv64(|x|, |w|) + |b|                K = k k Cin  (the REAL Cin: 3 for model.0)
    ref = silu(acc) or acc, then + res         (the residual is added AFTER the activation)
    bound = u |ref| + L (K + 2) 2^-23 mag + S(acc) + tiny
  u |ref|              the one storage rounding; absent for the float32 prediction rows (out_mode 1), whose accumulator is stored as it is.
  (K + 2) 2^-23 mag    float32 accumulation of K products, bias and residual in any order, rounding to nearest or truncating
                       (conv_bound.py).  The residual's magnitude is part of mag.  L = 1.1 where SiLU follows: an error d of the
                       accumulator becomes at most sup |silu'| d, and silu'(v) = s (1 + v (1 - s)), s = sigmoid(v), peaks at 1.0998.
  S(v)                 evaluation of SiLU itself, from the documented accuracy of what the kernels call.
                       16-bit kernels: v * rcp(1 + __expf(-v)).  __expf(x) = exp2(x log2 e): the product rounds once, an argument
                       error |x| log2(e) u32 changes exp2 by the relative |x| u32; v_exp_f32 is good to 1 ulp = 2 u32.  So e^-v has
                       relative error (|v| + 2) u32, 1 + e^-v at most that plus u32, v_rcp_f32 1 ulp = 2 u32, the product u32:
                           S(v) = (|v| + 6) u32 |silu(v)|, doubled for slack in the documented 1 ulp figures: (2 |v| + 12) u32 |silu(v)|.
                       It grows LINEARLY in |v| relative to silu(v) -- but for v -> -inf silu(v) ~ v e^v itself vanishes faster, so the
                       absolute term peaks near |v| ~ 2 and stays below 6 u32 for any v < 0; for v > 0 the error of e^-v is damped by
                       e^-v / (1 + e^-v) and the linear growth is only the bound's, not the kernel's.
                       yolo_f32.hip: __fdiv_rn(v, 1 + expf(-v)): expf 1 ulp, the sum u32, the division u32 (correctly rounded):
                           S(v) = 4 u32 |silu(v)|, taken as 6 u32 |silu(v)|: no growth with |v|.
                       Both: + 2^-119.  Where 1 / (1 + e^-v) falls below 2^-126 the fast reciprocal flushes it to zero; |v| < 128
                       there (e^-v overflows beyond), so the lost value is below 128 x 2^-126.
  tiny                 one smallest subnormal of the storage type.
  deconv               ConvTranspose2d(2, 2, 0): every output pixel has exactly one tap, the four (dy, dx) phases are 1x1 convs of
                       K = Cin scattered to (2y + dy, 2x + dx): the same bound with conv_transpose2d as conv64.

fused Bottleneck  (`bneck_reference`)
    The intermediate never leaves LDS; it is rounded to the storage type there.  ref = cv2(store(silu(cv1(x)))) + x.
    bound = cv2's own bound + conv64(d_mid, |w2|),   d_mid = bound1 + one storage ulp (2 u) of mid
    bound1 is cv1's bound above (it contains the storage rounding u |mid|): the device's unrounded intermediate is within
    bound1 - u |mid| of the reference's, and two values that close round to stored values at most that distance plus one ulp
    apart.  A device intermediate one rounding away from the reference's is therefore legitimate, and so is an intermediate that is
    not rounded at all (it is within u |mid| of the rounded one): that planted error is NOT in the list of tests/test_yolo_op_bound.py.
    conv64(d_mid, |w2|) is an error of cv2's ACCUMULATOR and is nevertheless added without the factor L = 1.1: the term is the one the
    project's issue for this check states, and a bound it states is not widened here.  What that costs: |silu'| exceeds 1 only for
    v > 1.28, by at most 10 %, so on such elements this one term is up to a tenth short of the first-order worst case -- a worst case in
    which the errors of all 9 Cin intermediate taps line up with the signs of w2.  Measured on the device the whole bound is used to 0.47.
    With bneck = 0 the two convs are judged singly, cv2 from the device's own stored intermediate.

depthwise  (`dw_reference`)   9 float32 fused multiply-adds on the bias, SiLU, + add: the conv bound with K = 9, float32 weights.
    Output channel c reads input channel (c / blk) blk_stride + blk_off + c % blk where blk != 0 (the v rows of a qkv map): part of the
    reference.

max-pool x3, nearest upsample  (`pool_reference`, `up_reference`)   exact: no arithmetic, only comparisons and copies.  The three
    cascaded 5x5 stride-1 pools with a -inf border land in channel slices [i C, (i + 1) C); torch.equal decides.

attention  (`attn_reference`)   per head q (32) k (32) v (64) interleaved, scale = 32^-0.5; tests/tf_attn_bound.py's derivation with
    the natural exponential.  P_ij = softmax_j(scale q_i . k_j), O = P v, A = P |v|, a_i = scale max_j sum_c |q_ic k_jc|, n = ceil(N / 32):
      argument of a probability: 32 exact products summed in float32 and the scale (before or after the sum): (32 + 4) u32 a_i;
      x - m and the telescoping arguments of the rescale factors: 4 u32 a_i; __expf's own product with log2 e on |x - m| <= 2 a_i, for
      the probability and the rescale factors: 4 u32 a_i; exp, rescale and reciprocal roundings (4 n + 8) u32:
          e_i = (32 + 12) u32 a_i + (4 n + 8) u32
      float32 sums of N terms, in numerator and denominator: (N + n + 10) u32 each:       E_i = 2 e_i + 2 (N + n + 10) u32
      the MFMA kernel of the 16-bit modes rounds P to the storage type for the second MFMA while its sum l adds the UNROUNDED values:
          u_P A with u_P = u (0 in the generic kernel and in float32 mode); f16: subnormal probabilities, N 2^-25 max |v|
      the output rounding u (|O| + error so far); f16: + 2^-25.
          bound = (u_P + E_i) A + u (|O| + (u_P + E_i) A) + [f16] (N 2^-25 max |v| + 2^-25) + tiny
    Normalising by the sum of the ROUNDED probabilities instead changes l by at most the relative u, O by u |O| <= u A: the u_P A term
    already allows that much, so this bound cannot tell the two apart and that planted error is not in the list either.
    Assertion 2 and the MFMA kernel: its yardstick is the plain float32 softmax stored ONCE, which has no rounded P.  The extra error
    is u sqrt(sum_j (P_ij v_jc)^2 / 3) against the storage rounding's u |O_ic| / sqrt(3): negligible where attention is diffuse and the values
    of neighbouring keys resemble each other, as in the network (emulated kernel on the synthetic checkpoint's qkv maps: 1.00 .. 1.08
    times the yardstick on the frames of the GPU walk).  On white noise the values cancel in O but not in that sum, both errors are of
    one size and a CORRECT kernel lands at sqrt(2) times the yardstick.  The tests therefore feed attention the network's own qkv maps.

f16 saturation: |ref| < F16_MAX_REF is asserted by `verdict`, never masked.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import torch
import torch.nn.functional as F

from .conv_bound import (F16_MAX_REF, REL_L2_MARGIN, TINY, UNIT_ROUNDOFF, Report, check, rel_l2, store)   # noqa: F401 (re-exported)

BN_EPS = 1e-3
U32 = 2.0 ** -24
SILU_LIPSCHITZ = 1.1
FLUSH = 2.0 ** -119
TDT = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}
GRAPH_REL_L2 = {"f16": 5e-3, "bf16": 8e-2, "f32": 2e-5}       # the whole-map thresholds of tests/test_gpu_yolo.py


@dataclass
class Judged:
    ref: torch.Tensor               # float64
    bound: torch.Tensor             # float64, assertion 1
    emu: torch.Tensor               # float32: the plain CPU float32 evaluation, stored once
    stat: torch.Tensor              # float64: assertion 2 of an op that is float32 throughout
    f32_throughout: bool


# ---- weights as the builder folds them ------------------------------------------------------------------------------------------
def fold_conv(sd, p, dt, eps=BN_EPS):
    """Conv2d(bias=False) + BatchNorm2d -> (w float32 rounded once to dt, b float32)"""
    s = sd[p + ".bn.weight"].double() / torch.sqrt(sd[p + ".bn.running_var"].double() + eps)
    w = (sd[p + ".conv.weight"].double() * s.view(-1, 1, 1, 1)).float()
    b = (sd[p + ".bn.bias"].double() - sd[p + ".bn.running_mean"].double() * s).float()
    return store(w, dt), b


def fold_dw(sd, p, eps=BN_EPS):
    """depthwise conv + BatchNorm -> (w float32 [C,1,3,3], b float32): not rounded to the storage type"""
    s = sd[p + ".bn.weight"].double() / torch.sqrt(sd[p + ".bn.running_var"].double() + eps)
    return (sd[p + ".conv.weight"].double() * s.view(-1, 1, 1, 1)).float(), (sd[p + ".bn.bias"].double() - sd[p + ".bn.running_mean"].double() * s).float()


def plain_wb(sd, p, dt):
    """nn.Conv2d(cin, cout, 1) with bias (head rows), nn.ConvTranspose2d(c, c, 2, 2) with bias (Proto)"""
    return store(sd[p + ".weight"].float(), dt), sd[p + ".bias"].float()


# ---- SiLU -----------------------------------------------------------------------------------------------------------------------
def silu64(v):
    return v * torch.sigmoid(v)


def silu_term(v, dt):
    s = silu64(v).abs()
    if dt == torch.float32:
        return 6 * U32 * s + FLUSH
    return (2 * v.abs() + 12) * U32 * s + FLUSH


# ---- conv / plain / deconv ------------------------------------------------------------------------------------------------------
def _c64(x, w, stride, deconv):
    if deconv:
        return F.conv_transpose2d(x.double(), w.double(), None, stride=2)
    return F.conv2d(x.double(), w.double(), None, stride=stride, padding=w.shape[-1] // 2)


def _c32(x, w, b, stride, deconv):
    if deconv:
        return F.conv_transpose2d(x.float(), w, b, stride=2)
    return F.conv2d(x.float(), w, b, stride=stride, padding=w.shape[-1] // 2)


def conv_parts(x, w, b, stride, act, res, dt, deconv=False, f32_rows=False, extra=None):
    """x [1,Cin,H,W] (the channels the weights have), res [1,Cout,Ho,Wo] or None -> (ref, bound, stat), float64.
    extra: an additional float64 error of the ACCUMULATOR (the Bottleneck's intermediate), added behind the Lipschitz factor as is."""
    K = w.shape[0] if deconv else w.shape[1] * w.shape[2] * w.shape[3]            # deconv weight is [Cin, Cout, 2, 2]: one tap per pixel
    bb = b.double().view(1, -1, 1, 1)
    acc = _c64(x, w, stride, deconv) + bb
    mag = _c64(x.abs(), w.abs(), stride, deconv) + bb.abs()
    if res is not None:
        mag = mag + res.double().abs()
    L = SILU_LIPSCHITZ if act else 1.0
    ref = silu64(acc) if act else acc
    s_eval = silu_term(acc, dt) if act else 0.0
    if res is not None:
        ref = ref + res.double()
    u = 0.0 if f32_rows else UNIT_ROUNDOFF[dt]
    tiny = TINY[torch.float32] if f32_rows else TINY[dt]
    rest = s_eval + tiny + (extra if extra is not None else 0.0)
    bound = u * ref.abs() + L * (K + 2) * 2.0 ** -23 * mag + rest
    stat = u * ref.abs() + L * (K + 2) ** 0.5 * 2.0 ** -23 * mag + rest
    return ref, bound, stat


def conv_emulate(x, w, b, stride, act, res, dt, deconv=False, f32_rows=False, res_first=False):
    """plain CPU float32 evaluation, stored once.  res_first: the planted error `residual before SiLU`."""
    y = _c32(x, w, b, stride, deconv)
    if res is not None and res_first:
        y = y + res.float()
    y = F.silu(y) if act else y
    if res is not None and not res_first:
        y = y + res.float()
    return y if f32_rows else store(y, dt)


def conv_reference(x, w, b, stride, act, res, dt, deconv=False, f32_rows=False) -> Judged:
    ref, bound, stat = conv_parts(x, w, b, stride, act, res, dt, deconv, f32_rows)
    return Judged(ref, bound, conv_emulate(x, w, b, stride, act, res, dt, deconv, f32_rows), stat, f32_rows or dt == torch.float32)


def bneck_reference(x, w1, b1, w2, b2, dt) -> Judged:
    """fused Bottleneck x + cv2(cv1(x)), both 3x3 stride 1 + SiLU, the intermediate stored to dt in LDS"""
    ref1, bound1, _ = conv_parts(x, w1, b1, 1, True, None, dt)
    mid = store(ref1, dt)
    d_mid = bound1 + 2 * UNIT_ROUNDOFF[dt] * mid.double().abs()
    extra = F.conv2d(d_mid, w2.double().abs(), None, padding=1)
    ref, bound, stat = conv_parts(mid, w2, b2, 1, True, x, dt, extra=extra)
    emu = conv_emulate(conv_emulate(x, w1, b1, 1, True, None, dt), w2, b2, 1, True, x, dt)
    return Judged(ref, bound, emu, stat, dt == torch.float32)


# ---- depthwise ------------------------------------------------------------------------------------------------------------------
def dw_select(x, C, blk, blk_stride, blk_off):
    """the input channels a depthwise op of C outputs reads, in output order"""
    if not blk:
        return x[:, :C]
    c = torch.arange(C)
    return x[:, (c // blk) * blk_stride + blk_off + c % blk]


def dw_reference(x, w, b, act, add, dt, blk=0, blk_stride=0, blk_off=0) -> Judged:
    C = w.shape[0]
    xs = dw_select(x, C, blk, blk_stride, blk_off)
    bb = b.double().view(1, -1, 1, 1)
    acc = F.conv2d(xs.double(), w.double(), None, padding=1, groups=C) + bb
    mag = F.conv2d(xs.double().abs(), w.double().abs(), None, padding=1, groups=C) + bb.abs()
    if add is not None:
        mag = mag + add.double().abs()
    L = SILU_LIPSCHITZ if act else 1.0
    ref = silu64(acc) if act else acc
    rest = (silu_term(acc, dt) if act else 0.0) + TINY[dt]
    if add is not None:
        ref = ref + add.double()
    u = UNIT_ROUNDOFF[dt]
    bound = u * ref.abs() + L * (9 + 2) * 2.0 ** -23 * mag + rest
    stat = u * ref.abs() + L * (9 + 2) ** 0.5 * 2.0 ** -23 * mag + rest
    y = F.conv2d(xs.float(), w, b, padding=1, groups=C)
    y = F.silu(y) if act else y
    if add is not None:
        y = y + add.float()
    return Judged(ref, bound, store(y, dt), stat, dt == torch.float32)


# ---- exact ops ------------------------------------------------------------------------------------------------------------------
def pool_reference(x, n=3):
    """n cascaded MaxPool2d(5, 1, 2) (-inf border) of x [1,C,H,W] -> [1, n C, H, W], in x's own dtype (exact in any)"""
    out, cur = [], x
    for _ in range(n):
        cur = F.max_pool2d(cur, 5, 1, 2)
        out.append(cur)
    return torch.cat(out, 1)


def up_reference(x):
    return F.interpolate(x, scale_factor=2, mode="nearest")


def exact_failures(name, got, x, fn):
    """an exact op: the device output must EQUAL fn of the device's input, evaluated in float32 and in float64"""
    out = []
    for t in (x.float(), x.double()):
        want = fn(t)
        if want.shape != got.shape or not torch.equal(got.to(t.dtype), want):
            bad = int((got.to(t.dtype) != want).sum()) if want.shape == got.shape else -1
            out.append(f"{name}: {bad} elements differ from the exact result ({t.dtype})")
    return out


# ---- attention ------------------------------------------------------------------------------------------------------------------
def split_qkv(qkv, heads):
    """qkv [heads * 128, N] -> q [h, N, 32], k [h, N, 32], v [h, N, 64]"""
    t = qkv.reshape(heads, 128, -1).permute(0, 2, 1)
    return t[..., :32], t[..., 32:64], t[..., 64:]


def attn_reference(qkv, heads, scale, dt, p_rounded) -> Judged:
    """qkv [heads * 128, N] as stored -> Judged of out [heads * 64, N].  p_rounded: the 16-bit MFMA kernel (P rounded to dt)."""
    q, k, v = (t.double() for t in split_qkv(qkv, heads))
    N = q.shape[1]
    P = torch.softmax(q @ k.transpose(-1, -2) * scale, dim=-1)
    O, A = P @ v, P @ v.abs()
    a = scale * (q.abs() @ k.abs().transpose(-1, -2)).amax(dim=-1, keepdim=True)
    n = (N + 31) // 32
    u = UNIT_ROUNDOFF[dt]
    uP = u if p_rounded else 0.0

    def total(cnt):       # cnt = identity: worst case; sqrt: the statistical form
        e = cnt(32 + 12) * U32 * a + cnt(4 * n + 8) * U32
        E = 2 * e + 2 * cnt(N + n + 10) * U32
        b = (uP + E) * A
        b = b + u * (O.abs() + b) + TINY[dt]
        if dt == torch.float16:
            b = b + (N * 2.0 ** -25 * v.abs().amax(dim=(-1, -2), keepdim=True) if p_rounded else 0.0) + 2.0 ** -25
        return b
    merge = lambda t: t.permute(0, 2, 1).reshape(heads * 64, N)
    qf, kf, vf = (t.float() for t in split_qkv(qkv, heads))
    emu = store(torch.softmax(qf @ kf.transpose(-1, -2) * torch.tensor(scale, dtype=torch.float32), dim=-1) @ vf, dt)
    return Judged(merge(O), merge(total(lambda c: c)), merge(emu), merge(total(math.sqrt)), dt == torch.float32)


def attn_emulate_mfma(qkv, heads, scale, dt, mutation=None):
    """yattn_mfma_kernel's steps in float32: 32-key blocks, running maximum, P rounded to dt for the value product, l from the
    unrounded values, one reciprocal.  mutation: None | "lastkey" (key N - 1 masked) | "noalpha" (no rescale when the maximum moves)
    | "lrounded" (normalised by the sum of the rounded probabilities)"""
    q, k, v = (t.float() for t in split_qkv(qkv, heads))
    N = q.shape[1]
    sc = torch.tensor(scale, dtype=torch.float32)
    m = torch.full((heads, N), -3.0e38)
    l = torch.zeros(heads, N)
    o = torch.zeros(heads, N, 64)
    live = N - 1 if mutation == "lastkey" else N
    for s in range(0, N, 32):
        x = (q @ k[:, s:s + 32].transpose(-1, -2)) * sc
        x = torch.where(torch.arange(s, s + x.shape[-1]) < live, x, torch.tensor(-3.0e38))
        mn = torch.maximum(m, x.amax(dim=-1))
        alpha = torch.exp(m - mn)
        p = torch.exp(x - mn[..., None])
        pr = p.to(dt).float()
        l = l * alpha + (pr if mutation == "lrounded" else p).sum(dim=-1)
        if mutation != "noalpha":
            o = o * alpha[..., None]
        o = o + pr @ v[:, s:s + 32]
        m = mn
    out = store(o * (1.0 / l)[..., None], dt)
    return out.permute(0, 2, 1).reshape(heads * 64, N)


# ---- the two assertions ---------------------------------------------------------------------------------------------------------
def verdict(name, got, j: Judged, dt, kernel=""):
    """-> (failure messages, Report, relL2(got) / yardstick of assertion 2)"""
    rep = check(name, got, j.ref, j.bound)
    tag = f"{name}{' [' + kernel + ']' if kernel else ''}"
    out = []
    if dt == torch.float16 and not rep.ref_absmax < F16_MAX_REF:
        out.append(f"{tag}: |ref| reaches {rep.ref_absmax:.3g}, too close to the float16 range for this check")
    if not rep.ok:
        out.append("assertion 1: " + rep.describe(kernel))
    if j.f32_throughout:
        yard = float(j.stat.norm() / j.ref.norm().clamp_min(1e-300))
        if not rep.rel_l2 <= yard:
            out.append(f"assertion 2 (float32 throughout): {tag}: relL2(got, ref) = {rep.rel_l2:.4g} > || stat || / || ref || = {yard:.4g}")
    else:
        yard = REL_L2_MARGIN * rel_l2(j.emu, j.ref)
        if not rep.rel_l2 <= yard:
            out.append(f"assertion 2: {tag}: relL2(got, ref) = {rep.rel_l2:.4g} > {REL_L2_MARGIN} x relL2(emu, ref) = {yard / REL_L2_MARGIN:.4g}")
    return out, rep, rep.rel_l2 / max(yard / (1.0 if j.f32_throughout else REL_L2_MARGIN), 1e-300)


# ---- one op of the engine's list, from its flope_yolo_op_info words -------------------------------------------------------------
def conv_weights(sd, name, dt, deconv):
    if name + ".conv.weight" in sd:
        return fold_conv(sd, name, dt)
    return plain_wb(sd, name, dt)


def judge_conv_info(sd, info, x, res, dt):
    """info: the words of one conv (kind conv, or one half of a Bottleneck run as two launches) -> Judged"""
    deconv = info["mode"] == 2
    w, b = conv_weights(sd, info["name"], dt, deconv)
    return conv_reference(x[:, :info["cin_w"]], w, b, info["s"], bool(info["act"]), res, dt, deconv, info["mode"] == 1)
