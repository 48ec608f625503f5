"""Element-wise checker of the float32 MFMA attention of the encoder (tf_attn_f32m<NT, VARLEN, CAUSAL> in flope_amd/csrc/tf_encoder.hip,
dtype="f32m", kernel id 3): the fp64 reference computed from the float32 inputs as given, a bound for every output
element and its statistical form, test data, and an emulation of the kernel's three passes that can be broken the way this kernel
breaks.  Helper of tests/test_tf_attn_f32m_bound.py (CPU: both assertions pass the emulation and fail its broken copies) and
tests/test_gpu_tf_attn_f32m.py (the device output).

Reference, per (sequence, head), query i, output dim c, in fp64 from the stored q, k, v.  S_i: the keys query i sees -- all n of its
sequence, under causal keys 0 .. i; n_i = |S_i|:

    P_ij = softmax_{j in S_i}(q_i . k_j / sqrt(hd)),   O_ic = sum_j P_ij v_jc,   A_ic = sum_j P_ij |v_jc|   (A >= |O|)
    a_ij = sum_c |q_ic k_jc| / sqrt(hd)  (>= |score_ij|),   a_i = max_{j in S_i} a_ij

What the kernel does instead, and what each operation can cost (u = 2^-24; every count is the worst case of the operations as
written in the kernel, first order in u):

  1. A probability's float32 value.  score = (MFMA chain over head_dim) * scale, e = expf(score - m), m the row's maximum.  An error
     of the maximum is a common factor of numerator and denominator and cancels; what does not is a relative error eps_ij of e_ij:
       - the dot product: hd products accumulated from a zero accumulator by v_mfma_f32_16x16x4_f32 (the fragments of dims >= hd
         are zero and add nothing).  In whatever order the hardware adds them that is at most hd - 1 roundings on the path of a
         product, and one more if the product itself is rounded before it is added:                     hd u a_i
       - scale = fl(1 / fl(sqrtf(hd))) on the host, two correctly rounded operations, and score = fl(dot * scale):     3 u a_i
       - score - m rounds once and |score - m| <= 2 a_i:                                                              2 u a_i
                                                                                         argument error <= (hd + 5) u a_i
       - an argument error dx changes expf by the factor e^dx: relative dx; expf itself is good to 1 ulp (the build has no
         fast-math: ocml's expf, documented 1 ulp):                                                                   2 u
     so   eps_i = (hd + 5) u a_i + 2 u.
  2. The denominator.  A lane adds ceil(n_i / 16) terms from 0.f (the first addition is exact), then four butterfly additions; every
     term is positive, so relative to sum e:                                                         (ceil(n_i / 16) + 3) u
     inv = 1.f / l is one correctly rounded division (no fast-math, hipcc's default correctly rounded divide): u, common to the row
     and NOT cancelled by anything behind it.  p = fl(e * inv) rounds once more per probability before the value pass -- a term the
     row kernels, which scale the finished sum, do not have:                                                          u + u
  3. The values.  Lw = the whole 16-key tiles the workgroup walks (all of them; under causal up to the tile of its last query).  A
     wave takes every fourth group of 4 keys, so Lw / 4 products per output in one wave's accumulator chain (zero probabilities
     included, they add nothing): at most Lw / 4 - 1 roundings on a product's path and one for the product; then the other three
     waves' partial sums are added in wave order: 3.  Relative to sum p |v|:                                   (Lw / 4 + 3) u
  4. The store is float32: no storage rounding.

     First order, with the probability error once in the numerator and once in the denominator:
         |got - O| <= E_i A_ic,    E_i = 2 (hd + 5) u a_i + (Lw / 4 + ceil(n_i / 16) + 12) u
     (12 = 2 x 2 for expf + 3 + 1 + 1 + 3.)
  5. tiny.  Where e, p = e * inv or a product p v falls below 2^-126 the result may be flushed or rounded as a subnormal:
     absolute 2^-126 at most each, the weight of e being <= 1 (l >= 1: the maximum's own e is 1), n keys:
         tiny_c = 3 n 2^-126 max_j |v_jc| + 2^-149

    bound_ic = E_i A_ic + tiny_c                                                                               (assertion 1)

Assertion 2 (float32 throughout, so the form of oracle/conv_bound.py: statistical_bound and oracle/yolo_op_bound.py):
relL2(got, ref) <= || stat || / || ref ||, stat = the same bound with every operation count under a square root,
    E_i(stat) = 2 sqrt(hd + 5) u a_i + sqrt(Lw / 4 + ceil(n_i / 16) + 12) u.  No margin.

Nothing here is fitted to an output.  The emulation below replays the kernel (the MFMA as the k-ordered float32 fmaf chain the
instruction is documented to be) and must pass both assertions on every test shape; the tests print the headroom.
"""
import functools
import math
from collections import namedtuple

import torch

from tf_attn_bound import merge_heads, ratio, split_heads       # noqa: F401  (ratio is the tests' assertion 1)

U32 = 2.0 ** -24
F32M = 3
KINDS = ("normal", "peaked", "offset")
RAGGED = (1, 17, 64, 5, 33)

MUTATIONS = ["p16", "pbf", "opnd10", "scale64", "nomask", "pair", "wave3", "qfrag", "head0v", "causal_lt", "rowL", "noshfl8"]

Case = namedtuple("Case", "B L H hd kind")


def _cases():
    """(L, hd) pairs: every head dim and every length at least once, the part-used head-dim tiles (4, 12, 20, 36, 68, 100) next to
    the tile-edge lengths; the three data kinds on the small shapes, `normal` on the large ones."""
    small = [(1, 4), (15, 4), (17, 4), (16, 12), (17, 12), (33, 12), (15, 16), (33, 16), (16, 20), (17, 20), (33, 20),
             (15, 36), (17, 68), (16, 100)]
    large = [(64, 32), (129, 32), (65, 36), (65, 64), (129, 64), (257, 68), (129, 100), (257, 16), (577, 128), (577, 4)]
    out = [Case(2, L, 3 if (L, hd) == (33, 16) else 2, hd, kind) for L, hd in small for kind in KINDS]
    out += [Case(1 if L > 129 else 2, L, 2, hd, "normal") for L, hd in large]
    return out


CASES = _cases()
RAGGED_CASES = [(12, "normal"), (12, "peaked"), (12, "offset"), (20, "normal"), (20, "peaked"), (20, "offset"), (36, "normal"),
                (68, "normal")]      # (head_dim, kind) of the ragged batches, H = 2: one per NT


def case_id(c):
    return "B%d-L%d-H%d-hd%d-%s" % tuple(c)


def nt_of(hd):
    """16-wide head-dim tiles the kernel is built for (tf_attn_f32m_nt of tf_attn_plan.h)"""
    return 1 if hd <= 16 else 2 if hd <= 32 else 4 if hd <= 64 else 8


def lds_limit(plan, hd):
    """the largest L that tf_attn_pick (through the host harness) still sends to tf_attn_f32m at this head_dim"""
    pick = lambda L: plan.tf_attn_pick(2, hd, L, 0, 1, 0, 1)
    lo, hi = 1, 1 << 20                     # pick(lo) == F32M, pick(hi) != F32M; the LDS need grows with L
    assert pick(lo) == F32M and pick(hi) != F32M
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if pick(mid) == F32M else (lo, mid)
    return lo


# ---- data ------------------------------------------------------------------------------------------------------------------------------
def _sequence(kind, n, H, hd, g):
    x = torch.randn(n, 3, H, hd, generator=g)
    if kind == "peaked":                  # one key of the first 16-key tile and one of the last scaled by 4
        x[3 % n, 1] *= 4.0
        x[(n - 1) // 16 * 16 + ((n - 1) % 16) // 2, 1] *= 4.0
    elif kind == "offset":                # a large component common to the keys of a head: a_i large, score differences small
        x[:, 1] = 0.25 * x[:, 1] + 3.0 * torch.randn(1, H, hd, generator=g)
    else:
        assert kind == "normal"
    return x.reshape(n, 3 * H * hd)


@functools.lru_cache(maxsize=None)
def make_qkv(kind, B, L, H, hd, seed=3):
    """float32 q, k, v [B, L, 3 H hd]"""
    g = torch.Generator().manual_seed(seed * 1000003 + B * 7919 + L * 31 + H * 5 + hd)
    return torch.stack([_sequence(kind, L, H, hd, g) for _ in range(B)])


@functools.lru_cache(maxsize=None)
def make_ragged(kind, lengths, H, hd, seed=3):
    """one float32 [n, 3 H hd] per length (a tuple); a sequence depends on its index in `lengths`, not on its place in a batch"""
    return [_sequence(kind, n, H, hd, torch.Generator().manual_seed(seed * 1000003 + i * 7919 + n * 31 + H * 5 + hd))
            for i, n in enumerate(lengths)]


# ---- reference and bounds ----------------------------------------------------------------------------------------------------------
Judged = namedtuple("Judged", "ref bound stat")


def _judge_sequence(seq, H, causal):
    """seq [n, 3 d] -> (O, bound, stat), each [n, d] in fp64"""
    q, k, v = (t[0].double() for t in split_heads(seq[None], H))                       # [H, n, hd]
    n, hd = q.shape[1], q.shape[2]
    i, j = torch.arange(n)[:, None], torch.arange(n)[None, :]
    seen = (j <= i) if causal else torch.ones(n, n, dtype=torch.bool)
    s = (q @ k.transpose(-1, -2) / math.sqrt(hd)).masked_fill(~seen, float("-inf"))
    P = torch.softmax(s, dim=-1)
    O, A = P @ v, P @ v.abs()
    a = (q.abs() @ k.abs().transpose(-1, -2) / math.sqrt(hd)).masked_fill(~seen, 0.0).amax(dim=-1, keepdim=True)     # [H, n, 1]
    rows = torch.arange(n)
    ni = torch.clamp(rows + 1, max=n) if causal else torch.full((n,), n)
    Lw = (torch.clamp(rows // 16 * 16 + 16, max=n) + 15) // 16 * 16 if causal else torch.full((n,), (n + 15) // 16 * 16)
    sums = (Lw // 4 + (ni + 15) // 16 + 12).double()[None, :, None]
    tiny = 3 * n * 2.0 ** -126 * v.abs().amax(dim=1, keepdim=True) + 2.0 ** -149
    total = lambda cnt: (2 * cnt(torch.tensor(hd + 5.0)) * U32 * a + cnt(sums) * U32) * A + tiny
    flat = lambda t: merge_heads(t[None])[0]
    return flat(O), flat(total(lambda c: c)), flat(total(torch.sqrt))


def reference_of(qkv, H, lengths=None, causal=False):
    """Judged(ref, bound, stat) in fp64, shaped like the output: [B, L, d] for qkv [B, L, 3 d], packed [T, d] with `lengths`"""
    qkv = qkv.detach().cpu()
    if lengths is None:
        parts = [_judge_sequence(seq, H, causal) for seq in qkv]
        return Judged(*(torch.stack([p[t] for p in parts]) for t in range(3)))
    off = [0]
    for n in lengths:
        off.append(off[-1] + int(n))
    parts = [_judge_sequence(qkv[off[b]:off[b + 1]], H, causal) for b in range(len(lengths))]
    return Judged(*(torch.cat([p[t] for p in parts]) for t in range(3)))


@functools.lru_cache(maxsize=None)
def reference(case, causal=False):
    return reference_of(make_qkv(case.kind, case.B, case.L, case.H, case.hd), case.H, causal=causal)


@functools.lru_cache(maxsize=None)
def reference_ragged(kind, lengths, H, hd, causal=False):
    return reference_of(torch.cat(make_ragged(kind, lengths, H, hd)), H, lengths=lengths, causal=causal)


def rel_l2(got, j):
    """assertion 2: (relL2(got, ref), || stat || / || ref ||)"""
    nrm = j.ref.norm().clamp_min(1e-300)
    return float((got.detach().cpu().double().reshape(j.ref.shape) - j.ref).norm() / nrm), float(j.stat.norm() / nrm)


def verdict(got, j):
    """-> (max err / bound, where, relL2 / yardstick); the output passes when both ratios are <= 1"""
    r, where = ratio(got.reshape(j.ref.shape), j.ref, j.bound)
    rel, yard = rel_l2(got, j)
    finite = bool(torch.isfinite(got).all())
    return r, where, (rel / max(yard, 1e-300) if finite else float("inf"))


# ---- the kernel's three passes -----------------------------------------------------------------------------------------------------------
def _fma(a, b, c):
    """float32 fmaf: the product is exact in fp64, the sum rounds to fp64 and then to float32"""
    return (a.double() * b.double() + c.double()).float()


def _trunc10(t):
    """float32 with the mantissa cut to 10 bits"""
    return (t.contiguous().view(torch.int32) & ~0x1FFF).view(torch.float32)


def _emulate_sequence(buf, row0, n, Lclamp, H, causal, mutation):
    d = buf.shape[1] // 3
    hd = d // H
    NT, Lp = nt_of(hd), (n + 15) // 16 * 16
    keys = row0 + torch.arange(Lp).clamp(max=Lclamp - 1)                 # min(key, L - 1): the load of a key past the sequence
    heads = lambda t: t.reshape(-1, H, hd).permute(1, 0, 2).contiguous()
    q, k, v = heads(buf[row0:row0 + n, :d]), heads(buf[keys, d:2 * d]), heads(buf[keys, 2 * d:])      # [H, n | Lp, hd]
    if mutation == "head0v":
        v = v[0:1].expand(H, -1, -1)
    if mutation == "opnd10":
        q, k = _trunc10(q), _trunc10(k)
    # 1. scores: MFMA (st, s) adds dims st 16 + 4 kq + s, kq = 0 .. 3, in that order to the accumulator
    acc = torch.zeros(H, n, Lp)
    for st in range(NT):
        for s in range(4):
            for kq in range(4):
                dim = st * 16 + 4 * kq
                c = min(dim, hd - 4) + s
                if dim < hd or mutation == "qfrag":                      # else: the query fragment is zero, fmaf(k, 0, acc) = acc
                    acc = _fma(k[:, None, :, c], q[:, :, None, c], acc)
    scale = (torch.tensor(1.0) / torch.sqrt(torch.tensor(64.0 if mutation == "scale64" else float(hd)))).float()
    i, j = torch.arange(n)[:, None], torch.arange(Lp)[None, :]
    cnt = torch.clamp(i + (0 if mutation == "causal_lt" else 1), max=n) if causal else torch.full((n, 1), n)      # this query's keys
    if mutation == "nomask":
        cnt = torch.where(cnt == n, torch.full_like(cnt, Lp), cnt)
    valid = j < cnt
    S = torch.where(valid, acc * scale, torch.tensor(-3.0e38))
    if mutation == "pair":                                               # tiles kt + 4 of (kt, kt + 4) never written: LDS as it was, 0.f
        S[:, :, (j[0] // 16) % 8 >= 4] = 0.0
    # 2. softmax: lane kl of a query takes keys kl, kl + 16, ...
    mx = S.masked_fill(~valid, -3.0e38).amax(dim=-1, keepdim=True)
    e = torch.where(valid, torch.exp(S - mx), torch.tensor(0.0))
    lane = torch.zeros(H, n, 16)
    for t in range(Lp // 16):
        lane = lane + e[:, :, t * 16:(t + 1) * 16]
    lanes = torch.arange(16)
    for o in (8, 4, 2, 1):
        if not (mutation == "noshfl8" and o == 8):
            lane = lane + lane[..., lanes ^ o]
    inv = 1.0 / lane
    p = torch.where(valid, e * inv.repeat(1, 1, Lp // 16), torch.tensor(0.0))            # zeros up to Lw
    if mutation == "p16":
        p = p.half().float()
    if mutation == "pbf":
        p = p.bfloat16().float()
    # 3. values: group g = keys 4 g .. 4 g + 3 goes to wave g % 4, in ascending g; a probability of 0 adds nothing, so walking every
    #    tile gives the bits of walking Lw
    part = []
    for w in range(4):
        o = torch.zeros(H, n, hd)
        for g in range(w, Lp // 4, 4):
            for kq in range(4):
                o = _fma(v[:, None, 4 * g + kq, :], p[:, :, 4 * g + kq, None], o)
        part.append(o)
    out = part[0]
    for w in range(1, 3 if mutation == "wave3" else 4):
        out = out + part[w]
    return out.permute(1, 0, 2).reshape(n, d)


def emulate(qkv, H, lengths=None, causal=False, mutation=None):
    """tf_attn_f32m's passes in torch float32 on the CPU: [B, L, 3 d] -> [B, L, d], or packed [T, 3 d] -> [T, d] with `lengths`.
    The packed rows are followed by NaN rows, as on the device.  mutation: None, or one defect
         p16, pbf   P rounded to f16 / bf16 before the value pass
         opnd10     score operands truncated to 10 mantissa bits
         scale64    scale of head_dim 64 whatever hd is
         nomask     the keys L .. Lp - 1 of the last tile (the clamped load of key L - 1) keep their score and their place in the softmax
         pair       the kt + 4 tile of a pair is never written
         wave3      wave 3's partial sums are not added
         qfrag      the query fragment for dims >= hd is not zeroed, so the clamped dims count twice
         head0v     heads >= 1 read head 0's V
         causal_lt  key < query instead of <=
         rowL       with lengths, a sequence's clamp uses the batch's longest L, so it reads the next sequence's rows
         noshfl8    the first butterfly step of the sum is missing"""
    assert mutation is None or mutation in MUTATIONS
    qkv = qkv.detach().cpu().float()
    shape = None
    if lengths is None:
        shape = qkv.shape
        lengths = [shape[1]] * shape[0]
        qkv = qkv.reshape(shape[0] * shape[1], shape[2])
    buf = torch.cat([qkv, torch.full((max(64, max(lengths)), qkv.shape[1]), float("nan"))])
    out, row0 = [], 0
    for n in lengths:
        n = int(n)
        out.append(_emulate_sequence(buf, row0, n, max(lengths) if mutation == "rowL" else n, H, causal, mutation))
        row0 += n
    out = torch.cat(out)
    return out if shape is None else out.reshape(shape[0], shape[1], -1)
