"""Checker of the encoder's attention under a compiled mask (tf_attn_masked_row in flope_amd/csrc/tf_encoder.hip): the
fp64 restatement of the whole masked forward, the test masks and data, an element-wise bound for the masked attention row, and an
emulation of the row's walk that can be broken the way this kernel breaks.  Helper of tests/test_tf_mask_bound.py (CPU: the
restatement against the reference's fixture, the bound against the emulation and its broken copies) and tests/test_gpu_tf_mask.py
(the device output).

Row i of a sequence of n tokens attends to S_i = {j < n : allowed[i, j]}; first / last: its first and last member, span = last -
first + 1, cnt = |S_i|.  Reference, per head and output dim c, in fp64 from the stored q, k, v (T = float32, f16 or bf16):

    P_j = softmax_{j in S_i}(q . k_j / sqrt(hd)),   O_c = sum_j P_j v_jc,   A_c = sum_j P_j |v_jc|   (A >= |O|)

What the row does instead, and what each operation can cost (u = 2^-24; u_T = 2^-24 / 2^-11 / 2^-8):

  1. A probability's float32 value.  score = (fmaf chain over hd from 0.f) * fl(1 / sqrt(hd)); p = expf(score - m), m the row's
     maximum.  An error of the maximum is a common factor and cancels; what does not is a relative error e of a probability's weight.
     With a_j = sum_c |q_c k_jc| / sqrt(hd) (>= |score_j|) and a = max_j a_j:
       - the chain: gamma(hd) sum |q k|; the scaling product and its rounded constant (sqrtf, one division): (hd + 4) u a
       - score - m rounds once, |score - m| <= 2 a: 2 u a                                        argument error <= (hd + 6) u a
       - an argument error dx changes expf by the factor e^dx: relative dx; expf itself is good to 1 ulp: 2 u
     so   e = (hd + 6) u a + 2 u.
  2. Sums in float32.  Denominator: a lane adds at most ceil(span / 64) terms (one per trip of the walk, fewer where a key is masked),
     then six shuffle adds: (ceil(span / 64) + 6) u relative to sum p.  Numerator, per element: ONE fmaf chain over the row's cnt allowed
     keys: cnt u relative to sum p |v|.  The reciprocal (2 u) and, in float32, the final product (u; for f16 it is part of the one output
     rounding): 4 u with slack.
     First order in both:  |sum p~ v / sum p~ - O| <= (2 e + (cnt + ceil(span / 64) + 10) u) A_c  =: E A_c.
  3. The float32 probabilities are NOT rounded to T (they never leave LDS as anything but float32): no u_T A term.
  4. The output is rounded to T once (f16: tf_mul_f16_bits): u_T |O~|, and for f16 at least half the subnormal spacing, 2^-25.

    bound_c = E A_c + u_T (|O_c| + E A_c) + [f16] 2^-25

Nothing in it is fitted to an output: the constants are the worst case of the operation counts above.  The emulation below replays
the walk (lanes based at first, 64-key trips, a masked key skipped, the butterfly sums, the value chain over set bits in ascending
order, output rounding) in float32 and must pass on every test shape; the tests print the headroom.
"""
import functools
import math

import numpy as np
import torch

TDT = {"f32": torch.float32, "f32m": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
U_T = {"f32": 2.0 ** -24, "f32m": 2.0 ** -24, "f16": 2.0 ** -11, "bf16": 2.0 ** -8}
U32 = 2.0 ** -24

LENGTHS = (1, 15, 33, 65, 130)            # one key; inside a word; one bit into the second word; one key into the second trip; a third trip
HEAD_DIMS = (6, 64)                       # element-wise loads (a 12-byte f16 slice); the MFMA kernels' head_dim
KINDS = ("random", "prefix", "band", "edge")
FIRSTS = (31, 32, 63, 64, 65)             # rows of the edge mask whose first allowed key is the row's own index: word and trip boundaries
PREFIX, BAND_K = 5, 3
MUTATIONS = ["nobit", "word31", "base0", "lastdrop", "maskedsum", "skiptrip"]


# ---- masks (bool [L, L], True = ALLOWED) -------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def make_allowed(kind, L, seed=5):
    i, j = torch.arange(L)[:, None], torch.arange(L)[None, :]
    if kind == "clear":
        return torch.ones(L, L, dtype=torch.bool)
    if kind == "causal":
        return j <= i
    if kind == "prefix":                  # prefix-LM: the first PREFIX keys visible to all, causal behind them
        return (j <= i) | (j < PREFIX)
    if kind == "band":                    # every pose sees its neighbours within +-k frames
        return (j - i).abs() <= BAND_K
    g = torch.Generator().manual_seed(seed * 7919 + L)
    a = ~(torch.rand(L, L, generator=g) < 0.4)
    a[torch.arange(L), torch.arange(L)] = True
    if kind == "random":
        return a
    assert kind == "edge"
    # the places this kernel can go wrong: a row whose only key is L - 1, one whose only key is 0, rows whose first key sits at a
    # word or trip boundary (and whose last is L - 1), a 64-key trip without a key between two that have some
    a[0] = False
    a[0, L - 1] = True
    if L > 1:
        a[1] = False
        a[1, 0] = True
    for f in FIRSTS:
        if f < L:
            a[f, :f] = False
            a[f, f] = True
            a[f, L - 1] = True
    if L >= 130:
        a[2] = False
        a[2, [0, 1, 2, 129]] = True       # based at key 0: trip 0 has keys, trip 1 (64 .. 127) none, trip 2 key 129
        a[3] = False
        a[3, [1, 63, 129]] = True         # based at key 1: trips 1 .. 64, 65 .. 128 (none), 129
    return a


def band_causal(L, W):
    i, j = torch.arange(L)[:, None], torch.arange(L)[None, :]
    return (j <= i) & (j > i - W)


def block_diagonal(lengths, causal=False):
    L = sum(lengths)
    a = torch.zeros(L, L, dtype=torch.bool)
    o = 0
    for n in lengths:
        a[o:o + n, o:o + n] = torch.ones(n, n, dtype=torch.bool).tril() if causal else True
        o += n
    return a


def to_torch_mask(allowed, floating=False):
    """allowed -> torch's mask: bool True = masked, or floating -inf / 0"""
    return torch.zeros(allowed.shape).masked_fill(~allowed, float("-inf")) if floating else ~allowed


# ---- the whole forward in fp64 -------------------------------------------------------------------------------------------------------
def _ln(x, w, b):
    mu = x.mean(-1, keepdims=True)
    var = ((x - mu) ** 2).mean(-1, keepdims=True)
    return (x - mu) / np.sqrt(var + 1e-5) * w + b


def masked_forward(sd, x, allowed, lengths=None, num_heads=4):
    """The reference module under mask = ~allowed, restated in fp64 numpy: x [B, L, in] -> [B, L, out].  lengths: sequence b is
    x[b, :lengths[b]], encoded alone under allowed[:n, :n]; the rows behind it are out_layer.bias."""
    g = lambda k: np.asarray(sd[k], dtype=np.float64)
    x = np.asarray(x, dtype=np.float64)
    allowed = np.asarray(allowed, dtype=bool)
    B, L = x.shape[0], x.shape[1]
    nl = 0
    while f"transformer_encoder.layers.{nl}.norm1.weight" in sd:
        nl += 1
    out = np.broadcast_to(g("out_layer.bias"), (B, L, g("out_layer.bias").shape[0])).copy()
    for b in range(B):
        n = L if lengths is None else int(lengths[b])
        ok = allowed[:n, :n]
        h = x[b, :n] @ g("embedding.weight").T + g("embedding.bias")
        d = h.shape[1]
        dh = d // num_heads
        for i in range(nl):
            p = f"transformer_encoder.layers.{i}."
            qkv = h @ g(p + "self_attn.in_proj_weight").T + g(p + "self_attn.in_proj_bias")
            q, k, v = (qkv[:, t * d:(t + 1) * d].reshape(n, num_heads, dh).transpose(1, 0, 2) for t in range(3))
            s = q @ k.transpose(0, 2, 1) / np.sqrt(dh)
            s = np.where(ok[None], s, -np.inf)
            s = s - s.max(-1, keepdims=True)
            pr = np.exp(s)
            pr = pr / pr.sum(-1, keepdims=True)
            a = (pr @ v).transpose(1, 0, 2).reshape(n, d) @ g(p + "self_attn.out_proj.weight").T + g(p + "self_attn.out_proj.bias")
            h = _ln(h + a, g(p + "norm1.weight"), g(p + "norm1.bias"))
            f = np.maximum(h @ g(p + "linear1.weight").T + g(p + "linear1.bias"), 0) @ g(p + "linear2.weight").T + g(p + "linear2.bias")
            h = _ln(h + f, g(p + "norm2.weight"), g(p + "norm2.bias"))
        out[b, :n] = h @ g("out_layer.weight").T + g("out_layer.bias")
    return out


# ---- the attention row: data, reference, bound ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def make_qkv(B, L, H, hd, dtype, seed=7):
    """Standard-normal q, k, v rounded to T, [B, L, 3 H hd]"""
    g = torch.Generator().manual_seed(seed * 1000003 + B * 7919 + L * 31 + H * 5 + hd)
    return torch.randn(B, L, 3 * H * hd, generator=g).to(TDT[dtype])


def _lens(B, L, lengths):
    return [L] * B if lengths is None else [int(v) for v in lengths]


def reference_of(qkv, allowed, H, dtype, lengths=None):
    """(O, bound) in fp64, both [B, L, d]; rows behind a length are 0 with bound 0"""
    qkv = qkv.cpu().double()
    B, L, d3 = qkv.shape
    d = d3 // 3
    hd = d // H
    uT = U_T[dtype]
    O = torch.zeros(B, L, d, dtype=torch.float64)
    Bd = torch.zeros(B, L, d, dtype=torch.float64)
    for b, n in enumerate(_lens(B, L, lengths)):
        ok = allowed[:n, :n]
        q, k, v = (qkv[b, :n, t * d:(t + 1) * d].reshape(n, H, hd).permute(1, 0, 2) for t in range(3))      # [H, n, hd]
        s = torch.einsum("hic,hjc->hij", q, k) / math.sqrt(hd)
        P = torch.softmax(s.masked_fill(~ok[None], float("-inf")), dim=-1)
        o = torch.einsum("hij,hjc->hic", P, v)
        A = torch.einsum("hij,hjc->hic", P, v.abs())
        a = (torch.einsum("hic,hjc->hij", q.abs(), k.abs()) / math.sqrt(hd)).masked_fill(~ok[None], 0.0).amax(dim=-1, keepdim=True)   # [H, n, 1]
        cnt = ok.sum(dim=1).double()
        idx = torch.arange(n)
        first = torch.where(ok, idx[None, :], torch.full((1, 1), n)).amin(dim=1)
        last = torch.where(ok, idx[None, :], torch.full((1, 1), -1)).amax(dim=1)
        trips = torch.ceil((last - first + 1).double() / 64)
        e = (hd + 6) * U32 * a + 2 * U32
        E = 2 * e + ((cnt + trips + 10) * U32)[None, :, None]
        bound = E * A
        bound = bound + uT * (o.abs() + bound)
        if dtype == "f16":
            bound = bound + 2.0 ** -25
        O[b, :n] = o.permute(1, 0, 2).reshape(n, d)
        Bd[b, :n] = bound.permute(1, 0, 2).reshape(n, d)
    return O, Bd


@functools.lru_cache(maxsize=None)
def reference(kind, B, L, H, hd, dtype, lengths=None):
    """reference_of(make_qkv(...), make_allowed(kind, L)); lengths: None or a tuple"""
    return reference_of(make_qkv(B, L, H, hd, dtype), make_allowed(kind, L), H, dtype, lengths)


def ratio(got, ref, bound, lengths=None):
    """max over the valid elements of |got - ref| / bound, and where; a non-finite output counts as infinitely wrong"""
    g = got.detach().cpu().double().reshape(ref.shape)
    valid = torch.zeros(ref.shape, dtype=torch.bool)
    for b, n in enumerate(_lens(ref.shape[0], ref.shape[1], lengths)):
        valid[b, :n] = True
    r = (g - ref).abs() / bound.clamp_min(1e-300)
    r = torch.where(torch.isfinite(g), r, torch.full_like(r, float("inf")))
    r = torch.where(valid, r, torch.zeros_like(r))
    i = int(r.argmax())
    return float(r.reshape(-1)[i]), tuple(int(t) for t in torch.unravel_index(torch.tensor(i), r.shape))


# ---- the walk ---------------------------------------------------------------------------------------------------------------------------
def _fma(a, b, c):
    """float32 fmaf: the product is exact in fp64, the sum rounds to fp64 and then to float32"""
    return (a.double() * b.double() + c.double()).float()


def _wave_sum(v):
    """wave_sum: v += shfl_xor(v, o) for o = 32 .. 1 on 64 lanes (last dim)"""
    lanes = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[..., lanes ^ o]
    return v


def emulate(qkv, allowed, H, dtype, lengths=None, mutation=None):
    """The row's walk in torch float32 on the CPU -> [B, L, d] in T (rows behind a length: 0).  mutation: None, or one defect
         nobit      the mask bit ignored: every key of first .. last taken
         word31     bits 31 and 32 of a row swapped (the word boundary)
         base0      lanes based at key 0 instead of first, the trip count still that of first .. last
         lastdrop   the last allowed key dropped
         maskedsum  a masked key's p counted in the sum
         skiptrip   the keys of the trip behind a trip without keys lost"""
    dt = TDT[dtype]
    qkv = qkv.cpu()
    B, L, d3 = qkv.shape
    d = d3 // 3
    hd = d // H
    scale = (torch.tensor(1.0) / torch.sqrt(torch.tensor(float(hd)))).float()
    out = torch.zeros(B, L, d, dtype=dt)
    for b, n in enumerate(_lens(B, L, lengths)):
        ok = allowed[:n, :n].clone()
        if mutation == "word31" and n > 32:
            ok[:, [31, 32]] = ok[:, [32, 31]]
        x = qkv[b, :n].float()
        q, k, v = (x[:, t * d:(t + 1) * d].reshape(n, H, hd).permute(1, 0, 2) for t in range(3))          # [H, n, hd]
        for i in range(n):
            cols = ok[i].nonzero().reshape(-1)
            if not len(cols):
                continue
            first, last = int(cols[0]), int(cols[-1])
            if mutation == "lastdrop":
                last -= 1
                if last < first:
                    out[b, i] = float("nan")
                    continue
            trips = (last - first) // 64 + 1
            base = 0 if mutation == "base0" else first
            width = trips * 64
            js = base + torch.arange(width)                                     # key of (trip, lane) = base + 64 trip + lane
            inside = (js >= first) & (js <= last) & (js < n)
            bit = torch.zeros(width, dtype=torch.bool)
            bit[inside] = ok[i, js[inside]]
            scored = inside.clone() if mutation == "nobit" else bit.clone()
            if mutation == "skiptrip":
                has = scored.view(trips, 64).any(dim=1)
                for t in range(1, trips):
                    if not has[t - 1] and has[t]:
                        scored[t * 64:(t + 1) * 64] = False
            if not bool(scored.any()):
                out[b, i] = float("nan")
                continue
            jj = js.clamp(0, n - 1)
            s = torch.zeros(H, width)
            for c in range(hd):                                                 # one fmaf chain per key over c = 0 .. hd - 1 from 0.f
                s = _fma(q[:, i, c][:, None].expand(H, width), k[:, jj, c], s)
            s = s * scale
            mx = s.masked_fill(~scored[None], float("-inf")).amax(dim=1, keepdim=True)
            p = torch.exp(s - mx)
            summed = scored | (inside & ~bit) if mutation == "maskedsum" else scored
            pl = p.masked_fill(~summed[None], 0.0).view(H, trips, 64)
            lane = torch.zeros(H, 64)
            for t in range(trips):                                              # a lane's sum in trip order
                lane = lane + pl[:, t]
            tot = _wave_sum(lane)[:, 0]
            inv = (1.0 / tot)
            o = torch.zeros(H, hd)
            for w in scored.nonzero().reshape(-1).tolist():                     # the set bits in ascending key order
                o = _fma(p[:, w][:, None].expand(H, hd), v[:, int(jj[w])], o)
            res = o.double() * inv.double()[:, None] if dtype == "f16" else (o * inv[:, None])     # f16: the product rounds once, to T
            out[b, i] = res.reshape(-1).to(dt)
    return out
