"""Checker of the encoder's attention under a compiled additive bias (tf_attn_masked_row<T, BIASED> in flope_amd/csrc/tf_encoder.hip; DESIGN.md
39): the fp64 restatement of the whole biased forward, the test biases, an element-wise bound for the biased attention row, and an
emulation of the row's walk that can be broken the way this kernel breaks.  Helper of tests/test_tf_bias_bound.py (CPU: the
restatement against the reference's fixture, the bound against the emulation and its broken copies) and tests/test_gpu_tf_bias.py
(the device output).  Masks, data, `ratio` and the float32 helpers are tests/tf_attn_mask_bound.py's.

A bias is float32 [P, L, L], P = 1 (one plane for every head) or H; -inf = masked, and the masked entries are the same in every plane.
Row i of head h of a sequence of n tokens attends to S_i = {j < n : bias[0, i, j] > -inf}; first / last / span / cnt as for a mask.
Reference, per head and output dim c, in fp64 from the stored q, k, v (T = float32, f16 or bf16) and the stored float32 bias b:

    P_j = softmax_{j in S_i}(q . k_j / sqrt(hd) + b_ij),   O_c = sum_j P_j v_jc,   A_c = sum_j P_j |v_jc|   (A >= |O|)

The bound is tests/tf_attn_mask_bound.py's with the one add accounted for (u = 2^-24; u_T = 2^-24 / 2^-11 / 2^-8).  With
a_j = sum_c |q_c k_jc| / sqrt(hd), a = max_j a_j, and now also ab = max_j (a_j + |b_ij|), both over the allowed keys:

  1. A probability's float32 value.  score = fl(fl(chain * fl(1 / sqrt(hd))) + b_ij); p = expf(score - m), m the row's maximum.
       - the chain, the scaling product and its rounded constant, as before: (hd + 4) u a
       - NEW the add rounds once, and its exact value is at most a_j + |b_ij| in magnitude: u (a_j + |b_ij|) <= u ab
       - score - m rounds once; every score is now at most ab in magnitude, so |score - m| <= 2 ab: 2 u ab  (was 2 u a: the later use
         of a_j has become a_j + |b_ij|)
       - an argument error dx is a relative error dx of the weight; expf itself is good to 1 ulp: 2 u
     so   e = (hd + 4) u a + 3 u ab + 2 u          (b = 0: ab = a and e = (hd + 7) u a + 2 u, one u a above the mask's: the add is
                                                    still made, and rounds nothing there)
  2. - 4. unchanged: the sums (cnt + ceil(span / 64) + 10) u, no rounding of p to T, one output rounding.

    E = 2 e + (cnt + ceil(span / 64) + 10) u,     bound_c = E A_c + u_T (|O_c| + E A_c) + [f16] 2^-25

Nothing in it is fitted to an output.  The emulation below replays the walk with the add as its own float32 rounding and must pass on
every test shape; its broken copies (MUTATIONS) must each fail.
"""
import functools
import math

import numpy as np
import torch

import tf_attn_mask_bound as MB
from tf_attn_mask_bound import HEAD_DIMS, LENGTHS, TDT, U32, U_T, make_qkv, ratio  # noqa: F401

NINF = float("-inf")
KINDS = ("holes", "alibi", "edge")        # 2 randn per head over the random allowed set; per-head causal ALiBi; 2 randn per head over the edge mask
MUTATIONS = ["nobias", "plane0", "lanerel", "transposed", "prescale", "cornerstride"]


# ---- biases (float32 [P, L, L]) -------------------------------------------------------------------------------------------------------
def alibi(L, slopes, causal=True):
    """-slopes[h] |i - j|, -inf above the diagonal when causal: what flope_amd.tf_encoder.alibi_bias must return"""
    i, j = torch.arange(L)[:, None], torch.arange(L)[None, :]
    b = -torch.tensor(slopes, dtype=torch.float32)[:, None, None] * (i - j).abs().float()[None]
    return b.masked_fill((j > i)[None], NINF) if causal else b


def over(allowed, values):
    """values [P, L, L] with -inf where the pair is not allowed"""
    return values.float().masked_fill(~allowed[None], NINF).contiguous()


@functools.lru_cache(maxsize=None)
def make_bias(kind, L, H, planes=None, seed=13):
    """The test bias of `kind` for sequences of L tokens and H heads; planes: H (default) or 1"""
    P = H if planes is None else planes
    if kind == "alibi":
        return alibi(L, [2.0 ** -(h + 1) for h in range(P)])
    g = torch.Generator().manual_seed(seed * 104729 + L * 31 + P)
    return over(MB.make_allowed("random" if kind == "holes" else kind, L), 2 * torch.randn(P, L, L, generator=g))


def allowed_of(bias):
    return bias[0] > NINF


# ---- the whole forward in fp64 -------------------------------------------------------------------------------------------------------
def biased_forward(sd, x, bias, lengths=None, num_heads=4):
    """The reference module under the float mask `bias` ([L, L], or [H, L, L]: head h of every batch element under plane h), restated
    in fp64 numpy: tests/tf_attn_mask_bound.py's masked_forward plus the bias on the scaled scores.  lengths: sequence b is
    x[b, :lengths[b]], encoded alone under bias[..., :n, :n]; the rows behind it are out_layer.bias."""
    g = lambda k: np.asarray(sd[k], dtype=np.float64)
    x = np.asarray(x, dtype=np.float64)
    bias = np.asarray(bias, dtype=np.float64)
    if bias.ndim == 2:
        bias = bias[None]
    B, L = x.shape[0], x.shape[1]
    nl = 0
    while f"transformer_encoder.layers.{nl}.norm1.weight" in sd:
        nl += 1
    out = np.broadcast_to(g("out_layer.bias"), (B, L, g("out_layer.bias").shape[0])).copy()
    for b in range(B):
        n = L if lengths is None else int(lengths[b])
        bb = bias[:, :n, :n]
        h = x[b, :n] @ g("embedding.weight").T + g("embedding.bias")
        d = h.shape[1]
        dh = d // num_heads
        for i in range(nl):
            p = f"transformer_encoder.layers.{i}."
            qkv = h @ g(p + "self_attn.in_proj_weight").T + g(p + "self_attn.in_proj_bias")
            q, k, v = (qkv[:, t * d:(t + 1) * d].reshape(n, num_heads, dh).transpose(1, 0, 2) for t in range(3))
            s = q @ k.transpose(0, 2, 1) / np.sqrt(dh) + bb
            s = s - s.max(-1, keepdims=True)
            pr = np.exp(s)
            pr = pr / pr.sum(-1, keepdims=True)
            a = (pr @ v).transpose(1, 0, 2).reshape(n, d) @ g(p + "self_attn.out_proj.weight").T + g(p + "self_attn.out_proj.bias")
            h = MB._ln(h + a, g(p + "norm1.weight"), g(p + "norm1.bias"))
            f = np.maximum(h @ g(p + "linear1.weight").T + g(p + "linear1.bias"), 0) @ g(p + "linear2.weight").T + g(p + "linear2.bias")
            h = MB._ln(h + f, g(p + "norm2.weight"), g(p + "norm2.bias"))
        out[b, :n] = h @ g("out_layer.weight").T + g("out_layer.bias")
    return out


# ---- the attention row: reference and bound -----------------------------------------------------------------------------------------
def reference_of(qkv, bias, H, dtype, lengths=None):
    """(O, bound) in fp64, both [B, L, d]; rows behind a length are 0 with bound 0"""
    qkv = qkv.cpu().double()
    B, L, d3 = qkv.shape
    d = d3 // 3
    hd = d // H
    uT = U_T[dtype]
    bias = bias.double().expand(H, L, L)
    O = torch.zeros(B, L, d, dtype=torch.float64)
    Bd = torch.zeros(B, L, d, dtype=torch.float64)
    for b, n in enumerate(MB._lens(B, L, lengths)):
        bb = bias[:, :n, :n]
        ok = bb[0] > NINF
        q, k, v = (qkv[b, :n, t * d:(t + 1) * d].reshape(n, H, hd).permute(1, 0, 2) for t in range(3))      # [H, n, hd]
        s = torch.einsum("hic,hjc->hij", q, k) / math.sqrt(hd) + bb
        P = torch.softmax(s, dim=-1)
        o = torch.einsum("hij,hjc->hic", P, v)
        A = torch.einsum("hij,hjc->hic", P, v.abs())
        aj = torch.einsum("hic,hjc->hij", q.abs(), k.abs()) / math.sqrt(hd)
        a = aj.masked_fill(~ok[None], 0.0).amax(dim=-1, keepdim=True)                                          # [H, n, 1]
        ab = (aj + bb.abs()).masked_fill(~ok[None], 0.0).amax(dim=-1, keepdim=True)
        cnt = ok.sum(dim=1).double()
        idx = torch.arange(n)
        first = torch.where(ok, idx[None, :], torch.full((1, 1), n)).amin(dim=1)
        last = torch.where(ok, idx[None, :], torch.full((1, 1), -1)).amax(dim=1)
        trips = torch.ceil((last - first + 1).double() / 64)
        e = (hd + 4) * U32 * a + 3 * U32 * ab + 2 * U32
        E = 2 * e + ((cnt + trips + 10) * U32)[None, :, None]
        bound = E * A
        bound = bound + uT * (o.abs() + bound)
        if dtype == "f16":
            bound = bound + 2.0 ** -25
        O[b, :n] = o.permute(1, 0, 2).reshape(n, d)
        Bd[b, :n] = bound.permute(1, 0, 2).reshape(n, d)
    return O, Bd


@functools.lru_cache(maxsize=None)
def reference(kind, B, L, H, hd, dtype, lengths=None, planes=None):
    """reference_of(make_qkv(...), make_bias(kind, L, H, planes)); lengths: None or a tuple.  Computed once and shared: do not write to it"""
    return reference_of(make_qkv(B, L, H, hd, dtype), make_bias(kind, L, H, planes), H, dtype, lengths)


# ---- the walk ---------------------------------------------------------------------------------------------------------------------------
def emulate(qkv, bias, H, dtype, lengths=None, mutation=None):
    """The row's walk in torch float32 on the CPU -> [B, L, d] in T (rows behind a length: 0): tests/tf_attn_mask_bound.py's emulate with
    score = fl(fl(chain * scale) + bias[h][i][j]).  mutation: None, or one defect
         nobias        the bias ignored
         plane0        plane 0 used for every head
         lanerel       the bias indexed lane-relative: brow[j - first]
         transposed    bias[h][j][i]
         prescale      the bias added before the scale: fl(fl(chain + b) * scale)
         cornerstride  rows of the bias strided by the sequence's n instead of the bias's L (shows in a ragged batch only)
    A defect that reads an entry of a masked pair reads its -inf (weight 0; a row left without weight is NaN)."""
    dt = TDT[dtype]
    qkv = qkv.cpu()
    B, L, d3 = qkv.shape
    d = d3 // 3
    hd = d // H
    scale = (torch.tensor(1.0) / torch.sqrt(torch.tensor(float(hd)))).float()
    planes = bias.float().expand(H, L, L).contiguous()
    if mutation == "plane0":
        planes = planes[:1].expand(H, L, L).contiguous()
    if mutation == "transposed":
        planes = planes.transpose(1, 2).contiguous()
    flat = planes.reshape(H, L * L)
    allowed = allowed_of(bias)
    out = torch.zeros(B, L, d, dtype=dt)
    for b, n in enumerate(MB._lens(B, L, lengths)):
        ok = allowed[:n, :n]
        x = qkv[b, :n].float()
        q, k, v = (x[:, t * d:(t + 1) * d].reshape(n, H, hd).permute(1, 0, 2) for t in range(3))          # [H, n, hd]
        stride = n if mutation == "cornerstride" else L
        for i in range(n):
            cols = ok[i].nonzero().reshape(-1)
            if not len(cols):
                continue
            first, last = int(cols[0]), int(cols[-1])
            trips = (last - first) // 64 + 1
            width = trips * 64
            js = first + torch.arange(width)                                    # key of (trip, lane) = first + 64 trip + lane
            scored = torch.zeros(width, dtype=torch.bool)
            inside = js <= last
            scored[inside] = ok[i, js[inside]]
            jj = js.clamp(0, n - 1)
            s = torch.zeros(H, width)
            for c in range(hd):                                                 # one fmaf chain per key over c = 0 .. hd - 1 from 0.f
                s = MB._fma(q[:, i, c][:, None].expand(H, width), k[:, jj, c], s)
            bj = flat[:, i * stride + (jj - first if mutation == "lanerel" else jj)]          # [H, width]
            bj = torch.where(scored[None], bj, torch.zeros_like(bj))
            if mutation == "nobias":
                s = s * scale
            elif mutation == "prescale":
                s = (s + bj) * scale
            else:
                s = s * scale                                                   # rounds to float32 ...
                s = s + bj                                                      # ... and the add rounds again
            mx = s.masked_fill(~scored[None], NINF).amax(dim=1, keepdim=True)
            p = torch.exp(s - mx)
            pl = p.masked_fill(~scored[None], 0.0).view(H, trips, 64)
            lane = torch.zeros(H, 64)
            for t in range(trips):                                              # a lane's sum in trip order
                lane = lane + pl[:, t]
            tot = MB._wave_sum(lane)[:, 0]
            inv = (1.0 / tot)
            o = torch.zeros(H, hd)
            for w in scored.nonzero().reshape(-1).tolist():                     # the set bits in ascending key order
                o = MB._fma(p[:, w][:, None].expand(H, hd), v[:, int(jj[w])], o)
            res = o.double() * inv.double()[:, None] if dtype == "f16" else (o * inv[:, None])     # f16: the product rounds once, to T
            out[b, i] = res.reshape(-1).to(dt)
    return out
