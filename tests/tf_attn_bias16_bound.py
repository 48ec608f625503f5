"""A compiled bias on the 16-bit MFMA attention (option "bias_mfma", the BIASED instantiation of tf_attn_tiled_masked in
flope_amd/csrc/tf_encoder.hip) on the test side: what tests/test_tf_bias16_bound.py (CPU) and tests/test_gpu_tf_bias16.py
(device) compare against.  tests/tf_attn_bound.py, tests/tf_attn_mask_bound.py, tests/tf_attn_mask16_bound.py and
tests/tf_attn_bias_bound.py are imported as they are; nothing here is fitted to an output.

The kernel's scores live in the log2 domain.  With x_j = fl(s_j * scale_log2e) the unbiased step's score (s_j the MFMA's float32 sum,
scale_log2e = fl(log2(e) / sqrt(hd))) the biased score is ONE fma, rounded once:

    y_j = fl(b_ij * LOG2E_f32 + x_j),      exact value  log2(e) (q . k_j / sqrt(hd) + b_ij)

  reference_of   fp64 biased attention from the 16-bit inputs and the float32 bias as given, and tests/tf_attn_mask16_bound.py's
                 element-wise bound with the fma accounted for.  In log2 units, over the keys query i is allowed, with
                 a_j = log2(e) / sqrt(hd) sum_c |q_c k_jc|, a = max_j a_j (that bound's a_i), bl = max_j log2(e) |b_ij| and
                 ab = max_j (a_j + log2(e) |b_ij|)  (a <= ab, bl <= ab):
                   - the chain, the scaling product and its rounded constant, as before:        (hd + 4) u a
                   - NEW the fma rounds once, its exact value at most ab in magnitude:           u ab
                   - NEW its float32 constant LOG2E_f32 is log2(e) (1 + d), |d| <= u:            u log2(e) |b_ij| <= u bl
                   - y - m rounds once with |y - m| <= 2 ab, and the alphas' arguments telescope to at most 2 ab: every later use of
                     a has become ab:                                                            4 u ab   (was 4 u a)
                 so the argument error is ((hd + 4) a + 5 ab + bl) u, and
                     e_i = ln(2) ((hd + 4) a + 5 ab + bl) u + (4 ns + 8) u
                 with everything behind it -- the exp2 and per-step roundings (4 ns + 8) u, the sums 2 (n + ns + 10) u, P rounded to T,
                 the output rounding, the f16 flush term -- unchanged.  At a zero bias ab = a and bl = 0: e_i = ln(2) (hd + 9) u a + ...,
                 one u a above tests/tf_attn_mask16_bound.py's (hd + 8): never smaller (the fma is still made).
  emulate        tests/tf_attn_mask16_bound.py's walk of tf_attn_tiled_masked in torch float32 plus the fma (product exact in fp64, the
                 sum rounded to fp64 and then to float32, as tests/tf_attn_mask_bound.py's _fma), the entry read from row
                 min(query, n - 1) of plane h with row stride L at the key's own column -- and six broken copies of it (MUTATIONS).
                 A zero bias gives that walk's bits: fma(0, c, x) = x up to the sign of a zero, which no later operation keeps.
                 The row clamp for a query at or past n is not among the defects: such a query is not stored by the kernel and not
                 walked here, so leaving the clamp out changes no output (on the device it would form an address outside the planes,
                 which is tests/test_tf_bias16_host.py's business, not a bound's).
"""
import math

import numpy as np
import torch

import tf_attn_bias_bound as BB
import tf_attn_bound as AB
import tf_attn_mask16_bound as M16
import tf_attn_mask_bound as MB

NINF = float("-inf")
MUTATIONS = ["nobias", "plane0", "nolog2e", "bitmap", "transposed", "cornerstride"]
NONE, SOME, ALL = M16.NONE, M16.SOME, M16.ALL
QB, KB = M16.QB, M16.KB
LENGTHS = M16.LENGTHS                       # 1, 33, 65, 129, 257
HEAD_DIMS = M16.HEAD_DIMS                   # 32, 64, 96, 128
KINDS = ("holes", "alibi", "edge", "gap")   # tests/tf_attn_bias_bound.py's three, and 2 randn per head over tf_attn_mask16_bound.gap_mask (L = 257 only)
LOG2E_F32 = torch.tensor(1.4426950408889634, dtype=torch.float32)

ratio = MB.ratio
allowed_of = BB.allowed_of


def make_bias(kind, L, H, planes=None):
    """float32 [P, L, L], P = H (default) or 1; -inf = masked"""
    if kind != "gap":
        return BB.make_bias(kind, L, H, planes)
    P = H if planes is None else planes
    g = torch.Generator().manual_seed(1709 + P)
    return BB.over(M16.gap_mask(L), 2 * torch.randn(P, L, L, generator=g))


def zero_over(allowed, planes=1):
    return BB.over(allowed, torch.zeros(planes, *allowed.shape))


def reference_of(qkv, bias, H, dtype, lengths=None):
    """(O, bound) in fp64, both [B, L, d]: tf_attn_mask16_bound.reference_of's formula with the fma's terms (module docstring); rows
    behind a length are 0 with bound 0"""
    qkv = qkv.cpu().double()
    B, L, d3 = qkv.shape
    d = d3 // 3
    hd = d // H
    uT = AB.U_T[dtype]
    bias = bias.double().expand(H, L, L)
    O = torch.zeros(B, L, d, dtype=torch.float64)
    Bd = torch.zeros(B, L, d, dtype=torch.float64)
    for b, n in enumerate(MB._lens(B, L, lengths)):
        bb = bias[:, :n, :n]
        ok = bb[0] > NINF
        q, k, v = (qkv[b, :n, t * d:(t + 1) * d].reshape(n, H, hd).permute(1, 0, 2) for t in range(3))      # [H, n, hd]
        P = torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(hd) + bb, dim=-1)
        o = P @ v
        A = P @ v.abs()
        aj = (AB.LOG2E / math.sqrt(hd)) * (q.abs() @ k.abs().transpose(-1, -2))
        bj = (AB.LOG2E * bb.abs()).masked_fill(~ok[None], 0.0)
        a = aj.masked_fill(~ok[None], 0.0).amax(dim=-1, keepdim=True)
        bl = bj.amax(dim=-1, keepdim=True)
        ab = (aj + bj).masked_fill(~ok[None], 0.0).amax(dim=-1, keepdim=True)
        ns = (n + 31) // 32
        e = math.log(2.0) * ((hd + 4) * a + 5 * ab + bl) * AB.U32 + (4 * ns + 8) * AB.U32
        E = 2 * e + 2 * (n + ns + 10) * AB.U32
        bound = (uT + E) * A
        bound = bound + uT * (o.abs() + bound)
        if dtype == "f16":
            bound = bound + (n * 2.0 ** -25 * v.abs().amax(dim=(-1, -2), keepdim=True) + 2.0 ** -25)
        O[b, :n] = o.permute(1, 0, 2).reshape(n, d)
        Bd[b, :n] = bound.permute(1, 0, 2).reshape(n, d)
    return O, Bd


def _fma(a, b, c):
    return MB._fma(a, b, c)


def emulate(qkv, bias, H, dtype, lengths=None, mutation=None, rows="wave"):
    """tf_attn_mask16_bound.emulate's walk (no defect of its own) with the biased score -> [B, L, d] in T (rows behind a length: 0).
    mutation: None, or one defect
         nobias        the bias ignored (the MASKED step)
         plane0        plane 0 for every head
         nolog2e       the bias added without the log2(e) factor: fma(b, 1, x)
         bitmap        the entry of column kb + 8 g + 4 u + q for the key kb + 16 u + 4 g + q (the lane's sixteen values taken as
                       consecutive columns)
         transposed    bias[h][key][query]
         cornerstride  rows of the bias strided by the sequence's n instead of the bias's L (shows in a ragged batch only)
    A defect that reads the entry of a masked pair reads its -inf (weight 0)."""
    dt = AB.TDT[dtype]
    qkv = qkv.cpu()
    B, L, d3 = qkv.shape
    d = d3 // 3
    hd = d // H
    allowed = allowed_of(bias)
    tm = M16.tile_map(allowed)
    words = M16._words(allowed)
    planes = bias.float().expand(H, L, L).contiguous()
    if mutation == "plane0":
        planes = planes[:1].expand(H, L, L).contiguous()
    if mutation == "transposed":
        planes = planes.transpose(1, 2).contiguous()
    flat = planes.reshape(H, L * L)
    scale = torch.tensor(AB.LOG2E, dtype=torch.float32) / torch.sqrt(torch.tensor(float(hd)))
    factor = torch.ones((), dtype=torch.float32) if mutation == "nolog2e" else LOG2E_F32
    ninf = torch.tensor(NINF)
    off = np.arange(32)
    if mutation == "bitmap":
        u, g, q = off // 16, (off % 16) // 4, off % 4
        off = 8 * g + 4 * u + q
    off = torch.from_numpy(off)
    out = torch.zeros(B, L, d, dtype=dt)
    for b, n in enumerate(MB._lens(B, L, lengths)):
        stride = n if mutation == "cornerstride" else L
        x = qkv[b, :n].float()
        q, k, v = (x[:, t * d:(t + 1) * d].reshape(n, H, hd).permute(1, 0, 2).contiguous()[None] for t in range(3))      # [1, H, n, hd]
        res = torch.empty(1, H, n, hd)
        for qb in range((n + QB - 1) // QB):
            entries = [e for e in tm[qb] if e[0] * KB < n]                   # the corner's prefix
            stages = [None, None]
            state = {}
            for w in range(4):
                q0 = qb * QB + 32 * w
                if q0 < n:
                    nq = min(32, n - q0)
                    state[w] = [torch.full((1, H, nq), NINF), torch.zeros(1, H, nq), torch.zeros(1, H, nq, hd)]
            for trip, (kblock, colany, cls) in enumerate(entries):
                krows = torch.arange(kblock * KB, kblock * KB + KB)
                keep = (krows < n) & torch.from_numpy(colany)
                src = krows.clamp(max=n - 1)
                z = torch.zeros(())
                stages[trip & 1] = (torch.where(keep[:, None], k[:, :, src], z), torch.where(keep[:, None], v[:, :, src], z))
                st = stages[trip & 1]
                for w, (m, l, o) in state.items():
                    q0 = qb * QB + 32 * w
                    nq = m.shape[-1]
                    for s in range(2):
                        kb = kblock * KB + 32 * s
                        c = cls[w][s]
                        if kb >= n or c == NONE:
                            continue
                        keys = torch.arange(kb, kb + 32)
                        seen = (keys < n)[None, :].expand(nq, 32)
                        if c == SOME:
                            seen = seen & M16._lane_bits(words[q0:q0 + nq, kb // 32], None)
                        kt = st[0][:, :, 32 * s:32 * s + 32].transpose(-1, -2)
                        sc = ((q @ kt)[:, :, q0:q0 + nq] if rows == "sequence" else q[:, :, q0:q0 + nq] @ kt) * scale
                        if mutation != "nobias":
                            col = (kb + off).clamp(max=L - 1)
                            idx = (torch.arange(q0, q0 + nq)[:, None] * stride + col[None, :]).clamp(max=L * L - 1)      # [nq, 32]
                            bv = flat[:, idx][None]                                                                    # [1, H, nq, 32]
                            bv = torch.where(seen, bv, torch.zeros(()))                # an unseen pair's entry (-inf) is discarded by the select
                            sc = _fma(bv, factor.expand_as(bv), sc)
                        sc = torch.where(seen, sc, ninf)
                        mnew = torch.maximum(m, sc.amax(dim=-1))
                        msafe = torch.where(mnew == ninf, torch.zeros(()), mnew)
                        alpha = torch.exp2(m - msafe)
                        p = torch.exp2(sc - msafe[..., None])
                        l = l * alpha + p.sum(dim=-1)
                        pt = p.to(dt).float()
                        if rows == "sequence":
                            pf = torch.zeros(1, H, n, 32)
                            pf[:, :, q0:q0 + nq] = pt
                            o = o * alpha[..., None] + (pf @ st[1][:, :, 32 * s:32 * s + 32])[:, :, q0:q0 + nq]
                        else:
                            o = o * alpha[..., None] + pt @ st[1][:, :, 32 * s:32 * s + 32]
                        m = mnew
                    state[w] = [m, l, o]
            for w, (m, l, o) in state.items():
                q0 = qb * QB + 32 * w
                res[:, :, q0:q0 + m.shape[-1]] = o * (1.0 / l)[..., None]
        out[b, :n] = AB.merge_heads(res.to(dt))[0]
    return out


RAGGED = (257, 130, 66, 1, 129)             # at L = 257: every query-block count, a length of one key, a corner that ends inside a step


def shapes():
    """(name, kind, L, planes, lengths): what tests/test_gpu_tf_bias16.py holds to the bound at every head_dim and 16-bit dtype, and
    tests/test_tf_bias16_bound.py the emulation.  planes None: one per head; "gap" exists at L = 257 only"""
    for L in LENGTHS:
        for kind in ("holes", "alibi", "edge"):
            yield f"{kind}{L}", kind, L, None, None
    yield "gap257", "gap", 257, None, None
    yield "holes129one", "holes", 129, 1, None
    yield "alibi257ragged", "alibi", 257, None, RAGGED
    yield "holes257ragged", "holes", 257, None, RAGGED
