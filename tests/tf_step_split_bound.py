"""Element-wise checker of the split-key step attention of the encoder's streams (tf_attn_split_row in flope_amd/csrc/tf_encoder.hip,
option "step_split"): the fp64 reference from the inputs as given, a bound for every output element, test data, and an
emulation of the row's walk that can be broken the way such a kernel breaks.  Helper of tests/test_tf_step_split_host.py (CPU: the
bound passes the emulation and fails its broken copies) and tests/test_gpu_tf_step_split.py (the device output).

One row per sequence: the query is the sequence's last token (row len - 1 of qkv [n, L, 3 d]), its keys are rows lo .. len - 1 with
lo = max(0, len - W) under a window W (0: none), Lv = len - lo of them.  Reference, per head and output dim c, in fp64 from the stored
q, k, v (T = float32, f16 or bf16):

    P_j = softmax_j(q . k_j / sqrt(hd)),   O_c = sum_j P_j v_jc,   A_c = sum_j P_j |v_jc|   (A >= |O|)

What the row does instead, and what each operation can cost (u = 2^-24; u_T = 2^-24 / 2^-11 / 2^-8; nb = ceil(Lv / 64) blocks, wave w
walks n_w = ceil((nb - w) / 4) of them, n = n_0 the most; LPS = hd sizeof(T) / 16 lanes per head slice, G = 64 / LPS lane groups):

  1. A probability's float32 value.  score = (fmaf chain over hd from 0.f) * fl(1 / sqrt(hd)); p = expf(score - m') with m' the wave's
     running maximum, earlier blocks carried on by alpha = expf(m - m') per block, the wave's state carried to the final maximum by
     expf(m_w - M) in the merge.  An error of a maximum is a common factor and cancels; what does not is a relative error e of a
     probability's weight.  With a_j = sum_c |q_c k_jc| / sqrt(hd) (>= |score_j|) and a = max_j a_j:
       - the chain: gamma(hd) sum |q k|; the scaling product and its rounded constant (sqrtf, one division): (hd + 4) u a
       - score - m' rounds once, |score - m'| <= 2 a: 2 u a; the alphas' arguments m - m' round once each and, the maximum being
         monotone, telescope to at most 2 a: 2 u a; m_w - M in the merge, once: 2 u a                   argument error <= (hd + 10) u a
       - an argument error dx changes expf by the factor e^dx: relative dx
       - expf is good to 1 ulp (2 u): for p, for each alpha, for the merge factor; o * alpha and fmaf(l, alpha, p) round once per
         block: 4 u per block; the merge's fmaf, the reciprocal (2 u) and, in float32, the final product: 10 u with slack
     so   e = (hd + 10) u a + (4 n + 10) u.
  2. Sums in float32.  Numerator, per element: a lane group adds the LPS keys it takes of each of the wave's n blocks in one fmaf
     chain, log2(G) butterfly adds, four merge fmafs; denominator: a lane adds one p per block, six shuffles, four merge fmafs.  Both
     relative to sum p |v| and sum p at most S u, S = n LPS + 10.
     First order in both:  |sum p~ v / sum p~ - O| <= (2 e + 2 S u) A_c  =: E A_c.
  3. The float32 probabilities are NOT rounded to T (they never leave registers and LDS as anything but float32): no u_T A term.
  4. The output is rounded to T once (f16: tf_mul_f16_bits): u_T |O~|, and for f16 at least half the subnormal spacing, 2^-25.

    bound_c = E A_c + u_T (|O_c| + E A_c) + [f16] 2^-25

Nothing in it is fitted to an output: the constants are the worst case of the operation counts above.  The emulation below replays
the walk (64-key blocks counted from lo, block b on wave b % 4, running maximum and rescale per block, the four partial states merged
in wave order with the waves without a block skipped by rule, one reciprocal, output rounding) over a model of the cache (a ring:
row (lo + k) % capacity) and of the token's own row, and must pass on every test shape; the tests print the headroom.
"""
import functools
import math

import torch

TDT = {"f32": torch.float32, "f32m": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
ESZ = {"f32": 4, "f32m": 4, "f16": 2, "bf16": 2}
U_T = {"f32": 2.0 ** -24, "f32m": 2.0 ** -24, "f16": 2.0 ** -11, "bf16": 2.0 ** -8}
U32 = 2.0 ** -24
WAVES, BLOCK = 4, 64

# (n, L, H, head_dim) of the issue: one key; a ragged single block at one lane per slice (f16); a full block; one key into wave 1;
# two blocks and a ragged third at 32 lanes per slice (f32); wave 0's second block, one key of it; a ragged fifth block; the capacity limit
CASES = [(2, 1, 2, 32), (2, 63, 2, 8), (1, 64, 2, 64), (3, 65, 2, 64), (1, 130, 1, 128), (2, 257, 2, 64), (1, 300, 4, 8), (1, 4096, 2, 64)]
RAGGED = ((3, 65, 2, 64), [65, 1, 64])               # the ragged lengths of one of them
# (n, L, H, head_dim, W, capacities): a ring that wraps inside the window
WINDOW_CASE = (2, 200, 2, 64, 70, (70, 96))

MUTATIONS = ["lastkey", "nowave", "noalpha", "nowrap", "owntwice"]


def step_split_ok(hd, dtype):
    """tf_step_split_ok of flope_amd/csrc/tf_encoder_stream.h: whole 16-byte vectors, a power-of-two count of them, at most 64"""
    ve = 16 // ESZ[dtype]
    lps = hd // ve
    return hd > 0 and hd % ve == 0 and lps <= 64 and lps & (lps - 1) == 0


def _lens(n, L, lengths):
    return [L] * n if lengths is None else [int(v) for v in lengths]


@functools.lru_cache(maxsize=None)
def make_qkv(n, L, H, hd, dtype, seed=7):
    """Standard-normal q, k, v rounded to T, [n, L, 3 H hd].  Where a wave walks a second block (L > 256), key 256 of every
    (sequence, head) is the last query scaled to a score of 6 (at L = 257 that is the query's own key):
    wave 0's running maximum then moves in its second block, and the other keys keep weights a float32 or 16-bit result shows."""
    g = torch.Generator().manual_seed(seed * 1000003 + n * 7919 + L * 31 + H * 5 + hd)
    x = torch.randn(n, L, 3, H, hd, generator=g)
    if L > 256:
        q = x[:, L - 1, 0]
        x[:, 256, 1] = q * (6.0 * math.sqrt(hd) / (q * q).sum(dim=-1, keepdim=True))
    return x.reshape(n, L, 3 * H * hd).to(TDT[dtype])


def _rows(qkv, H, b, ln, window):
    """q [H, hd], k, v [H, Lv, hd] of sequence b's last token and its visible keys"""
    d = qkv.shape[-1] // 3
    hd = d // H
    lo = max(0, ln - window) if window else 0
    q = qkv[b, ln - 1, :d].reshape(H, hd)
    k = qkv[b, lo:ln, d:2 * d].reshape(ln - lo, H, hd).permute(1, 0, 2)
    v = qkv[b, lo:ln, 2 * d:].reshape(ln - lo, H, hd).permute(1, 0, 2)
    return q, k, v, lo


def reference_of(qkv, H, dtype, lengths=None, window=0):
    """(O, bound) in fp64, both [n, d]"""
    qkv = qkv.cpu()
    n, L, d3 = qkv.shape
    hd = d3 // 3 // H
    lps = max(1, hd * ESZ[dtype] // 16)
    uT = U_T[dtype]
    O, Bd = [], []
    for b, ln in enumerate(_lens(n, L, lengths)):
        q, k, v, lo = (t.double() if torch.is_tensor(t) else t for t in _rows(qkv, H, b, ln, window))
        Lv = ln - lo
        P = torch.softmax(torch.einsum("hc,hjc->hj", q, k) / math.sqrt(hd), dim=-1)
        o = torch.einsum("hj,hjc->hc", P, v)
        A = torch.einsum("hj,hjc->hc", P, v.abs())
        a = (torch.einsum("hc,hjc->hj", q.abs(), k.abs()) / math.sqrt(hd)).amax(dim=-1, keepdim=True)      # [H, 1]
        nblk = -(-(-(-Lv // BLOCK)) // WAVES)                                    # wave 0's blocks: ceil(ceil(Lv / 64) / 4)
        e = (hd + 10) * U32 * a + (4 * nblk + 10) * U32
        E = 2 * e + 2 * (nblk * lps + 10) * U32
        bound = E * A
        bound = bound + uT * (o.abs() + bound)
        if dtype == "f16":
            bound = bound + 2.0 ** -25
        O.append(o.reshape(-1))
        Bd.append(bound.reshape(-1))
    return torch.stack(O), torch.stack(Bd)


@functools.lru_cache(maxsize=None)
def reference(n, L, H, hd, dtype, lengths=None, window=0, seed=7):
    """reference_of(make_qkv(...)); lengths: None or a tuple"""
    return reference_of(make_qkv(n, L, H, hd, dtype, seed), H, dtype, lengths, window)


def ratio(got, ref, bound):
    """max over elements of |got - ref| / bound, and where; a non-finite output counts as infinitely wrong"""
    g = got.detach().cpu().double()
    r = ((g - ref).abs() / bound)
    r = torch.where(torch.isfinite(g), r, torch.full_like(r, float("inf")))
    i = int(r.argmax())
    return float(r.reshape(-1)[i]), tuple(int(t) for t in torch.unravel_index(torch.tensor(i), r.shape))


def emulate(qkv, H, dtype, lengths=None, window=0, capacity=None, mutation=None):
    """The row's walk in torch float32 on the CPU -> [n, d] in T.  capacity: rows of the track's cache (None: the length; a window
    makes it a ring).  mutation: None, or one defect
         lastkey   lane 63 of a full block never scores its key
         nowave    wave 1's partial state left out of the merge
         noalpha   the running o and l not rescaled when the wave's maximum moves
         nowrap    a ring row taken as slo + k, without the wrap (what lies behind the track's rows reads as zeros)
         owntwice  the last cached key taken from the token's own row too"""
    dt = TDT[dtype]
    qkv = qkv.cpu()
    n, L, d3 = qkv.shape
    d = d3 // 3
    hd = d // H
    scale = torch.tensor(1.0, dtype=torch.float32) / torch.sqrt(torch.tensor(float(hd), dtype=torch.float32))
    out = []
    for b, ln in enumerate(_lens(n, L, lengths)):
        lo = max(0, ln - window) if window else 0
        Lv, nc = ln - lo, ln - 1 - lo
        cap = capacity if capacity is not None else max(ln, 1)
        # the cache as tf_cache_append leaves it: token i of rows 0 .. ln - 2 in row i % cap (a ring) or i; zeros behind the track
        cache = torch.zeros(2 * cap + Lv, 2 * d)
        for i in range(max(0, ln - 1 - cap) if window else 0, ln - 1):
            cache[i % cap if window else i] = qkv[b, i, d:].float()
        tok = qkv[b, ln - 1].float()
        slo = lo % cap if window else lo

        def key_row(kk):
            if kk >= nc or (mutation == "owntwice" and kk == nc - 1):
                return tok[d:]
            r = slo + kk
            if window and mutation != "nowrap" and r >= cap:
                r -= cap
            return cache[r]

        kvr = torch.stack([key_row(kk) for kk in range(Lv)])                       # [Lv, 2 d]
        k = kvr[:, :d].reshape(Lv, H, hd).permute(1, 0, 2)
        v = kvr[:, d:].reshape(Lv, H, hd).permute(1, 0, 2)
        q = tok[:d].reshape(H, hd)
        nb = -(-Lv // BLOCK)
        parts = []
        for w in range(WAVES):
            if w >= nb:                                                            # no block: no part in the merge, by rule
                continue
            m = torch.full((H,), float("-inf"))
            l = torch.zeros(H)
            o = torch.zeros(H, hd)
            for blk in range(w, nb, WAVES):
                k0, k1 = blk * BLOCK, min(Lv, blk * BLOCK + BLOCK)
                x = torch.einsum("hc,hjc->hj", q, k[:, k0:k1]) * scale
                if mutation == "lastkey" and k1 - k0 == BLOCK:
                    x[:, BLOCK - 1] = float("-inf")
                mn = torch.maximum(m, x.amax(dim=-1))
                alpha = torch.exp(m - mn)
                p = torch.exp(x - mn[:, None])
                if mutation == "noalpha":
                    alpha = torch.ones_like(alpha)
                l = l * alpha + p.sum(dim=-1)
                o = o * alpha[:, None] + torch.einsum("hj,hjc->hc", p, v[:, k0:k1])
                m = mn
            parts.append((w, m, l, o))
        if mutation == "nowave":
            parts = [p for p in parts if p[0] != 1]
        M = torch.stack([p[1] for p in parts]).amax(dim=0)
        ls = torch.zeros(H)
        os_ = torch.zeros(H, hd)
        for _, m, l, o in parts:
            f = torch.exp(m - M)
            ls = ls + f * l
            os_ = os_ + f[:, None] * o
        out.append((os_ * (1.0 / ls)[:, None]).reshape(-1).to(dt))
    return torch.stack(out)
