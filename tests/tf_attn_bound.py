"""Element-wise checker of the 16-bit MFMA attention kernels of the encoder (tf_attn_tiled, tf_attn_mfma in
flope_amd/csrc/tf_encoder.hip): the fp64 reference computed from the 16-bit inputs as given, a bound for every output element,
test data, and an emulation of the kernel's steps that can be broken the way kernels break.  Helper of tests/test_tf_attn_bound.py
(CPU: the bound passes the emulation and fails its broken copies) and tests/test_gpu_tf_attn_tiled.py (the device output).

Reference, per (batch, head), query i, output dim c, in fp64 from the stored q, k, v (T = f16 or bf16):

    P_ij = softmax_j(q_i . k_j / sqrt(hd)),   O_ic = sum_j P_ij v_jc,   A_ic = sum_j P_ij |v_jc|   (A >= |O|)

What the kernel does instead, and what each step can cost (u_T = 2^-11 f16, 2^-8 bf16; u = 2^-24; n = ceil(L / 32) steps):

  1. A probability's float32 value.  The kernel forms p~_ij = exp2(x_ij - m) with x = (q.k in float32) * fl(log2(e) / sqrt(hd)), m the
     running maximum, and carries earlier steps to the final maximum by one multiplication with alpha = exp2(m_old - m_new) per
     step.  Any error of the maximum itself is a common factor of numerator and denominator and cancels.  What does not cancel is a
     relative error e_ij of p~_ij.  With a_ij = log2(e) / sqrt(hd) * sum_c |q_ic k_jc| (>= |x_ij|) and a_i = max_j a_ij:
       - q.k on the MFMA: hd exact products summed in float32 in some order, gamma(hd) sum |q k|; the scaling product and the
         rounded constant, one u each:                                        argument error <= (hd + 4) u a_i   (2 u of slack)
       - x - m rounds once, |x - m| <= 2 a_i; the alphas' arguments m_old - m_new round once each and, the maximum being monotone,
         telescope to at most 2 a_i in total:                                 argument error <= 4 u a_i
       - an argument error dx changes exp2 by the factor 2^dx: relative ln(2) dx
       - v_exp_f32 is good to 1 ulp (2 u) for p and for each alpha; o * alpha and l * alpha + p round once per step: 4 u per step,
         8 u for p's own exp2, the reciprocal of l and the final product
     so   e_i = ln(2) (hd + 8) u a_i + (4 n + 8) u.
  2. Sums in float32.  The denominator adds L positive terms (per lane 8 per step, n steps, two shuffles), the numerator L products
     per element in the MFMA's order: relative to sum p and to sum p |v| at most (L + n + 10) u each.
     First order in both:  |sum p~ v / sum p~ - O| <= (2 e_i + 2 (L + n + 10) u) A_ic  =: E_i A_ic.
  3. P is rounded to T for the second MFMA while the denominator sums the unrounded values:          u_T sum_j P_ij |v_jc| = u_T A_ic.
     f16 only: probabilities below 2^-14 (relative to the running maximum of their step, hence <= their final weight times l,
     l >= 1) are subnormal and round with absolute error 2^-25 each:                                 L 2^-25 max |v|.
  4. The output is rounded to T: u_T |O~|, and for f16 at least half the subnormal spacing, 2^-25.

    bound_ic = (u_T + E_i) A_ic + u_T (|O_ic| + (u_T + E_i) A_ic) + [f16] (L 2^-25 max_jc |v_jc| + 2^-25)

Nothing in it is fitted to an output: the float32 constants are the worst case of the operation counts above.  The emulation
below replays those operations (32-key steps, running maximum, exp2, P rounded to T, float32 accumulators, one reciprocal, output
rounding) and must pass on every test shape; the headroom is printed by the tests.
"""
import functools
import math

import torch

TDT = {"f16": torch.float16, "bf16": torch.bfloat16}
U_T = {"f16": 2.0 ** -11, "bf16": 2.0 ** -8}
U32 = 2.0 ** -24
LOG2E = 1.4426950408889634

# (B, L, H, head_dim): single step, ragged step, second query block, block boundary, each head width
BASE_CASES = [(2, 1, 2, 32), (1, 33, 3, 32), (2, 129, 2, 64), (1, 200, 1, 96), (1, 577, 2, 128), (3, 65, 2, 64)]

MUTATIONS = ["nomask", "skip", "twice", "ring", "noalpha", "head0v", "dims64", "scale64"]


def cases(kb, ring):
    """The test shapes for a kernel that streams `kb` keys per block through `ring` LDS stages: the base cases and two lengths one
    and 33 keys past a full ring, where the first stage is written a second time."""
    return BASE_CASES + [(1, kb * ring + 1, 2, 128), (1, kb * ring + 33, 2, 32)]


def split_heads(qkv, H):
    """qkv [B, L, 3 d] -> q, k, v [B, H, L, hd] (views)"""
    B, L, d3 = qkv.shape
    d = d3 // 3
    q, k, v = (qkv[:, :, i * d:(i + 1) * d].reshape(B, L, H, d // H).permute(0, 2, 1, 3) for i in range(3))
    return q, k, v


def merge_heads(o):
    B, H, L, hd = o.shape
    return o.permute(0, 2, 1, 3).reshape(B, L, H * hd)


@functools.lru_cache(maxsize=None)
def make_qkv(B, L, H, hd, dtype, seed=5):
    """Standard-normal q, k, v rounded to T, [B, L, 3 H hd].  Per (batch, head) one key of the first 32-key step and one of the last
    are scaled by 4: a query is then likely to find its best key in one of the two, which one depends on the sign of two dot
    products -- so the running maximum of some queries is final after the first step and that of others jumps in the last one."""
    g = torch.Generator().manual_seed(seed * 1000003 + B * 7919 + L * 31 + H * 5 + hd)
    x = torch.randn(B, L, 3, H, hd, generator=g)
    if L > 32:
        first, last = 3 % L, (L - 1) // 32 * 32 + ((L - 1) % 32) // 2
        x[:, first, 1] *= 4.0
        x[:, last, 1] *= 4.0
    return x.reshape(B, L, 3 * H * hd).to(TDT[dtype])


@functools.lru_cache(maxsize=None)
def reference(B, L, H, hd, dtype, seed=5):
    """(O, bound) in fp64, both [B, L, H hd], for make_qkv(B, L, H, hd, dtype, seed)."""
    return reference_of(make_qkv(B, L, H, hd, dtype, seed), H, dtype)


def reference_of(qkv, H, dtype):
    q, k, v = (t.double() for t in split_heads(qkv.cpu(), H))
    hd, L = q.shape[-1], q.shape[-2]
    P = torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(hd), dim=-1)
    O = P @ v
    A = P @ v.abs()
    a = (LOG2E / math.sqrt(hd)) * (q.abs() @ k.abs().transpose(-1, -2)).amax(dim=-1, keepdim=True)       # [B, H, L, 1]
    n = (L + 31) // 32
    e = math.log(2.0) * (hd + 8) * U32 * a + (4 * n + 8) * U32
    E = 2 * e + 2 * (L + n + 10) * U32
    uT = U_T[dtype]
    bound = (uT + E) * A
    bound = bound + uT * (O.abs() + bound)
    if dtype == "f16":
        bound = bound + (L * 2.0 ** -25 * v.abs().amax(dim=(-1, -2), keepdim=True) + 2.0 ** -25)
    return merge_heads(O), merge_heads(bound)


def best_key_steps(qkv, H):
    """32-key step that holds each query's best key, [B, H, L]"""
    q, k, _ = (t.double() for t in split_heads(qkv.cpu(), H))
    return (q @ k.transpose(-1, -2)).argmax(dim=-1) // 32


def ratio(got, ref, bound):
    """max over elements of |got - ref| / bound, and where; a non-finite output counts as infinitely wrong"""
    g = got.detach().cpu().double()
    r = ((g - ref).abs() / bound)
    r = torch.where(torch.isfinite(g), r, torch.full_like(r, float("inf")))
    i = int(r.argmax())
    return float(r.reshape(-1)[i]), tuple(int(t) for t in torch.unravel_index(torch.tensor(i), r.shape))


def emulate(qkv, H, dtype, mutation=None, kb=64, ring=2):
    """The kernel's steps in torch float32 on the CPU.  mutation: None, or one defect
         nomask   padded keys of a ragged last step not set to -inf
         skip     the second 32-key step never processed          twice    ... processed twice
         ring     the third block's V (keys 2 kb ...) taken from the block that held its ring stage before (block 0)
         noalpha  accumulators not rescaled when the maximum moves
         head0v   heads >= 1 read head 0's V
         dims64   output dims >= 64 never written (left 0)
         scale64  scores scaled by 1 / sqrt(64) whatever head_dim is"""
    dt = TDT[dtype]
    q, k, v = (t.float().contiguous() for t in split_heads(qkv.cpu(), H))
    B, _, L, hd = q.shape
    n = (L + 31) // 32
    pad = n * 32 - L
    k = torch.nn.functional.pad(k, (0, 0, 0, pad))
    v = torch.nn.functional.pad(v, (0, 0, 0, pad))
    if mutation == "head0v":
        v = v[:, 0:1].expand(-1, H, -1, -1)
    scale = torch.tensor(LOG2E, dtype=torch.float32) / torch.sqrt(torch.tensor(64.0 if mutation == "scale64" else float(hd)))
    steps = list(range(n))
    if mutation == "skip":
        del steps[1]
    if mutation == "twice":
        steps.insert(1, 1)
    m = torch.full((B, H, L), float("-inf"))
    l = torch.zeros(B, H, L)
    o = torch.zeros(B, H, L, hd)
    spb = kb // 32
    for s in steps:
        ks = k[:, :, s * 32:(s + 1) * 32]
        sv = s - ring * spb if (mutation == "ring" and s // spb == ring) else s
        vs = v[:, :, sv * 32:(sv + 1) * 32]
        x = (q @ ks.transpose(-1, -2)) * scale
        if mutation != "nomask":
            valid = torch.arange(s * 32, (s + 1) * 32) < L
            x = torch.where(valid, x, torch.tensor(float("-inf")))
        mnew = torch.maximum(m, x.amax(dim=-1))
        alpha = torch.exp2(m - mnew)
        p = torch.exp2(x - mnew[..., None])
        l = l * alpha + p.sum(dim=-1)
        if mutation != "noalpha":
            o = o * alpha[..., None]
        o = o + p.to(dt).float() @ vs
        m = mnew
    out = o * (1.0 / l)[..., None]
    if mutation == "dims64":
        out[..., 64:] = 0.0
    return merge_heads(out.to(dt))
