"""Sliding-window attention on the 16-bit MFMA kernels (option "window_mfma") on the test side: what
tests/test_tf_window16_host.py (CPU) and tests/test_gpu_tf_window16.py (device) compare against.  tests/tf_attn_bound.py is imported
as it is; nothing here is fitted to an output.

  reference_of       fp64 windowed attention from the 16-bit inputs as given, and tf_attn_bound's element-wise bound evaluated on the
                     windowed P and A = P |v|, with a_i the largest |score| bound over the keys query i sees.  The operation counts of
                     the bound (L keys summed, n = ceil(L / 32) steps) stay those of the full sequence: query i sums min(i + 1, W) <= L
                     keys in at most n steps, so every term is an upper bound of the query's own.  The guard of the step (msafe: 0
                     subtracted where the running maximum is still -inf) rounds nothing -- exp2(-inf) is exactly 0 -- so the bound has
                     no term for it
  wave_steps         first keys of the 32-key steps the wave of queries q0 .. q0 + 31 takes
  emulate            the walk of tf_attn_tiled / tf_attn_mfma under causal with a window in torch float32: a wave starts at the step of
                     its first query's first visible key, takes the steps up to its last query, masks key < L && key <= query &&
                     key + W > query per lane and subtracts msafe -- and six broken copies of it (MUTATIONS)
"""
import math

import torch

import tf_attn_bound as AB

MUTATIONS = ["noguard", "nowin", "from0", "wavewin", "offbyone", "latefirst"]

# ((B, L, H, head_dim), W): a window inside one step, one key past a step, two steps, one key, a window over several blocks of the
# streamed kernel, exactly one step, W >= L (plain causal), more than two blocks
CASES = [((2, 129, 2, 64), 8), ((2, 129, 2, 64), 33), ((1, 200, 1, 96), 64), ((1, 161, 2, 32), 1), ((1, 577, 2, 128), 100),
         ((3, 65, 2, 64), 32), ((1, 33, 3, 32), 40), ((1, 290, 1, 64), 130)]


def window_lo(i, W):
    """flope_tf_plan::tf_window_lo: the first visible key of query i"""
    return i - W + 1 if W > 0 and i >= W else 0


def _visible(L, W):
    i, j = torch.arange(L)[:, None], torch.arange(L)[None, :]
    vis = j <= i
    return vis & (j > i - W) if W > 0 else vis                       # [query, key]


def reference_of(qkv, H, dtype, W):
    """(O, bound) in fp64, both [B, L, H hd]: tf_attn_bound.reference_of's formula on the windowed P, A and a_i"""
    q, k, v = (t.double() for t in AB.split_heads(qkv.cpu(), H))
    hd, L = q.shape[-1], q.shape[-2]
    vis = _visible(L, W)
    P = torch.softmax((q @ k.transpose(-1, -2) / math.sqrt(hd)).masked_fill(~vis, float("-inf")), dim=-1)
    O = P @ v
    A = P @ v.abs()
    a = (AB.LOG2E / math.sqrt(hd)) * (q.abs() @ k.abs().transpose(-1, -2)).masked_fill(~vis, 0.0).amax(dim=-1, keepdim=True)
    n = (L + 31) // 32
    e = math.log(2.0) * (hd + 8) * AB.U32 * a + (4 * n + 8) * AB.U32
    E = 2 * e + 2 * (L + n + 10) * AB.U32
    uT = AB.U_T[dtype]
    bound = (uT + E) * A
    bound = bound + uT * (O.abs() + bound)
    if dtype == "f16":
        bound = bound + (L * 2.0 ** -25 * v.abs().amax(dim=(-1, -2), keepdim=True) + 2.0 ** -25)
    return AB.merge_heads(O), AB.merge_heads(bound)


def wave_steps(q0, L, W, mutation=None):
    """first keys of the 32-key steps the wave of queries q0 .. q0 + 31 takes: kb < L, kb <= q0 + 31 and kb + 31 >= the first visible
    key of query q0 (tf_window_step_taken), ascending"""
    first = window_lo(q0, W) & ~31
    if mutation == "from0":
        first = 0
    if mutation == "latefirst":
        first = window_lo(q0 + 31, W) & ~31
    return [kb for kb in range(first, (L + 31) // 32 * 32, 32) if kb <= q0 + 31]


def emulate(qkv, H, dtype, W, mutation=None):
    """tf_attn_bound.emulate's operations (running maximum, exp2, P rounded to T, float32 accumulators, one reciprocal, output
    rounding) per wave of 32 queries on the windowed walk.  mutation: None, or one defect
         noguard    the running maximum itself subtracted, -inf included (exp2(-inf - -inf))
         nowin      no lower mask inside the steps the wave takes
         from0      the walk from step 0, no lower mask: plain causal
         wavewin    the lower mask taken from the wave's first query for all 32
         offbyone   key >= query - W instead of key > query - W
         latefirst  the first step taken from the wave's LAST query"""
    dt = AB.TDT[dtype]
    q, k, v = (t.float().contiguous() for t in AB.split_heads(qkv.cpu(), H))
    B, _, L, hd = q.shape
    pad = (L + 31) // 32 * 32 - L
    k = torch.nn.functional.pad(k, (0, 0, 0, pad))
    v = torch.nn.functional.pad(v, (0, 0, 0, pad))
    scale = torch.tensor(AB.LOG2E, dtype=torch.float32) / torch.sqrt(torch.tensor(float(hd)))
    ninf = torch.tensor(float("-inf"))
    out = torch.empty(B, H, L, hd)
    for q0 in range(0, L, 32):
        nq = min(32, L - q0)
        qi = torch.arange(q0, q0 + nq)
        qw = q[:, :, q0:q0 + nq]
        m = torch.full((B, H, nq), float("-inf"))
        l = torch.zeros(B, H, nq)
        o = torch.zeros(B, H, nq, hd)
        for kb in wave_steps(q0, L, W, mutation):
            keys = torch.arange(kb, kb + 32)
            x = (qw @ k[:, :, kb:kb + 32].transpose(-1, -2)) * scale
            seen = (keys[None, :] <= qi[:, None]) & (keys < L)[None, :]
            if W > 0:
                if mutation in ("nowin", "from0"):
                    pass
                elif mutation == "wavewin":
                    seen = seen & (keys > q0 - W)[None, :]
                elif mutation == "offbyone":
                    seen = seen & (keys[None, :] >= qi[:, None] - W)
                else:
                    seen = seen & (keys[None, :] > qi[:, None] - W)
            x = torch.where(seen, x, ninf)
            mnew = torch.maximum(m, x.amax(dim=-1))
            msafe = mnew if mutation == "noguard" else torch.where(mnew == ninf, torch.zeros(()), mnew)
            alpha = torch.exp2(m - msafe)
            p = torch.exp2(x - msafe[..., None])
            l = l * alpha + p.sum(dim=-1)
            o = o * alpha[..., None] + p.to(dt).float() @ v[:, :, kb:kb + 32]
            m = mnew
        out[:, :, q0:q0 + nq] = o * (1.0 / l)[..., None]
    return AB.merge_heads(out.to(dt))
