"""Causal attention of the encoder (option "causal") on the test side: what tests/test_tf_causal_host.py (CPU) and
tests/test_gpu_tf_causal.py (device) compare against.  tests/tf_attn_bound.py is imported as it is; nothing here is fitted to an output.

  causal_forward     the fp64 oracle forward (oracle/tf_encoder_ref.py) restated with query i attending to keys j <= i, pinned by
                     tests/golden/tf_causal_fixture.npz (the reference module under generate_square_subsequent_mask)
  reference_of       fp64 causal attention from the 16-bit inputs as given, and tf_attn_bound's element-wise bound evaluated on the
                     causal P and A = P |v|, with a_i the largest |score| bound over the keys query i sees.  The operation counts
                     of the bound (L keys summed, n = ceil(L / 32) steps) stay those of the full sequence: query i sums i + 1 <= L
                     keys in at most n steps, so every term is an upper bound of the query's own
  attention_fp64     fp64 causal attention of float inputs (the float32 kernels' reference)
  emulate            the 32-key-step walk of tf_attn_tiled / tf_attn_mfma under the option in torch float32: a wave of 32 queries
                     starts at step 0, takes the steps kb <= q0 + 31, masks key < L && key <= query per lane -- and four broken
                     copies of it (MUTATIONS)
"""
import math

import numpy as np
import torch

import tf_attn_bound as AB
from oracle import tf_encoder_ref as T

MUTATIONS = ["strict", "nodiag", "wavemask", "nomask"]


# ---- the whole encoder, fp64 ------------------------------------------------------------------------------------------------------
def causal_attention_block(x, w_in, b_in, w_out, b_out, heads):
    """oracle.tf_encoder_ref.attention with scores above the diagonal at -inf"""
    B, L, d = x.shape
    dh = d // heads
    qkv = x @ w_in.T + b_in
    q, k, v = (qkv[..., i * d:(i + 1) * d].reshape(B, L, heads, dh).transpose(0, 2, 1, 3) for i in range(3))
    s = q @ k.transpose(0, 1, 3, 2) / np.sqrt(dh)
    s = np.where(np.arange(L)[None, :] <= np.arange(L)[:, None], s, -np.inf)
    s = s - s.max(-1, keepdims=True)
    p = np.exp(s)
    p = p / p.sum(-1, keepdims=True)
    o = (p @ v).transpose(0, 2, 1, 3).reshape(B, L, d)
    return o @ w_out.T + b_out


def causal_forward(sd, x, num_heads, dtype=np.float64):
    """oracle.tf_encoder_ref.forward with causal attention: sd {name: array}, x [B, L, input_dim] -> [B, L, out_dim]"""
    g = lambda k: np.asarray(sd[k], dtype=dtype)
    h = np.asarray(x, dtype=dtype) @ g("embedding.weight").T + g("embedding.bias")
    for i in range(T.num_layers_of(sd)):
        p = f"transformer_encoder.layers.{i}."
        a = causal_attention_block(h, g(p + "self_attn.in_proj_weight"), g(p + "self_attn.in_proj_bias"),
                                   g(p + "self_attn.out_proj.weight"), g(p + "self_attn.out_proj.bias"), num_heads)
        h = T.layer_norm(h + a, g(p + "norm1.weight"), g(p + "norm1.bias"))
        f = np.maximum(h @ g(p + "linear1.weight").T + g(p + "linear1.bias"), 0) @ g(p + "linear2.weight").T + g(p + "linear2.bias")
        h = T.layer_norm(h + f, g(p + "norm2.weight"), g(p + "norm2.bias"))
    return h @ g("out_layer.weight").T + g("out_layer.bias")


# ---- stand-alone attention, fp64 --------------------------------------------------------------------------------------------------
def _visible(L):
    return torch.arange(L)[None, :] <= torch.arange(L)[:, None]          # [query, key]


def attention_fp64(qkv, H):
    """qkv [B, L, 3 d] of any float dtype -> fp64 causal attention [B, L, d]"""
    q, k, v = (t.double() for t in AB.split_heads(qkv.cpu(), H))
    hd, L = q.shape[-1], q.shape[-2]
    s = (q @ k.transpose(-1, -2) / math.sqrt(hd)).masked_fill(~_visible(L), float("-inf"))
    return AB.merge_heads(torch.softmax(s, dim=-1) @ v)


def reference_of(qkv, H, dtype):
    """(O, bound) in fp64, both [B, L, H hd]: tf_attn_bound.reference_of's formula on the causal P, A and a_i"""
    q, k, v = (t.double() for t in AB.split_heads(qkv.cpu(), H))
    hd, L = q.shape[-1], q.shape[-2]
    vis = _visible(L)
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


# ---- the kernels' walk, emulated --------------------------------------------------------------------------------------------------
def wave_steps(q0, L, mutation=None):
    """first keys of the 32-key steps the wave of queries q0 .. q0 + 31 takes: kb < L and kb <= q0 + 31, from step 0 on"""
    steps = [kb for kb in range(0, (L + 31) // 32 * 32, 32) if kb <= q0 + 31]
    if mutation == "nodiag":
        steps = [kb for kb in steps if kb != q0]
    return steps


def emulate(qkv, H, dtype, mutation=None):
    """tf_attn_bound.emulate's operations (running maximum, exp2, P rounded to T, float32 accumulators, one reciprocal, output
    rounding) per wave of 32 queries on the causal walk.  mutation: None, or one defect
         strict    key < query instead of key <= query (query 0 sees nothing)
         nodiag    the step that holds the wave's own queries skipped
         wavemask  the mask taken from the wave's first query for all 32
         nomask    no causal mask inside the steps the wave takes (keys past L still masked)"""
    dt = AB.TDT[dtype]
    q, k, v = (t.float().contiguous() for t in AB.split_heads(qkv.cpu(), H))
    B, _, L, hd = q.shape
    pad = (L + 31) // 32 * 32 - L
    k = torch.nn.functional.pad(k, (0, 0, 0, pad))
    v = torch.nn.functional.pad(v, (0, 0, 0, pad))
    scale = torch.tensor(AB.LOG2E, dtype=torch.float32) / torch.sqrt(torch.tensor(float(hd)))
    out = torch.empty(B, H, L, hd)
    for q0 in range(0, L, 32):
        nq = min(32, L - q0)
        qi = torch.arange(q0, q0 + nq)
        qw = q[:, :, q0:q0 + nq]
        m = torch.full((B, H, nq), float("-inf"))
        l = torch.zeros(B, H, nq)
        o = torch.zeros(B, H, nq, hd)
        for kb in wave_steps(q0, L, mutation):
            keys = torch.arange(kb, kb + 32)
            x = (qw @ k[:, :, kb:kb + 32].transpose(-1, -2)) * scale
            if mutation == "strict":
                seen = keys[None, :] < qi[:, None]
            elif mutation == "wavemask":
                seen = (keys <= q0)[None, :].expand(nq, -1)
            elif mutation == "nomask":
                seen = torch.ones(nq, 32, dtype=torch.bool)
            else:
                seen = keys[None, :] <= qi[:, None]
            seen = seen & (keys < L)[None, :]
            x = torch.where(seen, x, torch.tensor(float("-inf")))
            mnew = torch.maximum(m, x.amax(dim=-1))
            alpha = torch.exp2(m - mnew)
            p = torch.exp2(x - mnew[..., None])
            l = l * alpha + p.sum(dim=-1)
            o = o * alpha[..., None] + p.to(dt).float() @ v[:, :, kb:kb + 32]
            m = mnew
        out[:, :, q0:q0 + nq] = o * (1.0 / l)[..., None]
    return AB.merge_heads(out.to(dt))
