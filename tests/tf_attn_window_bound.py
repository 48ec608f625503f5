"""Sliding-window causal attention of the encoder (option "window") on the test side: what tests/test_tf_window_host.py
(CPU) and tests/test_gpu_tf_window.py (device) compare against.  tests/tf_attn_causal_bound.py is imported as it is; nothing here is
fitted to an output.

  window_forward     the fp64 causal restatement (tf_attn_causal_bound.causal_forward) with query i attending to keys i - W < j <= i
                     of its own sequence, pinned by tests/golden/tf_window_fixture.npz (the reference module under the banded mask);
                     W = 0 or W >= L is causal_forward itself.  With lengths every sequence is encoded alone at its own length and
                     the rows behind it are out_layer.bias (DESIGN.md 19's contract)
  band_mask          torch's spelling of the window: the [L, L] mask, float (-inf / 0) or bool (True = masked)
"""
import numpy as np
import torch

import tf_attn_causal_bound as CB
from oracle import tf_encoder_ref as T


def visible(L, W):
    """[query, key] bool: i - W < j <= i (W = 0: j <= i)"""
    i, j = np.arange(L)[:, None], np.arange(L)[None, :]
    return (j <= i) & ((j > i - W) if W > 0 else True)


def band_mask(L, W, dtype=torch.float32):
    vis = torch.from_numpy(visible(L, W))
    if dtype == torch.bool:
        return ~vis
    return torch.zeros(L, L, dtype=dtype).masked_fill(~vis, float("-inf"))


def window_attention_block(x, w_in, b_in, w_out, b_out, heads, W):
    """tf_attn_causal_bound.causal_attention_block with the scores outside the window at -inf as well"""
    B, L, d = x.shape
    dh = d // heads
    qkv = x @ w_in.T + b_in
    q, k, v = (qkv[..., i * d:(i + 1) * d].reshape(B, L, heads, dh).transpose(0, 2, 1, 3) for i in range(3))
    s = q @ k.transpose(0, 1, 3, 2) / np.sqrt(dh)
    s = np.where(visible(L, W), s, -np.inf)
    s = s - s.max(-1, keepdims=True)
    p = np.exp(s)
    p = p / p.sum(-1, keepdims=True)
    o = (p @ v).transpose(0, 2, 1, 3).reshape(B, L, d)
    return o @ w_out.T + b_out


def _forward(sd, x, W, num_heads, dtype):
    g = lambda k: np.asarray(sd[k], dtype=dtype)
    h = np.asarray(x, dtype=dtype) @ g("embedding.weight").T + g("embedding.bias")
    for i in range(T.num_layers_of(sd)):
        p = f"transformer_encoder.layers.{i}."
        a = window_attention_block(h, g(p + "self_attn.in_proj_weight"), g(p + "self_attn.in_proj_bias"),
                                   g(p + "self_attn.out_proj.weight"), g(p + "self_attn.out_proj.bias"), num_heads, W)
        h = T.layer_norm(h + a, g(p + "norm1.weight"), g(p + "norm1.bias"))
        f = np.maximum(h @ g(p + "linear1.weight").T + g(p + "linear1.bias"), 0) @ g(p + "linear2.weight").T + g(p + "linear2.bias")
        h = T.layer_norm(h + f, g(p + "norm2.weight"), g(p + "norm2.bias"))
    return h @ g("out_layer.weight").T + g("out_layer.bias")


def window_forward(sd, x, W, lengths=None, *, num_heads=4, dtype=np.float64):
    """sd {name: array}, x [B, L, input_dim] -> [B, L, out_dim] in fp64"""
    x = np.asarray(x, dtype=dtype)
    if lengths is None:
        return _forward(sd, x, W, num_heads, dtype) if W > 0 else CB.causal_forward(sd, x, num_heads, dtype)
    B, L = x.shape[:2]
    out = np.broadcast_to(np.asarray(sd["out_layer.bias"], dtype=dtype), (B, L, len(sd["out_layer.bias"]))).copy()
    for b, n in enumerate(int(v) for v in lengths):
        out[b, :n] = window_forward(sd, x[b:b + 1, :n], W, num_heads=num_heads, dtype=dtype)[0]
    return out
