"""Host-side mirror of the reference's `TransformerEncoder` (scripts/tf_encoder.py:5-27) over the
C-ABI `flope_tf_*` (include/flope_amd.h).  Same constructor arguments, same state_dict names, same
call: `enc(x)` with x float32 [B, L, input_dim] on the GPU -> float32 [B, L, out_dim].  Right-padded
ragged batches take `lengths=` (or torch's `src_key_padding_mask=`): each sequence is encoded alone at
its own length, rows behind it come back as `out_layer.bias`, as from the reference module.
Causal attention takes `is_causal=True` or torch's `mask=` holding the causal mask: position t sees positions <= t of its own
sequence, so a track is encoded once and every row is the answer the encoder gives when the track ends there.
Sliding-window causal attention takes `window=W` beside it (or `mask=` holding the banded causal mask): position t sees positions
t - W < j <= t; `enc.open_stream(tracks, capacity, window=W)` is the same live, over a ring cache that is never full.
A 16-bit encoder made with `window_mfma=1` keeps its MFMA attention kernels under a window.
An encoder made with `step_split=1` splits the keys of a stream's step() / extend() over the four waves of a workgroup.
A 16-bit encoder made with `extend_mfma=1` runs a stream's extend() on the MFMA attention step: the MFMA forward's rows in bits.
Any other [L, L] mask is compiled once with `enc.make_mask(mask)` and passed as `mask=` to any number of calls: query i is a softmax over
exactly its allowed keys, a masked key is never loaded, and a sequence of a ragged batch is encoded under the mask's top-left corner
(DESIGN.md 37).  A 16-bit encoder made with `mask_mfma=1` runs attention under a compiled mask on the MFMA attention step over the mask's
tile map, loading only the 64-key blocks some query of a 128-row block allows.
An additive float mask -- torch's `mask=` with values other than -inf / 0, one [L, L] plane or one per head -- is compiled with
`enc.make_bias(bias)` and passed the same way; `alibi_bias(L, slopes)` builds the distance bias this encoder, which has no positional
term, needs to tell the order of the poses behind a query.  A 16-bit encoder made with `bias_mfma=1` runs attention
under a compiled bias on the MFMA attention step over the tile map of the bias's allowed set.
A 16-bit encoder made with `skinny=1` runs every MFMA linear of 1 .. 32 rows -- a live step, a short extend, prefill or forward -- with one
wave per 16-row feature tile instead of a few 128-row workgroups: the same bits, another launch shape.  With
`skinny_ln=1` on top of it, a LayerNorm directly in front of such a linear (model_dim % 64 == 0, at most 512) runs inside the linear's
launch: the same bits again, 2 num_layers - 1 launches fewer per forward; `enc.last_ln` counts them.
The layer's architecture is torch's: `norm_first=True` (pre-norm), `activation="gelu"` (the erf form) and `final_norm=True`
(nn.TransformerEncoder(norm=LayerNorm), state_dict keys transformer_encoder.norm.*) in any combination, through every forward, mask and
stream; `arch_of(module)` reads the three from a torch module.  The defaults are the reference's encoder, bit for bit.

Eval-mode semantics only (dropout is identity), as everywhere in this package.  There is no CPU
path: construction fails loudly without a HIP device or without the built library.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from .engine import _DTYPES, _require_gpu, _stream_ptr


_ACTS = {"relu": _lib.TF_ACT_RELU, "gelu": _lib.TF_ACT_GELU}


def check_arch(norm_first=False, activation="relu", final_norm=False, layer_norm_eps=1e-5) -> dict:
    """The architecture keywords of TransformerEncoder, validated without a device: {"norm_first", "activation", "final_norm"}.
    ValueError on anything the kernels do not run: an activation other than the strings "relu" / "gelu" (torch's erf GELU; the tanh
    form and callables have no kernel), a layer_norm_eps other than 1e-5, flags that are not bools."""
    for name, v in (("norm_first", norm_first), ("final_norm", final_norm)):
        if not isinstance(v, (bool, np.bool_)) and v not in (0, 1):
            raise ValueError(f"{name} must be True or False (got {v!r})")
    if not isinstance(activation, str) or activation not in _ACTS:
        raise ValueError(f'activation must be "relu" or "gelu" (torch\'s erf form); {activation!r} has no kernel')
    if float(layer_norm_eps) != 1e-5:
        raise ValueError(f"layer_norm_eps must be 1e-5 (got {layer_norm_eps!r}): the LayerNorm kernels hold that constant")
    return {"norm_first": bool(norm_first), "activation": activation, "final_norm": bool(final_norm)}


def arch_of(module) -> dict:
    """The three architecture keywords of TransformerEncoder for a torch module that holds an nn.TransformerEncoder as
    `.transformer_encoder` (the reference script's shape): TransformerEncoder(..., **arch_of(m)) runs m's layers.  Works without a
    GPU.  ValueError on anything this encoder cannot run: layers that differ, eps != 1e-5, bias=False, an activation other than ReLU or
    the erf GELU, a final norm that is not an affine LayerNorm over model_dim."""
    import torch.nn.functional as F
    te = getattr(module, "transformer_encoder", None)
    if not isinstance(te, torch.nn.TransformerEncoder):
        raise ValueError("module.transformer_encoder must be an nn.TransformerEncoder")
    found = set()
    for i, ly in enumerate(te.layers):
        if not isinstance(ly, torch.nn.TransformerEncoderLayer):
            raise ValueError(f"layers.{i} is not an nn.TransformerEncoderLayer")
        act = ly.activation
        if act is F.relu or isinstance(act, torch.nn.ReLU):
            name = "relu"
        elif act is F.gelu or (isinstance(act, torch.nn.GELU) and getattr(act, "approximate", "none") == "none"):
            name = "gelu"
        else:
            raise ValueError(f"layers.{i}.activation = {act!r}: only ReLU and the erf GELU have a kernel")
        for n in (ly.norm1, ly.norm2):
            if not isinstance(n, torch.nn.LayerNorm) or n.eps != 1e-5:
                raise ValueError(f"layers.{i}: LayerNorm eps must be 1e-5 (got {getattr(n, 'eps', None)!r})")
            if n.weight is None or n.bias is None:
                raise ValueError(f"layers.{i}: a LayerNorm without weight or bias (bias=False) has no kernel")
        for what, t in (("self_attn.in_proj_bias", ly.self_attn.in_proj_bias), ("self_attn.out_proj.bias", ly.self_attn.out_proj.bias),
                        ("linear1.bias", ly.linear1.bias), ("linear2.bias", ly.linear2.bias)):
            if t is None:
                raise ValueError(f"layers.{i}.{what} is missing (bias=False) and has no kernel")
        found.add((bool(ly.norm_first), name))
    if len(found) > 1:
        raise ValueError(f"the layers differ in (norm_first, activation): {sorted(found)}")
    norm_first, name = found.pop() if found else (False, "relu")
    fn = te.norm
    if fn is not None:
        if not isinstance(fn, torch.nn.LayerNorm) or fn.eps != 1e-5 or fn.weight is None or fn.bias is None:
            raise ValueError("transformer_encoder.norm must be an nn.LayerNorm with eps 1e-5, weight and bias")
    return check_arch(norm_first, name, fn is not None)


def expected_keys(num_layers: int, final_norm: bool = False) -> list:
    keys = ["embedding.weight", "embedding.bias"]
    for i in range(num_layers):
        p = f"transformer_encoder.layers.{i}."
        keys += [p + s for s in ("self_attn.in_proj_weight", "self_attn.in_proj_bias", "self_attn.out_proj.weight",
                                 "self_attn.out_proj.bias", "linear1.weight", "linear1.bias", "linear2.weight",
                                 "linear2.bias", "norm1.weight", "norm1.bias", "norm2.weight", "norm2.bias")]
    if final_norm:
        keys += ["transformer_encoder.norm.weight", "transformer_encoder.norm.bias"]
    return keys + ["out_layer.weight", "out_layer.bias"]


def _host_lengths(lengths, batch):
    """lengths (a sequence or a CPU integer tensor of `batch` values) -> a ctypes int array"""
    if isinstance(lengths, torch.Tensor):
        if lengths.is_cuda or lengths.dtype.is_floating_point or lengths.dtype == torch.bool:
            raise ValueError("lengths must be a sequence or a CPU integer tensor (grid sizes are computed from it on the host)")
        lengths = lengths.reshape(-1).tolist()
    vals = [int(v) for v in lengths]
    if len(vals) != batch:
        raise ValueError(f"lengths has {len(vals)} values for a batch of {batch}")
    if any(v < -2 ** 31 or v >= 2 ** 31 for v in vals):
        raise ValueError("a length does not fit an int")
    return (C.c_int * len(vals))(*vals)


def _mask_to_lengths(mask, B, L):
    """torch's src_key_padding_mask (bool [B, L], True = padding) -> lengths; only right padding has a packed form"""
    mask = torch.as_tensor(mask)
    if mask.dtype != torch.bool or tuple(mask.shape) != (B, L):
        raise ValueError(f"src_key_padding_mask must be a bool tensor {(B, L)}, got {mask.dtype} {tuple(mask.shape)}")
    valid = ~mask.cpu()
    lengths = valid.sum(dim=1)
    prefix = torch.arange(L)[None, :] < lengths[:, None]
    wrong = ((valid != prefix).any(dim=1) | (lengths == 0)).nonzero().reshape(-1).tolist()
    if wrong:
        raise ValueError(f"src_key_padding_mask row {wrong[0]}: the valid entries must form a non-empty prefix of the row (right padding)")
    return lengths.tolist()


def _mask_is_causal(mask, L):
    """torch's `mask` of nn.TransformerEncoder.forward -> True (the causal mask) or False (no mask).  Accepted: None; an all-False bool
    or all-zero floating [L, L] (no mask); the causal [L, L] mask, bool with True exactly above the diagonal or floating with -inf
    exactly above the diagonal and 0 elsewhere (generate_square_subsequent_mask).  Anything else has no kernel and raises ValueError
    naming the first offending (row, col).  Checked on the host: a device mask is copied there."""
    if mask is None:
        return False
    mask = torch.as_tensor(mask)
    if tuple(mask.shape) != (L, L) or not (mask.dtype == torch.bool or mask.dtype.is_floating_point):
        raise ValueError(f"mask must be a bool or floating tensor {(L, L)}, got {mask.dtype} {tuple(mask.shape)}")
    m = mask.detach().cpu()
    above = torch.ones(L, L, dtype=torch.bool).triu(1)
    if m.dtype == torch.bool:
        clear, causal = ~m, m == above
    else:
        m = m.double()
        clear, causal = m == 0, torch.where(above, m == float("-inf"), m == 0)
    if bool(clear.all()):
        return False
    if bool(causal.all()):
        return True
    r, c = (int(v) for v in (~causal).nonzero()[0])
    raise ValueError(f"mask[{r}, {c}] = {mask[r, c].item()!r} is not the causal mask's entry ({'masked' if c > r else 'clear'}): only the "
                     "causal mask (masked exactly above the diagonal) or an all-clear mask has a kernel")


def _mask_window(mask, L):
    """torch's `mask` of nn.TransformerEncoder.forward -> (causal, W).  Accepts everything _mask_is_causal accepts -- None or an
    all-clear [L, L] mask: (False, 0); the causal mask: (True, 0) -- and the banded causal mask: masked exactly where j > i or
    j <= i - W for one W in 1 .. L - 1, bool (True = masked) or floating (-inf / 0): (True, W).  Anything else has no kernel and raises
    ValueError naming the first offending (row, col): the first entry that is not the causal mask's, unless that entry is a masked
    [W, 0] -- then the mask is held to the band of window W and the first entry off that band is named.  Checked on the host."""
    if mask is None:
        return False, 0
    mask = torch.as_tensor(mask)
    if tuple(mask.shape) != (L, L) or not (mask.dtype == torch.bool or mask.dtype.is_floating_point):
        raise ValueError(f"mask must be a bool or floating tensor {(L, L)}, got {mask.dtype} {tuple(mask.shape)}")
    m = mask.detach().cpu()
    if m.dtype == torch.bool:
        clear, masked = ~m, m
    else:
        m = m.double()
        clear, masked = m == 0, m == float("-inf")
    if bool(clear.all()):
        return False, 0
    i, j = torch.arange(L)[:, None], torch.arange(L)[None, :]
    above = j > i
    causal = torch.where(above, masked, clear)
    if bool(causal.all()):
        return True, 0
    r, c = (int(v) for v in (~causal).nonzero()[0])
    if c == 0 and r >= 1 and bool(masked[r, c]):             # the first masked entry below the diagonal of a band of window r
        band = torch.where(above | (j <= i - r), masked, clear)
        if bool(band.all()):
            return True, r
        r2, c2 = (int(v) for v in (~band).nonzero()[0])
        want = "masked" if c2 > r2 or c2 <= r2 - r else "clear"
        raise ValueError(f"mask[{r2}, {c2}] = {mask[r2, c2].item()!r} is not the entry of the banded causal mask of window {r} ({want}), "
                         f"which mask[{r}, 0] starts: only the causal mask, a banded causal mask (masked exactly where col > row or "
                         "col <= row - W) or an all-clear mask has a kernel")
    raise ValueError(f"mask[{r}, {c}] = {mask[r, c].item()!r} is not the causal mask's entry ({'masked' if c > r else 'clear'}): only the "
                     "causal mask (masked exactly above the diagonal), a banded causal mask (also masked where col <= row - W) or an "
                     "all-clear mask has a kernel")


def _mask_allowed(mask):
    """torch's `mask` of nn.TransformerEncoder.forward, any square one -> the bool [L, L] CPU tensor of ALLOWED pairs.  bool: True =
    masked (torch's convention); floating: -inf = masked, 0 = allowed, anything else raises ValueError naming the first such entry.
    No pattern is looked for."""
    mask = torch.as_tensor(mask)
    if mask.dim() != 2 or mask.shape[0] != mask.shape[1] or mask.shape[0] < 1 or not (mask.dtype == torch.bool or mask.dtype.is_floating_point):
        raise ValueError(f"mask must be a bool or floating tensor [L, L] with L >= 1, got {mask.dtype} {tuple(mask.shape)}")
    m = mask.detach().cpu()
    if m.dtype == torch.bool:
        return ~m
    m = m.double()
    allowed, masked = m == 0, m == float("-inf")
    wrong = ~(allowed | masked)
    if bool(wrong.any()):
        r, c = (int(v) for v in wrong.nonzero()[0])
        raise ValueError(f"mask[{r}, {c}] = {mask[r, c].item()!r}: a floating mask holds -inf (masked) or 0 (allowed); additive biases have no kernel")
    return allowed


def _pack_allowed(allowed):
    """bool [L, L] of allowed pairs -> the uint32 words [L][ceil(L / 32)] flope_tf_mask_create takes (bit j % 32 of word j / 32)"""
    L = allowed.shape[0]
    words = (L + 31) // 32
    a = torch.zeros(L, words * 32, dtype=torch.int64)
    a[:, :L] = allowed.to(torch.int64)
    packed = (a.view(L, words, 32) << torch.arange(32, dtype=torch.int64)).sum(dim=2)
    return (C.c_uint32 * (L * words))(*packed.reshape(-1).tolist())


def alibi_bias(L, slopes, causal=True):
    """The ALiBi bias for sequences of L tokens, float32 [len(slopes), L, L]: -slopes[h] * |i - j| for query i and key j of head h, and
    with `causal` -inf above the diagonal.  Pass it to `enc.make_bias` (len(slopes) = num_heads, or 1).  This encoder has no
    positional term, so without it a causal or windowed forward cannot tell in which order the poses behind a query came."""
    slopes = torch.as_tensor(slopes, dtype=torch.float32).reshape(-1)
    i, j = torch.arange(int(L))[:, None], torch.arange(int(L))[None, :]
    bias = -slopes[:, None, None] * (i - j).abs().to(torch.float32)[None]
    if causal:
        bias = bias.masked_fill((j > i)[None], float("-inf"))
    return bias


def alibi_distances(D, slopes):
    """The ALiBi distance table for a stream (`enc.open_stream(..., bias=)`), float32 [len(slopes), D]: -slopes[h] * dist for
    dist = 0 .. D - 1, the products `alibi_bias` makes, so that distance_bias(alibi_distances(L, s), L) is alibi_bias(L, s) bit for
    bit.  D is the state's window, or its capacity without one."""
    slopes = torch.as_tensor(slopes, dtype=torch.float32).reshape(-1)
    return -slopes[:, None] * torch.arange(int(D)).abs().to(torch.float32)[None]


def distance_bias(table, L, window=0):
    """The [planes, L, L] bias a distance table stands for, float32: entry [h][i][j] is table[h][i - j] for j <= i and, with `window`,
    i - j < window, and -inf elsewhere -- what `enc.make_bias` takes, and the forward under it is what a stream opened with
    `bias=table` returns row by row.  table: floating [D] or [planes, D] with D >= min(L, window or L) (ValueError)."""
    table = torch.as_tensor(table)
    L, window = int(L), int(window)
    if table.dim() not in (1, 2) or not table.dtype.is_floating_point:
        raise ValueError(f"table must be a floating tensor [D] or [planes, D], got {table.dtype} {tuple(table.shape)}")
    if L < 1 or window < 0:
        raise ValueError(f"L must be positive and window 0 (none) or positive, got L = {L}, window = {window}")
    t = table.detach().to(device="cpu", dtype=torch.float32).reshape(-1, table.shape[-1])
    need = min(L, window or L)
    if t.shape[1] < need:
        raise ValueError(f"table has {t.shape[1]} distances, a forward of L = {L}" + (f" under window = {window}" if window else "") + f" needs {need}")
    i, j = torch.arange(L)[:, None], torch.arange(L)[None, :]
    dist = i - j
    seen = (dist >= 0) & ((dist < window) if window else torch.ones_like(dist, dtype=torch.bool))
    bias = t[:, dist.clamp(0, t.shape[1] - 1)]
    return bias.masked_fill(~seen[None], float("-inf")).contiguous()


class TransformerEncoder:
    def __init__(self, input_dim, model_dim, out_dim, num_heads, num_layers, ff_dim, dropout=0.1,
                 dtype="f32", max_tokens=4096, device=None, attn_tiled=0, fused=0, window_mfma=0, step_split=0, extend_mfma=0,
                 mask_mfma=0, bias_mfma=0, skinny=0, skinny_ln=0, norm_first=False, activation="relu", final_norm=False, layer_norm_eps=1e-5):
        self.arch = check_arch(norm_first, activation, final_norm, layer_norm_eps)       # torch's keywords, readable back
        _require_gpu()
        self.lib = _lib.load()
        self.device = torch.device(device if device is not None else "cuda:0")
        if self.device.type != "cuda":
            raise RuntimeError("flope_amd.TransformerEncoder runs on a HIP device only (no CPU path)")
        self.dims = (input_dim, model_dim, out_dim, num_heads, num_layers, ff_dim)
        self.dropout = dropout          # kept for signature parity; eval mode -> identity
        self.dtype = dtype
        self.max_tokens = int(max_tokens)
        self.handle = C.c_void_p()
        idx = self.device.index if self.device.index is not None else 0
        rc = self.lib.flope_tf_create(idx, input_dim, model_dim, out_dim, num_heads, num_layers, ff_dim,
                                      self.max_tokens, _DTYPES[dtype], C.byref(self.handle))
        if rc:
            msg = self.lib.flope_tf_last_error(None)
            raise RuntimeError(f"flope_tf_create failed ({rc}): {msg.decode() if msg else ''}")
        if dtype == "f32m":                      # a FLOPE_DT_F32 handle with the linears and attention on the exact-fp32 MFMA
            rc = self.lib.flope_tf_set_option(self.handle, b"f32mfma", 1)
            if rc < 0:
                self.close()
                raise RuntimeError(f"flope_tf_set_option(f32mfma) failed ({rc})")
        if self.arch != check_arch():            # the architecture, stated before the weights are loaded (include/flope_amd.h)
            for name, value in (("norm_first", int(self.arch["norm_first"])), ("activation", _ACTS[self.arch["activation"]]),
                                ("final_norm", int(self.arch["final_norm"]))):
                rc = self.lib.flope_tf_set_option(self.handle, name.encode(), value)
                if rc < 0:
                    self.close()
                    raise RuntimeError(f"flope_tf_set_option({name}) failed ({rc})")
        self.last_attn_kernel = None             # FLOPE_TF_ATTN_* id of the last attention() launch
        self.last_linear_kernel = None           # FLOPE_TF_LIN_* id of the last linear() launch
        self.last_ln_kernel = None               # FLOPE_TF_LN_* id of the last layernorm() launch
        if attn_tiled:                           # 16-bit handles: MFMA attention for head_dim 32 .. 128 at any length (0 .. 2, include/flope_amd.h)
            rc = self.lib.flope_tf_set_option(self.handle, b"attn_tiled", int(attn_tiled))
            if rc < 0:
                self.close()
                raise ValueError(f"attn_tiled must be 0, 1 or 2 (got {attn_tiled!r})")
        self.last_forward_fused = False          # whether the last forward() ran as the single launch of option "fused"
        if fused:                                # float32 handles: one launch per forward where a sequence fits in LDS (0 or 1, include/flope_amd.h)
            rc = self.lib.flope_tf_set_option(self.handle, b"fused", int(fused))
            if rc < 0:
                self.close()
                raise ValueError(f"fused must be 0 or 1 (got {fused!r})")
        if window_mfma:                          # 16-bit handles: a windowed attention keeps its MFMA kernel (0 or 1, include/flope_amd.h)
            rc = self.lib.flope_tf_set_option(self.handle, b"window_mfma", int(window_mfma))
            if rc < 0:
                self.close()
                raise ValueError(f"window_mfma must be 0 or 1 (got {window_mfma!r})")
        if step_split:                           # every dtype: a stream's step / extend split a token's keys over four waves (0 or 1, include/flope_amd.h)
            rc = self.lib.flope_tf_set_option(self.handle, b"step_split", int(step_split))
            if rc < 0:
                self.close()
                raise ValueError(f"step_split must be 0 or 1 (got {step_split!r})")
        if extend_mfma:                          # 16-bit handles: a stream's extend runs its attention on the MFMA step (0 or 1, include/flope_amd.h)
            rc = self.lib.flope_tf_set_option(self.handle, b"extend_mfma", int(extend_mfma))
            if rc < 0:
                self.close()
                raise ValueError(f"extend_mfma must be 0 or 1 (got {extend_mfma!r})")
        if mask_mfma:                            # 16-bit handles: attention under a compiled mask runs on the MFMA step (0 or 1, include/flope_amd.h)
            rc = self.lib.flope_tf_set_option(self.handle, b"mask_mfma", int(mask_mfma))
            if rc < 0:
                self.close()
                raise ValueError(f"mask_mfma must be 0 or 1 (got {mask_mfma!r})")
        if bias_mfma:                            # 16-bit handles: attention under a compiled bias runs on the MFMA step (0 or 1, include/flope_amd.h)
            rc = self.lib.flope_tf_set_option(self.handle, b"bias_mfma", int(bias_mfma))
            if rc < 0:
                self.close()
                raise ValueError(f"bias_mfma must be 0 or 1 (got {bias_mfma!r})")
        if skinny:                               # 16-bit handles: an MFMA linear of 1 .. 32 rows runs one wave per 16-row feature tile, the same bits (0 or 1, include/flope_amd.h)
            rc = self.lib.flope_tf_set_option(self.handle, b"skinny", int(skinny))
            if rc < 0:
                self.close()
                raise ValueError(f"skinny must be 0 or 1 (got {skinny!r})")
        if skinny_ln:                            # 16-bit handles under skinny=1: a LayerNorm in front of a skinny linear of K = model_dim <= 512 runs inside that linear's launch, the same bits (0 or 1, include/flope_amd.h)
            rc = self.lib.flope_tf_set_option(self.handle, b"skinny_ln", int(skinny_ln))
            if rc < 0:
                self.close()
                raise ValueError(f"skinny_ln must be 0 or 1 (got {skinny_ln!r})")

    def _check(self, rc):
        if rc:
            msg = self.lib.flope_tf_last_error(self.handle)
            raise RuntimeError(f"flope_amd error {rc}: {msg.decode() if msg else ''}")

    # nn.Module-style no-ops the reference's callers use
    def eval(self):
        return self

    def to(self, device):
        if torch.device(device) != self.device and torch.device(device).index not in (None, self.device.index):
            raise RuntimeError("the encoder is bound to the device it was created on")
        return self

    def load_state_dict(self, sd: dict) -> None:
        want = expected_keys(self.dims[4], self.arch["final_norm"])
        if not self.arch["final_norm"] and "transformer_encoder.norm.weight" in sd:
            raise ValueError("state_dict holds transformer_encoder.norm.weight, but this encoder was made with final_norm=False: "
                             "dropping a trained norm gives wrong poses (see arch_of)")
        missing = [k for k in want if k not in sd]
        if missing:
            raise KeyError(f"state_dict is missing {missing[:3]}{'...' if len(missing) > 3 else ''}")
        items = [(k, torch.as_tensor(sd[k]).detach().to("cpu", torch.float32).contiguous()) for k in want]
        n = len(items)
        names = (C.c_char_p * n)(*[k.encode() for k, _ in items])
        ptrs = (C.c_void_p * n)(*[t.data_ptr() for _, t in items])
        ndims = (C.c_int * n)(*[t.dim() for _, t in items])
        shape_arrs = [(C.c_int64 * max(t.dim(), 1))(*t.shape) for _, t in items]
        shapes = (C.c_void_p * n)(*[C.cast(a, C.c_void_p).value for a in shape_arrs])
        with torch.cuda.device(self.device):
            self._check(self.lib.flope_tf_load_weights(self.handle, n, names, ptrs, ndims, shapes))

    def set_option(self, name: str, value: int) -> int:
        if name in ("step_split", "extend_mfma", "mask_mfma", "bias_mfma", "skinny", "skinny_ln", "norm_first", "activation", "final_norm"):    # the newer options raise on a refused value (the others keep returning the code)
            rc = self.lib.flope_tf_set_option(self.handle, name.encode(), int(value))
            self._check_arg(rc)
            return rc
        return self.lib.flope_tf_set_option(self.handle, name.encode(), int(value))

    def _state_causal(self, causal):
        """Every call that runs or counts attention states the option first, so a plain call after a causal one is non-causal"""
        rc = self.lib.flope_tf_set_option(self.handle, b"causal", int(bool(causal)))
        if rc < 0:
            raise RuntimeError(f"flope_tf_set_option(causal) failed ({rc})")

    def _state_window(self, causal, window):
        """... and the window beside it: `window` > 0 needs causal (ValueError), anything else is stated as it is"""
        window = int(window)
        if window < 0:
            raise ValueError(f"window must be 0 (none) or a positive number of keys, got {window}")
        if window > 0 and not causal:
            raise ValueError(f"window={window} needs is_causal=True or a causal / banded mask: a window without causal has no kernel")
        self._state_causal(causal)
        rc = self.lib.flope_tf_set_option(self.handle, b"window", window)
        if rc < 0:
            raise RuntimeError(f"flope_tf_set_option(window) failed ({rc})")

    def make_mask(self, mask) -> "TransformerEncoderMask":
        """Compiles any [L, L] attention mask -- bool (True = masked, torch's convention) or floating (-inf / 0), on any device -- into
        a device-resident TransformerEncoderMask that forward(), attention(), flops() and forward_plan() take as `mask=` (DESIGN.md
        37).  No pattern is recognised: a causal tensor compiled this way runs the masked kernel.  ValueError: another shape, dtype or
        value (the first offending entry is named), a row without an allowed key (the reference returns NaN there), L > max_tokens."""
        return TransformerEncoderMask(self, mask)

    def make_bias(self, bias) -> "TransformerEncoderMask":
        """Compiles an additive attention bias -- a floating [L, L] tensor (one plane for every head) or [H, L, L] (one per head), on
        any device -- into a TransformerEncoderMask that forward() and attention() take as `mask=`, fixed-length and ragged (DESIGN.md
        39).  -inf = masked, as in make_mask: never loaded.  Any finite value is added to the pair's scaled score before the softmax
        (torch's float `mask`); the values are kept as float32 whatever the encoder's dtype.  Torch's 3-D form [B * H, L, L] is this
        [H, L, L] repeated batch-major: pass one batch element's H planes.  A sequence of n tokens of a ragged batch is encoded under
        the top-left n x n corner of every plane.  `.planes` of the result is 1 or H.  ValueError: another shape or dtype, +inf or NaN
        (the message names plane, row, col), planes whose -inf entries differ (write a per-head difference as a large negative finite
        value), a row without an allowed key, L > max_tokens."""
        return TransformerEncoderMask(self, None, bias=bias)

    def _compiled(self, mask, seq_len, is_causal, window):
        """The checks every call that takes a compiled mask starts with"""
        if mask.enc is not self:
            raise ValueError("the mask was compiled by another encoder")
        mask._live()
        if is_causal or int(window) != 0:
            raise ValueError("a compiled mask together with is_causal=True or window != 0: say it in the mask")
        if seq_len is not None and int(seq_len) != mask.L:
            raise ValueError(f"the mask was compiled for sequences of {mask.L} tokens, this call has {int(seq_len)}")

    def flops(self, batch: int, seq_len: int, lengths=None, *, is_causal=False, window=0, mask=None) -> float:
        """Algorithmic FLOPs of one forward; `is_causal`: attention counted over the keys a causal forward meets, `window`: over
        the min(t + 1, window) keys query t meets under a window, `mask` (a compiled one): over its allowed pairs."""
        if isinstance(mask, TransformerEncoderMask):
            self._compiled(mask, seq_len, is_causal, window)
            return self.lib.flope_tf_forward_flops_masked(self.handle, int(batch), None if lengths is None else _host_lengths(lengths, batch), mask.handle)
        self._state_window(is_causal, window)
        if lengths is None:
            return self.lib.flope_tf_forward_flops(self.handle, batch, seq_len)
        return self.lib.flope_tf_forward_flops_varlen(self.handle, batch, _host_lengths(lengths, batch))

    def forward_plan(self, batch: int, seq_len: int, lengths=None, *, is_causal=False, window=0, mask=None) -> str:
        """"fused" or "launches": what forward() of x [batch, seq_len, input_dim] (with these `lengths`, with `is_causal`, with
        `window`: always "launches", with a compiled `mask`: always "launches") would run under the current options.  Enqueues
        nothing; a shape the forward refuses raises ValueError."""
        if isinstance(mask, TransformerEncoderMask):
            self._compiled(mask, seq_len, is_causal, window)
            return "launches"
        self._state_window(is_causal, window)
        with torch.cuda.device(self.device):
            rc = self.lib.flope_tf_forward_plan(self.handle, int(batch), int(seq_len), None if lengths is None else _host_lengths(lengths, batch))
        self._check_arg(rc)
        return "fused" if rc == _lib.TF_FWD_FUSED else "launches"

    # The entry points added after the fixed-length forward (the ragged calls, linear, layernorm) share this checker: a refused call
    # (FLOPE_EINVAL: a bad length, too many tokens, a misaligned buffer, an unknown name) is the caller's argument and raises
    # ValueError, and a result >= 0 (a kernel id) passes.  _check keeps raising RuntimeError for forward() and attention() without
    # lengths, whose behaviour stays as it was.  For the same reason only the newer calls are wrapped in torch.cuda.device().
    def _check_arg(self, rc):
        if rc < 0:
            msg = self.lib.flope_tf_last_error(self.handle)
            msg = msg.decode() if msg else ""
            raise (ValueError if rc == _lib.EINVAL else RuntimeError)(f"flope_amd error {rc}: {msg}")

    def forward(self, x: torch.Tensor, lengths=None, src_key_padding_mask=None, *, mask=None, is_causal=False, window=0) -> torch.Tensor:
        """x [B, L, input_dim] -> [B, L, out_dim].  `lengths`: a sequence or CPU integer tensor of B values, 1 <= lengths[b] <= L --
        sequence b is x[b, :lengths[b]], the rows behind it are padding (never read) and come back as out_layer.bias.
        `src_key_padding_mask`: bool [B, L], True = padding (torch's convention); it must mask a suffix of every row and is turned
        into lengths on the host.  With neither, every sequence has length L (the fixed-length path, unchanged).
        `is_causal=True`, or `mask` = the [L, L] causal mask (torch's generate_square_subsequent_mask(L), or bool with True above the
        diagonal): row t attends to rows <= t of its own sequence, so forward(x[:, :n], is_causal=True) is the first n rows of
        forward(x, is_causal=True), bit for bit.  An all-clear `mask` means none; any other mask, or one that contradicts
        `is_causal=True`, raises ValueError.  The mask is checked on the host: a device mask costs a copy, `is_causal=True` costs
        nothing.  Two deliberate differences from torch: `is_causal=True` without a mask means causal here (torch ignores that hint
        silently), and with `lengths` the rows behind a sequence still come back as out_layer.bias, never read (torch leaves its
        nested-tensor path once a mask is given and computes something there).
        `window=W` (W >= 1, with `is_causal=True` or such a mask; ValueError without), or `mask` = the banded causal [L, L] mask
        (masked exactly where col > row or col <= row - W, bool or -inf / 0): row t attends to rows t - W < j <= t of its own sequence
        (inside each sequence with `lengths`).  With `window_mfma=0` attention then runs the generic kernel for every dtype and shape,
        and W >= L gives the generic causal kernel's bits; on a handle made with `window_mfma=1` a 16-bit forward keeps the MFMA
        kernel it would run without a window, and W >= L gives that kernel's causal bits.  The forward is never the
        single launch.  A banded mask together with another `window` raises
        ValueError.  The option is stated per call: a plain call after a windowed one has no window.
        `mask` = a TransformerEncoderMask (make_mask): any set of allowed (query, key) pairs, see there; with `is_causal=True` or a
        `window` it raises ValueError.  One made by make_bias also adds its float32 value to every allowed pair's score, per head
        where it has H planes."""
        if not x.is_cuda or x.device != self.device:
            raise RuntimeError(f"input must live on {self.device} (got {x.device}); no CPU path")
        if x.dim() != 3 or x.shape[2] != self.dims[0]:
            raise ValueError(f"expected [B, L, {self.dims[0]}], got {tuple(x.shape)}")
        if lengths is not None and src_key_padding_mask is not None:
            raise ValueError("give lengths or src_key_padding_mask, not both")
        x = x.to(torch.float32).contiguous()
        B, L = x.shape[0], x.shape[1]
        if src_key_padding_mask is not None:
            lengths = _mask_to_lengths(src_key_padding_mask, B, L)
        if isinstance(mask, TransformerEncoderMask):
            # a compiled mask (make_mask): any [L, L] set of allowed pairs.  Sequence b of a ragged batch is encoded
            # alone under the mask's top-left lengths[b] x lengths[b] corner.  Always the launch sequence; options "causal" and
            # "window" are neither read nor written.  On an encoder with `mask_mfma=1` a 16-bit forward runs its attention on the
            # MFMA kernel over the mask's tile map; the id of the attention launches is kept in `last_attn_kernel`.
            self._compiled(mask, L, is_causal, window)
            y = torch.empty((B, L, self.dims[2]), dtype=torch.float32, device=self.device)
            lh = None if lengths is None else _host_lengths(lengths, B)
            with torch.cuda.device(self.device):
                self._check_arg(self.lib.flope_tf_forward_masked(self.handle, x.data_ptr(), B, L, lh, mask.handle, y.data_ptr(), _stream_ptr(self.device)))
            self.last_forward_fused = False
            self.last_attn_kernel = self.lib.flope_tf_last_forward_masked(self.handle)       # tf_attn_masked, tf_attn_tiled_masked under mask_mfma, the BIASED instantiation of either under a bias (of the second: bias_mfma)
            self._keep = x
            return y
        causal, band = _mask_window(mask, L)
        if is_causal and mask is not None and not causal:
            raise ValueError("is_causal=True with a mask that is not the causal mask")
        window = int(window)
        if band and window and window != band:
            raise ValueError(f"window={window} with a banded mask of window {band}")
        self._state_window(causal or is_causal, window or band)
        y = torch.empty((B, L, self.dims[2]), dtype=torch.float32, device=self.device)
        lh = None if lengths is None else _host_lengths(lengths, B)
        if lengths is None:
            self._check(self.lib.flope_tf_forward(self.handle, x.data_ptr(), B, L, y.data_ptr(), _stream_ptr(self.device)))
        else:
            with torch.cuda.device(self.device):
                self._check_arg(self.lib.flope_tf_forward_varlen(self.handle, x.data_ptr(), B, L, lh, y.data_ptr(),
                                                                    _stream_ptr(self.device)))
        self.last_forward_fused = self.lib.flope_tf_last_forward(self.handle) == _lib.TF_FWD_FUSED      # what that forward recorded
        self._keep = x
        return y

    __call__ = forward

    def attention(self, qkv: torch.Tensor, lengths=None, out: torch.Tensor = None, *, is_causal=False, window=0, mask=None) -> torch.Tensor:
        """softmax(q k^T / sqrt(head_dim)) v per head of qkv [B, L, 3 * model_dim] in the handle's dtype -> [B, L, model_dim], by
        the kernel a forward of this (B, L) would launch under the current options; its id is kept in `last_attn_kernel`.  Needs no
        weights.  `out`: a contiguous tensor of the result's shape and dtype to write into.
        With `lengths` (B values), qkv is the packed 2-D [T, 3 * model_dim] of a ragged batch, T = sum(lengths), sequence b at rows
        sum(lengths[:b]) onwards; the result is the packed [T, model_dim].
        `is_causal`: query i attends to keys <= i of its own sequence; the kernel is the one the shape picks without it.
        `window=W` (with `is_causal=True`): keys i - W < j <= i, by the generic kernel with `window_mfma=0`, by the 16-bit MFMA
        kernel the call would take without a window on a handle made with `window_mfma=1`.
        `mask` (a compiled one, make_mask): softmax over the allowed keys only, by tf_attn_masked (`last_attn_kernel` = 4) for every
        dtype and shape, or, on a 16-bit encoder with `mask_mfma=1` and head_dim 32 / 64 / 96 / 128, by tf_attn_tiled_masked
        (`last_attn_kernel` = 5); with `lengths` each sequence under the mask's corner.  A compiled bias (make_bias) is
        passed the same way and runs the BIASED instantiation of tf_attn_masked (`last_attn_kernel` = 6) on every dtype and under every option
        but `bias_mfma=1`, under which a 16-bit encoder at head_dim 32 / 64 / 96 / 128 runs the BIASED instantiation of tf_attn_tiled_masked
        (`last_attn_kernel` = 7)."""
        if mask is not None and not isinstance(mask, TransformerEncoderMask):
            raise ValueError("attention() takes a compiled mask (enc.make_mask), not a tensor")
        if mask is not None:
            self._compiled(mask, None, is_causal, window)
        else:
            self._state_window(is_causal, window)
        tdt = {"f16": torch.float16, "bf16": torch.bfloat16}.get(self.dtype, torch.float32)
        d = self.dims[1]
        if not qkv.is_cuda or qkv.device != self.device:
            raise RuntimeError(f"input must live on {self.device} (got {qkv.device}); no CPU path")
        if lengths is not None:
            n = len(lengths)
            lh = _host_lengths(lengths, n)
            T = sum(int(v) for v in lh)
            if qkv.dim() != 2 or qkv.shape[1] != 3 * d or qkv.dtype != tdt or not qkv.is_contiguous() or qkv.shape[0] != T:
                raise ValueError(f"expected a contiguous {tdt} tensor [{T}, {3 * d}] (T = sum(lengths)), got {qkv.dtype} {tuple(qkv.shape)}")
            if out is None:
                out = torch.empty((T, d), dtype=tdt, device=self.device)
            elif out.shape != (T, d) or out.dtype != tdt or out.device != self.device or not out.is_contiguous():
                raise ValueError(f"out must be a contiguous {tdt} tensor {(T, d)} on {self.device}")
            with torch.cuda.device(self.device):
                if mask is not None:
                    rc = self.lib.flope_tf_attention_masked(self.handle, qkv.data_ptr(), n, mask.L, lh, mask.handle, out.data_ptr(), _stream_ptr(self.device))
                else:
                    rc = self.lib.flope_tf_attention_varlen(self.handle, qkv.data_ptr(), n, lh, out.data_ptr(), _stream_ptr(self.device))
            self._check_arg(rc)
            self.last_attn_kernel = rc
            self._keep = qkv
            return out
        if qkv.dim() != 3 or qkv.shape[2] != 3 * d or qkv.dtype != tdt or not qkv.is_contiguous():
            raise ValueError(f"expected a contiguous {tdt} tensor [B, L, {3 * d}], got {qkv.dtype} {tuple(qkv.shape)}")
        B, L = qkv.shape[0], qkv.shape[1]
        if out is None:
            out = torch.empty((B, L, d), dtype=tdt, device=self.device)
        elif out.shape != (B, L, d) or out.dtype != tdt or out.device != self.device or not out.is_contiguous():
            raise ValueError(f"out must be a contiguous {tdt} tensor {(B, L, d)} on {self.device}")
        if mask is not None:
            with torch.cuda.device(self.device):
                rc = self.lib.flope_tf_attention_masked(self.handle, qkv.data_ptr(), B, L, None, mask.handle, out.data_ptr(), _stream_ptr(self.device))
            self._check_arg(rc)
        else:
            rc = self.lib.flope_tf_attention(self.handle, qkv.data_ptr(), B, L, out.data_ptr(), _stream_ptr(self.device))
        if rc < 0:
            self._check(rc)
        self.last_attn_kernel = rc
        self._keep = qkv
        return out

    # ---- one operation of the forward on a caller's tensor (include/flope_amd.h: flope_tf_linear, flope_tf_layernorm) ----------
    def _tdt(self):
        return {"f16": torch.float16, "bf16": torch.bfloat16}.get(self.dtype, torch.float32)

    def _padded(self, t, rows, cols, dt, what):
        """`t` [rows, cols] as a tensor whose storage holds roundup(rows, 128) rows from its first element on (16-bit handles: the
        MFMA linear reads and writes whole 128-row tiles).  A contiguous view with that much room behind it is used as it is,
        anything else is copied to the head of a fresh padded allocation whose pad rows are zero."""
        if t.device != self.device:
            raise RuntimeError(f"{what} must live on {self.device} (got {t.device}); no CPU path")
        if t.dim() != 2 or tuple(t.shape) != (rows, cols) or t.dtype != dt:
            raise ValueError(f"{what}: expected a {dt} tensor [{rows}, {cols}], got {t.dtype} {tuple(t.shape)}")
        if self.dtype in ("f32", "f32m"):
            return t if t.is_contiguous() else t.contiguous()
        need = (rows + 127) // 128 * 128 * cols
        room = t.untyped_storage().nbytes() // t.element_size() - t.storage_offset()
        if t.is_contiguous() and room >= need:
            return t
        big = torch.zeros(need, dtype=dt, device=self.device)
        big[:rows * cols] = t.reshape(-1)
        return big[:rows * cols].view(rows, cols)

    def _linear_dims(self, name):
        i, d, o, _, nl, ff = self.dims
        if name == "embedding":
            return d, i
        if name == "out_layer":
            return o, d
        parts = name.split(".")
        if len(parts) == 3 and parts[0] == "layers" and parts[1].isdigit() and int(parts[1]) < nl:
            nk = {"in_proj": (3 * d, d), "out_proj": (d, d), "linear1": (ff, d), "linear2": (d, ff)}.get(parts[2])
            if nk:
                return nk
        raise ValueError(f"unknown linear {name!r}: embedding, out_layer, layers.<i>.in_proj / out_proj / linear1 / linear2")

    @staticmethod
    def _act_id(relu, act):
        """the FLOPE_TF_ACT_* id of linear()'s / linear_ln_act()'s `relu=` flag and `act=` name; ValueError where both are given and disagree"""
        if act is None:
            return _lib.TF_ACT_RELU if relu else _lib.TF_ACT_NONE
        if not isinstance(act, str) or act not in _ACTS:
            raise ValueError(f'act must be None, "relu" or "gelu" (got {act!r})')
        if relu and act != "relu":
            raise ValueError(f"relu=True together with act={act!r}")
        return _ACTS[act]

    def linear(self, name, x, res=None, relu=False, out_f32=False, out=None, act=None):
        """act(x W^T + b (+ res)) of the loaded linear `name` ("embedding", "out_layer", "layers.<i>.in_proj" / ".out_proj" /
        ".linear1" / ".linear2") by the kernel a forward launches for it at this row count under the current options; its
        FLOPE_TF_LIN_* id is kept in `last_linear_kernel`.  x [rows, K] in the handle's dtype, or float32 (the network input; the only form
        an MFMA embedding with input_dim % 64 != 0 takes, since its kernel reads zero-padded rows: ValueError otherwise);
        res [rows, N] in the handle's dtype; the result is [rows, N] in the handle's dtype, float32 with out_f32.
        16-bit handles: x, res and the result live in storage of roundup(rows, 128) rows (the MFMA linear works on whole 128-row
        tiles: pad rows of x and res may hold anything, those of the result are overwritten).  A tensor that is a view with that
        much room behind it is used in place -- the result keeps its padded storage --, any other is copied into one.
        `out`: a [rows, N] tensor to write into, under the same rule (never copied: too little room is an error).
        `act`: "relu" or "gelu" (torch's erf GELU on the float32 accumulator) beside the `relu` flag; ValueError if both
        are given and disagree, and for GELU together with `res`, which has no kernel."""
        aid = self._act_id(relu, act)
        if aid == _lib.TF_ACT_GELU and res is not None:
            raise ValueError("act=\"gelu\" together with res has no kernel")
        tdt = self._tdt()
        N, K = self._linear_dims(name)
        if x.dim() != 2 or x.shape[1] != K:
            raise ValueError(f"{name}: expected [rows, {K}], got {tuple(x.shape)}")
        rows = x.shape[0]
        f16h = self.dtype in ("f16", "bf16")
        x_f32 = f16h and x.dtype == torch.float32
        x = self._padded(x, rows, K, torch.float32 if x_f32 else tdt, "x")
        if res is not None:
            res = self._padded(res, rows, N, tdt, "res")
        odt = torch.float32 if (out_f32 or not f16h) else tdt
        if out is None:
            rpad = (rows + 127) // 128 * 128 if f16h else rows
            out = torch.empty((rpad, N), dtype=odt, device=self.device)[:rows]
        elif self._padded(out, rows, N, odt, "out") is not out:
            raise ValueError(f"out must be a contiguous {odt} tensor [{rows}, {N}] with storage for {(rows + 127) // 128 * 128} rows")
        with torch.cuda.device(self.device):
            rc = self.lib.flope_tf_linear_act(self.handle, name.encode(), x.data_ptr(), int(x_f32), res.data_ptr() if res is not None else None,
                                              out.data_ptr(), int(odt == torch.float32), rows, aid, _stream_ptr(self.device))
        self._check_arg(rc)
        self.last_linear_kernel = rc
        self._keep = (x, res)
        return out

    def linear_plan(self, name, rows):
        """The FLOPE_TF_LIN_* id linear() would launch for the loaded linear `name` at `rows` rows under the current options, in the form
        a forward runs it (embedding: float32 in; out_layer: float32 out; out_proj / linear2: with a residual; linear1: with the encoder's activation).
        Launches nothing."""
        self._linear_dims(name)
        rc = self.lib.flope_tf_linear_plan(self.handle, name.encode(), int(rows))
        self._check_arg(rc)
        return rc

    def linear_ln(self, name, x, weight, bias, relu=False, out=None, normed=None):
        """(y, normed): normed = LayerNorm(x; weight, bias) and y = act(normed W^T + b) of the loaded linear `name` in the ONE launch a
        forward runs for the pair under option skinny_ln (tf_gemm_skinny_ln); the id (FLOPE_TF_LIN_SKINNY_LN = 6) is kept
        in `last_linear_kernel`.  x [rows, model_dim] in the handle's 16-bit dtype, weight / bias device float32 [model_dim].  ValueError
        where the option's rule has no such launch for this handle, linear and row count (linear_ln_plan tells).  The storage rule of
        linear(): x, y and normed live in storage of roundup(rows, 128) rows; `out` / `normed`: tensors to write into, never copied.
        x must not share storage with either result."""
        return self.linear_ln_act(name, x, weight, bias, "relu" if relu else None, out=out, normed=normed)

    def linear_ln_act(self, name, x, weight, bias, act, out=None, normed=None):
        """linear_ln() with the activation named: `act` None, "relu" or "gelu" (DESIGN.md 50)."""
        aid = self._act_id(False, act)
        tdt, d = self._tdt(), self.dims[1]
        N, K = self._linear_dims(name)
        if x.dim() != 2 or x.shape[1] != d:
            raise ValueError(f"{name}: expected [rows, {d}], got {tuple(x.shape)}")
        rows = x.shape[0]
        for t in (weight, bias):
            if t.device != self.device or tuple(t.shape) != (d,) or t.dtype != torch.float32 or not t.is_contiguous():
                raise ValueError(f"weight and bias must be contiguous float32 [{d}] on {self.device}")
        x = self._padded(x, rows, d, tdt, "x")
        rpad = (rows + 127) // 128 * 128
        res = []
        for t, cols, what in ((out, N, "out"), (normed, d, "normed")):
            if t is None:
                t = torch.empty((rpad, cols), dtype=tdt, device=self.device)[:rows]
            elif self._padded(t, rows, cols, tdt, what) is not t:
                raise ValueError(f"{what} must be a contiguous {tdt} tensor [{rows}, {cols}] with storage for {rpad} rows")
            res.append(t)
        out, normed = res
        with torch.cuda.device(self.device):
            rc = self.lib.flope_tf_linear_ln_act(self.handle, name.encode(), x.data_ptr(), weight.data_ptr(), bias.data_ptr(), normed.data_ptr(),
                                                 out.data_ptr(), rows, aid, _stream_ptr(self.device))
        self._check_arg(rc)
        self.last_linear_kernel = rc
        self._keep = (x, weight, bias)
        return out, normed

    def linear_ln_plan(self, name, rows):
        """FLOPE_TF_LIN_SKINNY_LN (6) where linear_ln() would launch for the loaded linear `name` at `rows` rows under the current
        options, otherwise the FLOPE_TF_LIN_* id of the linear of the separate form.  Launches nothing."""
        self._linear_dims(name)
        rc = self.lib.flope_tf_linear_ln_plan(self.handle, name.encode(), int(rows))
        self._check_arg(rc)
        return rc

    @property
    def last_ln(self):
        """(launched, folded): the stand-alone LayerNorm launches of the last forward / stream call that ran kernel by kernel, and the
        LayerNorms that ran inside the next linear's launch (option skinny_ln)"""
        a, b = C.c_int(0), C.c_int(0)
        self._check_arg(self.lib.flope_tf_last_ln(self.handle, C.byref(a), C.byref(b)))
        return a.value, b.value

    def layernorm(self, x, weight, bias, out=None):
        """LayerNorm (eps 1e-5, biased variance) of x [rows, model_dim] in the handle's dtype with device float32 weight / bias
        [model_dim], by the kernel a forward launches; its FLOPE_TF_LN_* id is kept in `last_ln_kernel`.  Needs no weights."""
        tdt, d = self._tdt(), self.dims[1]
        if x.device != self.device or weight.device != self.device or bias.device != self.device:
            raise RuntimeError(f"x, weight and bias must live on {self.device}; no CPU path")
        if x.dim() != 2 or x.shape[1] != d or x.dtype != tdt or not x.is_contiguous():
            raise ValueError(f"expected a contiguous {tdt} tensor [rows, {d}], got {x.dtype} {tuple(x.shape)}")
        for t in (weight, bias):
            if tuple(t.shape) != (d,) or t.dtype != torch.float32 or not t.is_contiguous():
                raise ValueError(f"weight and bias must be contiguous float32 [{d}]")
        if out is None:
            out = torch.empty_like(x)
        elif out.shape != x.shape or out.dtype != tdt or out.device != self.device or not out.is_contiguous():
            raise ValueError(f"out must be a contiguous {tdt} tensor {tuple(x.shape)} on {self.device}")
        with torch.cuda.device(self.device):
            rc = self.lib.flope_tf_layernorm(self.handle, x.data_ptr(), out.data_ptr(), weight.data_ptr(), bias.data_ptr(), x.shape[0],
                                             _stream_ptr(self.device))
        self._check_arg(rc)
        self.last_ln_kernel = rc
        self._keep = (x, weight, bias)
        return out

    def open_stream(self, tracks: int, capacity: int, window: int = 0, bias=None, positions: str = "host", max_rows=None) -> "TransformerEncoderStream":
        """A stream state for `tracks` live tracks of up to `capacity` tokens each (TransformerEncoderStream): feed one new token per
        track with step() and get the row a causal forward of the whole track would end with, without running it again;
        extend() appends several tokens per track in one call, with the bits of those steps.
        `window=W` (1 <= W <= capacity): sliding-window attention over a ring cache -- a track is never full, positions are absolute,
        and step() at position t returns row t of enc(track[: t + 1], is_causal=True, window=W), bit for bit with `window_mfma=0`
        (with `window_mfma=1`: in bits where that forward's attention is the generic kernel, within the attention kernels'
        tolerances elsewhere).
        `bias=table`: a distance table, floating [D], [1, D] or [num_heads, D] with D = window, or capacity without
        one -- a relative bias such as `alibi_distances(D, slopes)`; every entry finite.  The query at position p then scores key j
        as its scaled score + table[h][p - j], and step(), extend() and prefill() return, in bits and in every dtype and under every
        option, the rows of enc(x, mask=enc.make_bias(distance_bias(table, L, window))) with `bias_mfma=0` (the option does not reach a
        stream: DESIGN.md 44).  Without it the encoder has no positional
        term and a track's last row does not depend on the order of the poses behind it.
        `positions="device"` (needs `window`): the positions live in device memory and the state is stepped by an
        association only the device knows -- `step_tracker(tracker)` behind a DeviceTracker's update, or `step_assoc(x, assoc)` --
        without a host wait; `max_rows` (default: max_tokens) is the most rows one call takes.  step(), extend() and
        prefill() are not offered on such a state."""
        return TransformerEncoderStream(self, tracks, capacity, window, bias, positions, max_rows)

    def close(self):
        if getattr(self, "handle", None) and self.handle.value:
            self.lib.flope_tf_destroy(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class TransformerEncoderMask:
    """An [L, L] attention mask compiled for one encoder (include/flope_amd.h: flope_tf_mask_*): the allowed (query, key)
    pairs as bits on the device, made once by `enc.make_mask(mask)` and passed as `mask=` to any number of forwards.  `L`: the
    sequence length it was made for; `allowed`: the number of allowed pairs; `planes`: 0, or the 1 or num_heads float32 planes of an
    additive bias when it was made by `enc.make_bias(bias)` (attention then runs the BIASED instantiation of tf_attn_masked); `tile_stats`: what option `mask_mfma` walks,
    a dict of query_blocks (of 128 rows), blocks_listed (64-key blocks over all of them) and steps_none / steps_some / steps_all (the 8
    (wave, 32-key step) tiles of every listed block by class).  It keeps its encoder alive; after enc.close() or its own
    close() its use raises RuntimeError."""

    def __init__(self, enc: TransformerEncoder, mask, bias=None):
        self.enc = enc
        self.handle = C.c_void_p()
        if not enc.handle.value:
            raise RuntimeError("the encoder of this mask has been closed")
        if bias is not None:
            # a compiled additive bias (make_bias): the same handle type, its allowed set derived from the -inf entries
            # and every refusal made on the C side, which names (plane, row, col)
            bias = torch.as_tensor(bias)
            if bias.dim() not in (2, 3) or bias.shape[-1] != bias.shape[-2] or bias.shape[-1] < 1 or not bias.dtype.is_floating_point:
                raise ValueError(f"bias must be a floating tensor [L, L] or [H, L, L] with L >= 1, got {bias.dtype} {tuple(bias.shape)}")
            b = bias.detach().to(device="cpu", dtype=torch.float32).reshape(-1, bias.shape[-1], bias.shape[-1]).contiguous()
            self.L = int(b.shape[-1])
            with torch.cuda.device(enc.device):
                rc = enc.lib.flope_tf_bias_create(enc.handle, self.L, int(b.shape[0]), C.cast(b.data_ptr(), C.POINTER(C.c_float)), C.byref(self.handle))
            enc._check_arg(rc)
        else:
            allowed = _mask_allowed(mask)
            self.L = int(allowed.shape[0])
            empty = (~allowed.any(dim=1)).nonzero().reshape(-1).tolist()
            if empty:
                raise ValueError(f"mask row {empty[0]} has no allowed key: a softmax over nothing (the reference returns NaN for it)")
            with torch.cuda.device(enc.device):
                rc = enc.lib.flope_tf_mask_create(enc.handle, self.L, _pack_allowed(allowed), C.byref(self.handle))
            enc._check_arg(rc)
        self.planes = int(enc.lib.flope_tf_mask_bias_planes(self.handle))        # 0: a plain mask; 1 or num_heads: a bias
        n, pairs = C.c_int(), C.c_longlong()
        enc._check_arg(enc.lib.flope_tf_mask_info(self.handle, C.byref(n), C.byref(pairs)))
        self.allowed = int(pairs.value)
        qb, st = C.c_int(), [C.c_longlong() for _ in range(4)]
        enc._check_arg(enc.lib.flope_tf_mask_tiles(self.handle, C.byref(qb), *[C.byref(v) for v in st]))
        self.tile_stats = dict(zip(("query_blocks", "blocks_listed", "steps_none", "steps_some", "steps_all"), [int(qb.value)] + [int(v.value) for v in st]))

    def _live(self):
        if not self.enc.handle.value:
            raise RuntimeError("the encoder of this mask has been closed")
        if not self.handle.value:
            raise RuntimeError("the mask has been closed")

    def close(self):
        if getattr(self, "handle", None) and self.handle.value:
            self.enc.lib.flope_tf_mask_destroy(self.handle)      # after enc.close() this frees the host part only
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _host_tracks(tracks):
    """tracks (None, a sequence or a CPU integer tensor) -> (count or None, a ctypes int array or None)"""
    if tracks is None:
        return None, None
    if isinstance(tracks, torch.Tensor):
        if tracks.is_cuda or tracks.dtype.is_floating_point or tracks.dtype == torch.bool:
            raise ValueError("tracks must be a sequence or a CPU integer tensor (positions are kept on the host)")
        tracks = tracks.reshape(-1).tolist()
    vals = [int(v) for v in tracks]
    if any(v < -2 ** 31 or v >= 2 ** 31 for v in vals):
        raise ValueError("a track index does not fit an int")
    return len(vals), (C.c_int * len(vals))(*vals)


class TransformerEncoderStream:
    """The encoder run live over `tracks` tracks (include/flope_amd.h: flope_tf_stream_*).  The state keeps every
    layer's keys and values of each track's tokens so far, up to `capacity` per track, and the number of tokens each track holds
    (`positions`).  step() takes one new token per track and returns the encoder's output for it: the row enc(track, is_causal=True)
    would end with -- in bits where that forward's attention runs the generic kernel, within the attention kernels' tolerances
    elsewhere.  prefill() loads whole histories in one causal forward.  extend() appends several tokens per track behind what the
    track holds, in one ragged launch sequence: its rows and the cache it leaves are, in bits, those of the same tokens
    fed by step() one at a time, in every dtype, on linear and windowed states alike.  The calls on one state run on the current stream in
    program order; keep them on one stream.  The state keeps its encoder alive; after enc.close() its calls raise RuntimeError.
    With `window` = W >= 1 (1 <= W <= capacity, ValueError outside) the cache is a ring and the state is never full:
    positions are absolute and unbounded, the token at position t attends to positions max(0, t + 1 - W) .. t, and step() returns row
    t of enc(track[: t + 1], is_causal=True, window=W), alone or behind a prefill(), for any capacity >= W -- with `window_mfma=0`
    in bits for every dtype; on an encoder made with `window_mfma=1` in bits where that forward's attention is the generic kernel,
    within the attention kernels' tolerances elsewhere (step() itself is always the generic order).
    prefill() is then enc(x, lengths=lengths, is_causal=True, window=W) in bits under either value, takes sequences longer than
    `capacity` (the ring keeps their last `capacity` tokens) and leaves the tracks at their lengths.
    On an encoder with option `step_split` = 1 (`enc.set_option("step_split", v)` may flip it between calls) step() and
    extend() run the split-key attention kernel where `step_plan` says "split": their rows are then no longer the causal forward's
    bits but a deterministic function of the track's own keys, element-wise within a derived bound of fp64, and everything above that
    is stated in bits among step(), extend(), ring capacities and the other tracks of a call still holds in bits.  prefill() and the
    forwards are untouched by it.
    On a 16-bit encoder with option `extend_mfma` = 1 (it may be flipped between calls too) extend() runs its attention on
    the MFMA step where `extend_plan()` says "mfma" (head_dim 32 / 64 / 96 / 128): its rows are then, in bits, the rows of
    enc(track, is_causal=True[, window=W]) where that forward's attention is an MFMA kernel, whatever the split into chunks, and the
    cache it leaves is prefill()'s.  It wins over `step_split` for extend() alone; step(), prefill() and the forwards do not read it.
    With `bias` (`enc.open_stream(..., bias=table)`) the state carries a distance table [planes, D], planes = 1 or
    num_heads (`bias_planes`; 0 without one), D = window or capacity: step(), extend() and prefill() add table[h][p - j] to the scaled
    score of query p and key j and return the rows of the forward under enc.make_bias(distance_bias(table, L, window)) in bits, in
    every dtype and whatever `attn_tiled`, `step_split` or `extend_mfma` say -- `step_plan` / `extend_plan()` answer "biased"."""

    def __init__(self, enc: TransformerEncoder, tracks: int, capacity: int, window: int = 0, bias=None, positions: str = "host", max_rows=None):
        self.enc = enc
        self.state = C.c_void_p()
        self.tracks, self.capacity, self.window = int(tracks), int(capacity), int(window)
        self.last_attn_kernel = None             # FLOPE_TF_STEP_* id of the last attention() launch, FLOPE_TF_EXTEND_* of the last attention_extend()
        self._handle()
        if self.window < 0:
            raise ValueError(f"window must be 0 (a linear cache) or 1 .. capacity, got {self.window}")
        if positions not in ("host", "device"):
            raise ValueError(f"positions must be 'host' or 'device', got {positions!r}")
        self.positions_on = positions
        self.max_rows = 0
        if positions == "host" and max_rows is not None:
            raise ValueError("max_rows belongs to positions='device'")
        if positions == "device":
            self.max_rows = enc.max_tokens if max_rows is None else int(max_rows)
        self.bias_planes = 0
        if bias is not None:
            # every refusal of the table's contents is made on the C side, which names (plane, distance)
            if not isinstance(bias, torch.Tensor) or bias.dim() not in (1, 2) or not bias.dtype.is_floating_point or bias.shape[-1] < 1:
                what = f"{bias.dtype} {tuple(bias.shape)}" if isinstance(bias, torch.Tensor) else type(bias).__name__
                raise ValueError(f"bias must be a floating tensor [D], [1, D] or [{enc.dims[3]}, D], got {what}")
            if bias.is_cuda and bias.device != enc.device:
                raise ValueError(f"bias lives on {bias.device}, the encoder on {enc.device}")
            t = bias.detach().to(device="cpu", dtype=torch.float32).reshape(-1, bias.shape[-1]).contiguous()
            with torch.cuda.device(enc.device):
                if positions == "device":
                    rc = enc.lib.flope_tf_stream_open_device(enc.handle, self.tracks, self.capacity, self.window, self.max_rows, int(t.shape[0]),
                                                             int(t.shape[1]), C.cast(t.data_ptr(), C.POINTER(C.c_float)), C.byref(self.state))
                else:
                    rc = enc.lib.flope_tf_stream_open_bias(enc.handle, self.tracks, self.capacity, self.window, int(t.shape[0]), int(t.shape[1]),
                                                           C.cast(t.data_ptr(), C.POINTER(C.c_float)), C.byref(self.state))
            enc._check_arg(rc)
            self.bias_planes = int(enc.lib.flope_tf_stream_bias_planes(self.state))
            return
        with torch.cuda.device(enc.device):
            if positions == "device":
                rc = enc.lib.flope_tf_stream_open_device(enc.handle, self.tracks, self.capacity, self.window, self.max_rows, 0, 0, None, C.byref(self.state))
            elif self.window:
                rc = enc.lib.flope_tf_stream_open_window(enc.handle, self.tracks, self.capacity, self.window, C.byref(self.state))
            else:
                rc = enc.lib.flope_tf_stream_open(enc.handle, self.tracks, self.capacity, C.byref(self.state))
        enc._check_arg(rc)

    def _handle(self):
        if not self.enc.handle.value:
            raise RuntimeError("the encoder of this stream has been closed")

    def _live(self):
        self._handle()
        if not self.state.value:
            raise RuntimeError("the stream has been closed")

    def _check_x(self, x, dims):
        enc = self.enc
        if not x.is_cuda or x.device != enc.device:
            raise RuntimeError(f"input must live on {enc.device} (got {x.device}); no CPU path")
        if x.dim() != dims or x.shape[-1] != enc.dims[0]:
            want = "[n, L, {}]" if dims == 3 else "[n, {}]"
            raise ValueError(f"expected {want.format(enc.dims[0])}, got {tuple(x.shape)}")
        return x.to(torch.float32).contiguous()

    def step(self, x: torch.Tensor, tracks=None, out: torch.Tensor = None) -> torch.Tensor:
        """x [n, input_dim]: row r is the next token of track tracks[r] (None: n == the state's track count, row r is track r) ->
        [n, out_dim].  Tracks must be distinct and none at capacity (ValueError names the offending row; nothing has moved then);
        a windowed state has no such limit.
        `out`: a float32 [n, out_dim] tensor with contiguous rows to write into."""
        self._live()
        enc = self.enc
        x = self._check_x(x, 2)
        n = x.shape[0]
        cnt, th = _host_tracks(tracks)
        if cnt is not None and cnt != n:
            raise ValueError(f"tracks has {cnt} values for {n} rows")
        y = self._out(out, (n, enc.dims[2]))
        with torch.cuda.device(enc.device):
            rc = enc.lib.flope_tf_stream_step(self.state, x.data_ptr(), n, th, y.data_ptr(), _stream_ptr(enc.device))
        enc._check_arg(rc)
        self._keep = x
        return y

    def prefill(self, x: torch.Tensor, lengths=None, tracks=None, out: torch.Tensor = None) -> torch.Tensor:
        """x [n, L, input_dim], sequence b the history of track tracks[b] (None as in step), `lengths` as in forward() -> the causal
        forward enc(x, lengths=lengths, is_causal=True) [n, L, out_dim], bit for bit; the tracks then hold their lengths' tokens
        (whatever they held before is overwritten) and the next step() continues them.  A windowed state: the forward is the one
        with window=W, and L may exceed the capacity."""
        self._live()
        enc = self.enc
        x = self._check_x(x, 3)
        n, L = x.shape[0], x.shape[1]
        cnt, th = _host_tracks(tracks)
        if cnt is not None and cnt != n:
            raise ValueError(f"tracks has {cnt} values for {n} sequences")
        lh = None if lengths is None else _host_lengths(lengths, n)
        y = self._out(out, (n, L, enc.dims[2]))
        with torch.cuda.device(enc.device):
            rc = enc.lib.flope_tf_stream_prefill(self.state, x.data_ptr(), n, L, lh, th, y.data_ptr(), _stream_ptr(enc.device))
        enc._check_arg(rc)
        self._keep = x
        return y

    def extend(self, x: torch.Tensor, lengths=None, tracks=None, out: torch.Tensor = None) -> torch.Tensor:
        """Appends several tokens per track in one call.  x [n, L, input_dim], sequence b the NEXT lengths[b] tokens
        (1 .. L, right-padded; None: all L) of track tracks[b] (None as in step), behind whatever the track holds -> [n, L, out_dim]:
        row i of sequence b is what step() would return for that token, bit for bit in every dtype and under every option, and the
        tracks end as the same steps would leave them, so any split of a track into extend() / step() calls gives the same bits.
        Rows behind a length are out_layer.bias.  Tracks must be distinct; on a linear state position + length must stay within the
        capacity (ValueError names the offending index; nothing has moved then), a windowed state takes chunks of any length (the
        ring keeps the last `capacity` tokens).
        `out`: a float32 [n, L, out_dim] contiguous tensor to write into."""
        self._live()
        enc = self.enc
        x = self._check_x(x, 3)
        n, L = x.shape[0], x.shape[1]
        cnt, th = _host_tracks(tracks)
        if cnt is not None and cnt != n:
            raise ValueError(f"tracks has {cnt} values for {n} sequences")
        lh = None if lengths is None else _host_lengths(lengths, n)
        y = self._out(out, (n, L, enc.dims[2]))
        with torch.cuda.device(enc.device):
            rc = enc.lib.flope_tf_stream_extend(self.state, x.data_ptr(), n, L, lh, th, y.data_ptr(), _stream_ptr(enc.device))
        enc._check_arg(rc)
        self._keep = x
        return y

    @property
    def step_plan(self) -> str:
        """"row", "split" or "biased": the attention kernel a step() / extend() of this state would launch now -- "split" under the
        encoder's option `step_split` where the head slice is a power-of-two count of 16-byte vectors, "biased" on a
        state with a distance table, whatever the options.  Enqueues nothing."""
        self._live()
        rc = self.enc.lib.flope_tf_stream_step_plan(self.state)
        self.enc._check_arg(rc)
        return {_lib.TF_STEP_SPLIT: "split", _lib.TF_STEP_BIASED: "biased"}.get(rc, "row")

    def attention(self, qkv: torch.Tensor, lengths=None, out: torch.Tensor = None) -> torch.Tensor:
        """A test hook: the attention launch of step() alone, on a caller's tensor.  qkv [n, L, 3 * model_dim] in the handle's dtype
        -> [n, model_dim]: row b is what step()'s attention writes for a token whose q | k | v is row lengths[b] - 1 (None: L - 1) of
        sequence b, on a track that holds the k | v columns of the rows in front of it (a windowed state: the ring keeps the last
        `capacity` of them), by the kernel step() would run now; its id is kept in `last_attn_kernel` (0 row, 1 split).  It
        overwrites layer 0's cache rows of tracks 0 .. n - 1 and leaves those tracks at position 0.  Needs no weights.
        ValueError: n outside 1 .. tracks, a length outside 1 .. L or, on a linear state, above the capacity."""
        self._live()
        enc = self.enc
        tdt, d = enc._tdt(), enc.dims[1]
        if not qkv.is_cuda or qkv.device != enc.device:
            raise RuntimeError(f"input must live on {enc.device} (got {qkv.device}); no CPU path")
        if qkv.dim() != 3 or qkv.shape[2] != 3 * d or qkv.dtype != tdt or not qkv.is_contiguous():
            raise ValueError(f"expected a contiguous {tdt} tensor [n, L, {3 * d}], got {qkv.dtype} {tuple(qkv.shape)}")
        n, L = qkv.shape[0], qkv.shape[1]
        lh = None if lengths is None else _host_lengths(lengths, n)
        if out is None:
            out = torch.empty((n, d), dtype=tdt, device=enc.device)
        elif tuple(out.shape) != (n, d) or out.dtype != tdt or out.device != enc.device or not out.is_contiguous():
            raise ValueError(f"out must be a contiguous {tdt} tensor {(n, d)} on {enc.device}")
        with torch.cuda.device(enc.device):
            rc = enc.lib.flope_tf_stream_attention(self.state, qkv.data_ptr(), n, L, lh, out.data_ptr(), _stream_ptr(enc.device))
        enc._check_arg(rc)
        self.last_attn_kernel = rc
        self._keep = qkv
        return out

    def extend_plan(self) -> str:
        """"row", "split" or "mfma": the attention kernel an extend() of this state would launch now -- "mfma" under the encoder's option
        `extend_mfma` on a 16-bit handle with head_dim 32 / 64 / 96 / 128, otherwise what `step_plan` says ("biased" on a
        state with a distance table, in front of every option).  Enqueues nothing."""
        self._live()
        rc = self.enc.lib.flope_tf_stream_extend_plan(self.state)
        self.enc._check_arg(rc)
        return {_lib.TF_EXTEND_MFMA: "mfma", _lib.TF_EXTEND_SPLIT: "split", _lib.TF_EXTEND_BIASED: "biased"}.get(rc, "row")

    def attention_extend(self, qkv: torch.Tensor, lengths, cached, out: torch.Tensor = None) -> torch.Tensor:
        """A test hook: the attention launch of extend() alone, on a caller's tensor.  qkv [n, L, 3 * model_dim] in the handle's dtype
        -> [n, L, model_dim]: of sequence b, rows 0 .. cached[b] - 1 are loaded into track b as its history (k | v columns; a windowed
        state: the ring keeps the last `capacity` of them), rows cached[b] .. lengths[b] - 1 are the chunk, and those rows of the
        result are what extend()'s attention writes for them, by the kernel extend() would run now; its id is kept in
        `last_attn_kernel` (0 row, 1 split, 2 mfma).  Every other row of `out` is left as it is (a fresh result: zeros).  It
        overwrites layer 0's cache rows of tracks 0 .. n - 1 and leaves those tracks at position 0.  Needs no weights.
        ValueError: n outside 1 .. tracks, a length outside 1 .. L or, on a linear state, above the capacity, cached[b] outside
        0 .. lengths[b] - 1, chunks of more than max_tokens rows together."""
        self._live()
        enc = self.enc
        tdt, d = enc._tdt(), enc.dims[1]
        if not qkv.is_cuda or qkv.device != enc.device:
            raise RuntimeError(f"input must live on {enc.device} (got {qkv.device}); no CPU path")
        if qkv.dim() != 3 or qkv.shape[2] != 3 * d or qkv.dtype != tdt or not qkv.is_contiguous():
            raise ValueError(f"expected a contiguous {tdt} tensor [n, L, {3 * d}], got {qkv.dtype} {tuple(qkv.shape)}")
        n, L = qkv.shape[0], qkv.shape[1]
        lh, ch = _host_lengths(lengths, n), _host_lengths(cached, n)
        if out is None:
            out = torch.zeros((n, L, d), dtype=tdt, device=enc.device)
        elif tuple(out.shape) != (n, L, d) or out.dtype != tdt or out.device != enc.device or not out.is_contiguous():
            raise ValueError(f"out must be a contiguous {tdt} tensor {(n, L, d)} on {enc.device}")
        with torch.cuda.device(enc.device):
            rc = enc.lib.flope_tf_stream_attention_extend(self.state, qkv.data_ptr(), n, L, lh, ch, out.data_ptr(), _stream_ptr(enc.device))
        enc._check_arg(rc)
        self.last_attn_kernel = rc
        self._keep = qkv
        return out

    def _out(self, out, shape):
        if out is None:
            return torch.empty(shape, dtype=torch.float32, device=self.enc.device)
        if tuple(out.shape) != tuple(shape) or out.dtype != torch.float32 or out.device != self.enc.device or not out.is_contiguous():
            raise ValueError(f"out must be a contiguous float32 tensor {tuple(shape)} on {self.enc.device}")
        return out

    def step_assoc(self, x: torch.Tensor, assoc: torch.Tensor, overflow: torch.Tensor = None, out: torch.Tensor = None) -> torch.Tensor:
        """A device-positioned state.  x [n, input_dim] float32 and assoc int32 [n] on the device: assoc[m] >= 0 names
        the track row m belongs to, a negative value -1 - t the track t it opened, INT32_MIN a row to skip (a DeviceTracker's
        encoding); `overflow`: an int32 tensor of one element on the device, non-zero = every row is refused.  -> [n, out_dim]: the
        row step() would return for each row that feeds its track (the first row of the call that names the track, a track below
        `tracks`), out_layer.bias for the others -- `last_feed()` tells which.  No host wait.  n = 0 returns an empty result."""
        self._live()
        enc = self.enc
        x = self._check_x(x, 2)
        n = x.shape[0]
        if not (isinstance(assoc, torch.Tensor) and assoc.device == enc.device and assoc.dtype == torch.int32 and assoc.is_contiguous() and assoc.numel() == n):
            raise ValueError(f"assoc must be a contiguous int32 tensor [{n}] on {enc.device}")
        if overflow is not None and not (isinstance(overflow, torch.Tensor) and overflow.device == enc.device and overflow.dtype == torch.int32 and
                                         overflow.numel() == 1):
            raise ValueError(f"overflow must be an int32 tensor of one element on {enc.device}")
        y = self._out(out, (n, enc.dims[2]))
        with torch.cuda.device(enc.device):
            rc = enc.lib.flope_tf_stream_step_assoc(self.state, x.data_ptr(), assoc.data_ptr(), None if overflow is None else overflow.data_ptr(), n,
                                                    y.data_ptr(), _stream_ptr(enc.device))
        enc._check_arg(rc)
        self._keep = (x, assoc, overflow)
        return y

    def step_tracker(self, tracker, source: str = "measurement", out: torch.Tensor = None) -> torch.Tensor:
        """A device-positioned state, right behind `tracker.update(...)` on the same stream: one token for every
        track the update touched, taken on the device from the tracker's last frame -- source "measurement": the row's measurement
        [x y z | qx qy qz qw] in the world frame; "mean": its track's filtered mean after the frame -- rounded to float32, zeros
        behind column 6.  -> [n, out_dim], n the frame's measurements: row m is the encoder's row for measurement m where it feeds
        its track (the first measurement of the frame on a track below `tracks`), out_layer.bias elsewhere; `last_feed()` tells
        which.  No host wait.  RuntimeError: the same update fed twice, or no update since the tracker was made or reset."""
        self._live()
        enc = self.enc
        if source not in ("measurement", "mean"):
            raise ValueError(f"source must be 'measurement' or 'mean', got {source!r}")
        n = int(tracker.last_n)
        if n < 0:
            n = 0                                  # (the call refuses it with the reason)
        y = self._out(out, (n, enc.dims[2]))
        with torch.cuda.device(enc.device):
            rc = enc.lib.flope_tf_stream_step_tracker(self.state, tracker.handle, _lib.TF_FEED_MEAN if source == "mean" else _lib.TF_FEED_MEAS,
                                                      y.data_ptr() if n else None, _stream_ptr(enc.device))
        enc._check_arg(rc)
        return y

    def last_feed(self):
        """-> (tracks_or_codes int32 [n], positions int32 [n]) of the last step_assoc() / step_tracker(): per row the track it fed and
        the position its token took, or a negative code (_lib.TF_FEED_*) and 0.  Waits for that call."""
        self._live()
        t, p = np.empty(max(self.max_rows, 1), dtype=np.int32), np.empty(max(self.max_rows, 1), dtype=np.int32)
        n = self.enc.lib.flope_tf_stream_read_feed(self.state, t.ctypes.data, p.ctypes.data, len(t))
        self.enc._check_arg(n)
        return t[:n].copy(), p[:n].copy()

    def last_tokens(self) -> np.ndarray:
        """test hook: the float32 token rows [n, input_dim] the last step_assoc() / step_tracker() ran on.  Waits for that call."""
        self._live()
        tok = np.empty((max(self.max_rows, 1), self.enc.dims[0]), dtype=np.float32)
        n = self.enc.lib.flope_tf_stream_read_tokens(self.state, tok.ctypes.data, len(tok))
        self.enc._check_arg(n)
        return tok[:n].copy()

    def reset(self, tracks=None) -> None:
        """The given tracks (None: all) hold nothing again; their stale cache rows are never read.  Enqueues nothing; a
        device-positioned state resets all its tracks, by a memset on the current stream."""
        self._live()
        if self.max_rows:
            if tracks is not None:
                raise ValueError("a device-positioned state resets all its tracks: reset()")
            with torch.cuda.device(self.enc.device):
                self.enc._check_arg(self.enc.lib.flope_tf_stream_reset_device(self.state, _stream_ptr(self.enc.device)))
            return
        cnt, th = _host_tracks(tracks)
        self.enc._check_arg(self.enc.lib.flope_tf_stream_reset(self.state, cnt or 0, th))

    def position(self, track: int) -> int:
        """tokens track `track` holds"""
        self._live()
        rc = self.enc.lib.flope_tf_stream_position(self.state, int(track))
        self.enc._check_arg(rc)
        return rc

    @property
    def positions(self) -> list:
        """tokens held per track; a device-positioned state reads them back (and waits for its last call)"""
        if self.max_rows:
            self._live()
            pos = np.empty(self.tracks, dtype=np.int32)
            self.enc._check_arg(self.enc.lib.flope_tf_stream_read_positions(self.state, pos.ctypes.data, self.tracks))
            return pos.tolist()
        return [self.position(t) for t in range(self.tracks)]

    def close(self):
        if getattr(self, "state", None) and self.state.value:
            self.enc.lib.flope_tf_stream_close(self.state)      # after enc.close() this frees the host part only: the cache went with the handle
            self.state = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
