"""Element-wise checker of the encoder's linear and LayerNorm launches (tf_gemm_mfma, tf_linear_f32m, tf_linear_generic,
tf_linear_rowwave, tf_linear_rowwave_vec, tf_layernorm, tf_layernorm_vec in flope_amd/csrc/tf_encoder.hip): the fp64 reference
computed from the values the device is fed, a bound for every output element, the test shapes and inputs, and a float32 emulation
of each operation that can be broken the way kernels break.  Helper of tests/test_tf_linear_bound.py (CPU: the bound passes the
emulation in three summation orders and fails its broken copies) and tests/test_gpu_tf_ops.py (the device output, through
flope_tf_linear / flope_tf_layernorm).

Linear (the bound of oracle/conv_bound.py, with its constants; K = in_features, T = the type the output is stored in):

    ref   = act(x W^T + b + r)                         fp64
    mag   = |x| |W|^T + |b| + |r|                      fp64
    bound = u |ref| + (K + 2) 2^-23 mag + tiny         u = 2^-11 (f16), 2^-8 (bf16), 2^-24 (float32 output)

  u |ref|            the one round-to-nearest of the store;
  (K + 2) 2^-23 mag  K products, the bias and the residual summed in float32 IN ANY ORDER, one ulp (not half) per addition so that
                     neither the matrix unit's accumulator rounding nor a separately rounded product (float32 x float32 inputs
                     without a fused multiply-add) can exceed it;
  tiny               one smallest subnormal of T (a ReLU'd value next to zero).
  x and r are the exact values the device is fed (16-bit values widened; a float32 network input that tf_cast_pad rounds to 16 bits
  in front of tf_gemm_mfma enters as that rounded value).  W is what the kernel multiplies by: the checkpoint weight rounded once to
  the handle's type for tf_gemm_mfma (pack_linear), the float32 weight for every other kernel.  |relu(a) - relu(b)| <= |a - b|, so
  the ReLU needs no term.

LayerNorm over d features, from the stored row x in fp64: mu = mean(x), var = mean((x - mu)^2) (biased), r = 1 / sqrt(var + 1e-5),

    ref_c   = (x_c - mu) r w_c + b_c
    bound_c = u |ref_c| + (d + 8) 2^-23 (|x_c - mu| + mean_j |x_j|) r |w_c| + 2^-23 |b_c| + tiny

  What the kernels do in float32 (v = 2^-24), and what each step costs:
  1. mean: d values summed in any order and one division: |mu~ - mu| <= (d + 1) v mean|x| =: dm.  It shifts every x_c - mu~ by the
     same dm, which the factor r |w_c| carries to the output: the mean|x| term.  It is what matters on rows with almost no variance
     (|x_c - mu| -> 0, r -> 1 / sqrt(eps) = 316) and on rows with a large common offset (mean|x| >> |x_c - mu|).
  2. t_c = x_c - mu~ rounds once: v |t_c|.
  3. variance: mean(t~^2) = var + dm^2 exactly, plus d products and d - 1 additions of positive terms, one division, one addition
     of eps: relative (d + 3) v of var + eps; r = 1 / sqrt(.) halves it and adds a square root and a division at one v each.
     dm^2 <= ((d + 1) v mean|x|)^2 is second order (1e-8 of eps at d = 2056 and an offset of 100).
     Relative error of r~: ((d + 3) / 2 + 2) v, carried by |x_c - mu| r |w_c|: the |x_c - mu| term.
  4. (t~ r~) w_c + b_c: three more roundings, the last one of the whole value: v (|ref_c - b_c| + |b_c|).
  Sum: ((d + 3) / 2 + 6) v |x_c - mu| r |w_c| + (d + 1) v mean|x| r |w_c| + v |b_c|  <=  the bound's terms, which spend the same
  factor 2 per rounding as the linear's (one ulp, not half) and round the two counts up to one (d + 8).
  The exactly constant row has var = 0 in fp64 and ref = b; the device's t~ is dm-sized and r = 316: inside the mean|x| term.

Nothing is fitted to an output.  The emulations replay float32 arithmetic (products and sums rounded to float32 after every
operation, one store) in three summation orders -- sequential, pairwise, and 64 strided lanes then a butterfly, the order of the
wave kernels -- and must stay inside the bound on every case below; their worst err / bound is printed by the CPU test and recorded
in DESIGN.md 20.
"""
import functools

import numpy as np
import torch

from oracle import conv_bound as CB
from oracle import tf_encoder_ref as T

TDT = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32, "f32m": torch.float32}
U = {k: CB.UNIT_ROUNDOFF[v] for k, v in TDT.items()}
TINY = {k: CB.TINY[v] for k, v in TDT.items()}
ACC = 2.0 ** -23                     # one float32 ulp per addition (oracle/conv_bound.py)
LN_EPS = 1e-5
ORDERS = ["seq", "pairwise", "lanes64"]

GENERIC, ROWWAVE, ROWWAVE_VEC, MFMA, F32M = 0, 1, 2, 3, 4          # FLOPE_TF_LIN_* of include/flope_amd.h
LN_SCALAR, LN_VEC = 0, 1                                            # FLOPE_TF_LN_*

# handles: (input_dim, model_dim, out_dim, heads, layers, ff_dim)
A = (24, 128, 9, 2, 1, 256)
B = (70, 192, 5, 3, 1, 384)
C = (16, 8, 9, 1, 0, 8)
D_VEC, D_ROW, D_16, D_16R = (8, 1360, 9, 1, 0, 8), (8, 1368, 9, 1, 0, 8), (8, 768, 16, 1, 0, 8), (8, 1360, 16, 1, 0, 8)
F1, F2 = (20, 72, 9, 6, 1, 100), (24, 384, 9, 6, 1, 1536)
A_ROWS = (1, 127, 128, 129, 250)


def _case(dims, name, rows, kernel, relu=False, res=False, x_f32=False, out_f32=False, generic=0):
    return dict(dims=dims, name=name, rows=rows, kernel=kernel, relu=relu, res=res, x_f32=x_f32, out_f32=out_f32, generic=generic)


def linear_cases(dtype):
    """Every linear launch the device test makes on a handle of `dtype`, with the FLOPE_TF_LIN_* id it must report."""
    cs = []
    if dtype in ("f16", "bf16"):
        for r in A_ROWS:
            cs += [_case(A, "embedding", r, MFMA, x_f32=True),                 # Kp = 64 behind tf_cast_pad's zero columns
                   _case(A, "layers.0.in_proj", r, MFMA),                      # two k chunks: both LDS buffers
                   _case(A, "layers.0.out_proj", r, MFMA, res=True),
                   _case(A, "layers.0.out_proj", r, MFMA, relu=True, res=True),  # (no forward launches this form; the kernel has it)
                   _case(A, "layers.0.linear1", r, MFMA, relu=True),
                   _case(A, "layers.0.linear2", r, MFMA, res=True),            # four k chunks: the ring reused
                   _case(A, "out_layer", r, ROWWAVE_VEC, out_f32=True)]
        cs.append(_case(A, "layers.0.in_proj", 1100, MFMA))                    # 27 workgroups: not a multiple of the 8 XCDs
        for g in (0, 1):
            for r in (1, 33):
                cs += [_case(B, "layers.0.linear1", r, GENERIC if g else MFMA, relu=True, generic=g),    # three k chunks
                       _case(B, "embedding", r, GENERIC, x_f32=True, generic=g),
                       _case(B, "layers.0.in_proj", r, GENERIC, generic=g),
                       _case(B, "layers.0.in_proj", r, GENERIC, x_f32=True, generic=g),
                       _case(B, "layers.0.out_proj", r, GENERIC, res=True, generic=g),
                       _case(B, "layers.0.out_proj", r, GENERIC, relu=True, res=True, generic=g),
                       _case(B, "layers.0.linear2", r, GENERIC, res=True, generic=g),
                       _case(B, "out_layer", r, ROWWAVE_VEC, out_f32=True, generic=g)]
        cs += [_case(C, "embedding", 33000, ROWWAVE, x_f32=True),              # 8192 blocks x 4 rows: a second grid-stride pass
               _case(C, "out_layer", 33000, ROWWAVE_VEC, out_f32=True),        # 2048 blocks x 8 rows: a third pass
               _case(D_VEC, "out_layer", 5, ROWWAVE_VEC, out_f32=True),        # 48960 bytes of LDS
               _case(D_ROW, "out_layer", 5, ROWWAVE, out_f32=True),            # 49248 > 49152
               _case(D_16, "out_layer", 5, ROWWAVE_VEC, out_f32=True),         # all 16 accumulators, exactly 49152 bytes
               _case(D_16R, "out_layer", 5, ROWWAVE, out_f32=True)]            # all 16 accumulators of the scalar form
    elif dtype == "f32m":
        for dims in (F1, F2):
            for r in (37, 131, 771):
                cs += [_case(dims, "embedding", r, F32M), _case(dims, "layers.0.in_proj", r, F32M),
                       _case(dims, "layers.0.out_proj", r, F32M, res=True), _case(dims, "layers.0.linear1", r, F32M, relu=True),
                       _case(dims, "layers.0.linear2", r, F32M, res=True), _case(dims, "out_layer", r, F32M)]
    else:
        for r in (37, 131):
            cs += [_case(F1, "embedding", r, GENERIC), _case(F1, "layers.0.in_proj", r, GENERIC),
                   _case(F1, "layers.0.out_proj", r, GENERIC, res=True), _case(F1, "layers.0.out_proj", r, GENERIC, relu=True, res=True),
                   _case(F1, "layers.0.linear1", r, GENERIC, relu=True), _case(F1, "layers.0.linear2", r, GENERIC, res=True),
                   _case(F1, "out_layer", r, ROWWAVE)]
        cs += [_case(C, "embedding", 33000, ROWWAVE), _case(C, "out_layer", 33000, ROWWAVE)]
    return cs


def case_id(c):
    return "%s-%s-r%d%s%s%s%s%s" % ("x".join(str(v) for v in c["dims"]), c["name"], c["rows"], "-relu" if c["relu"] else "", "-res" if c["res"] else "",
                                    "-xf32" if c["x_f32"] else "", "-yf32" if c["out_f32"] else "", "-generic" if c["generic"] else "")


# ---- weights and inputs ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def state_dict(dims):
    """oracle.tf_encoder_ref.synthetic_state_dict(seed 5) rounded to float32, as TransformerEncoder.load_state_dict rounds it"""
    sd = T.synthetic_state_dict(dims[0], dims[1], dims[2], dims[4], dims[5], seed=5)
    return {k: torch.from_numpy(np.asarray(v, dtype=np.float32)) for k, v in sd.items()}


def weight_keys(name):
    if name in ("embedding", "out_layer"):
        return name + ".weight", name + ".bias"
    _, i, op = name.split(".")
    p = f"transformer_encoder.layers.{i}."
    return {"in_proj": (p + "self_attn.in_proj_weight", p + "self_attn.in_proj_bias"),
            "out_proj": (p + "self_attn.out_proj.weight", p + "self_attn.out_proj.bias"),
            "linear1": (p + "linear1.weight", p + "linear1.bias"), "linear2": (p + "linear2.weight", p + "linear2.bias")}[op]


def kernel_weight(W, dtype, kernel):
    """The weight the kernel multiplies by: rounded once to the handle's type for tf_gemm_mfma, float32 otherwise."""
    return W.to(TDT[dtype]).float() if kernel == MFMA else W


@functools.lru_cache(maxsize=None)
def linear_inputs(dims, name, rows, dtype, x_f32, res, seed=7):
    """(x, r): x [rows, K] standard normal, float32 where the case feeds float32, else rounded to the handle's type; r [rows, N]
    standard normal in the handle's type, or None."""
    wk, _ = weight_keys(name)
    N, K = state_dict(dims)[wk].shape
    g = torch.Generator().manual_seed(seed * 1000003 + rows * 31 + N * 7 + K)
    x = torch.randn(rows, K, generator=g)
    r = torch.randn(rows, N, generator=g) if res else None
    tdt = TDT[dtype]
    return (x if (x_f32 or tdt == torch.float32) else x.to(tdt)), (None if r is None else r.to(tdt))


def fed(x, dtype, kernel):
    """x as the kernel reads it: a float32 input to tf_gemm_mfma passes tf_cast_pad's one rounding first."""
    return x.to(TDT[dtype]) if (kernel == MFMA and x.dtype == torch.float32) else x


def out_key(c, dtype):
    return "f32" if (c["out_f32"] or dtype in ("f32", "f32m")) else dtype


def linear_reference(x, W, b, r, relu, out):
    """-> (ref, bound) in fp64 [rows, N].  x, r: as fed; W: as multiplied; out: "f16" / "bf16" / "f32", the type stored."""
    xd, Wd, bd = x.double(), W.double(), b.double()
    acc = xd @ Wd.t() + bd
    mag = xd.abs() @ Wd.abs().t() + bd.abs()
    if r is not None:
        acc = acc + r.double()
        mag = mag + r.double().abs()
    ref = torch.relu(acc) if relu else acc
    return ref, U[out] * ref.abs() + (W.shape[1] + 2) * ACC * mag + TINY[out]


@functools.lru_cache(maxsize=None)
def _case_reference(dims, name, rows, dtype, kernel, relu, res, x_f32, out):
    sd = state_dict(dims)
    wk, bk = weight_keys(name)
    x, r = linear_inputs(dims, name, rows, dtype, x_f32, res)
    return linear_reference(fed(x, dtype, kernel), kernel_weight(sd[wk], dtype, kernel), sd[bk], r, relu, out)


def case_reference(c, dtype):
    return _case_reference(c["dims"], c["name"], c["rows"], dtype, c["kernel"], c["relu"], c["res"], c["x_f32"], out_key(c, dtype))


def ratio(got, ref, bound):
    """max over elements of |got - ref| / bound, and where; a non-finite output counts as infinitely wrong"""
    g = got.detach().cpu().double()
    r = (g - ref).abs() / bound
    r = torch.where(torch.isfinite(g), r, torch.full_like(r, float("inf")))
    i = int(r.argmax())
    return float(r.reshape(-1)[i]), tuple(int(t) for t in torch.unravel_index(torch.tensor(i), r.shape))


# ---- float32 emulation --------------------------------------------------------------------------------------------------------------
def fsum(p, order, acc_dtype=torch.float32):
    """Sum of p over its last axis with every partial sum rounded to acc_dtype, in one of ORDERS."""
    p = p.to(acc_dtype)
    n = p.shape[-1]
    if order == "seq":
        s = torch.zeros(p.shape[:-1], dtype=acc_dtype)
        for k in range(n):
            s = s + p[..., k]
        return s
    if order == "pairwise":
        while p.shape[-1] > 1:
            if p.shape[-1] % 2:
                p = torch.cat([p, torch.zeros(p.shape[:-1] + (1,), dtype=acc_dtype)], dim=-1)
            p = p[..., 0::2] + p[..., 1::2]
        return p[..., 0]
    assert order == "lanes64"
    pad = (-n) % 64
    if pad:
        p = torch.cat([p, torch.zeros(p.shape[:-1] + (pad,), dtype=acc_dtype)], dim=-1)
    p = p.reshape(p.shape[:-1] + (-1, 64))
    s = torch.zeros(p.shape[:-2] + (64,), dtype=acc_dtype)
    for i in range(p.shape[-2]):
        s = s + p[..., i, :]
    o = 32
    while o:
        s = s[..., :o] + s[..., o:2 * o]
        o >>= 1
    return s[..., 0]


LINEAR_MUTATIONS = ["dropk", "bias2", "bias16", "resrow", "relu_first", "round2", "acc16", "lastrow"]


def emulate_linear(x, W, b, r, relu, out, order="seq", mutation=None, dtype16="bf16"):
    """act(x W^T + b + r) with float32 products and float32 partial sums, stored once to `out`.  mutation: None, or one defect
         dropk       one 8-wide k chunk dropped for one row (the middle row, the second chunk where there is one)
         bias2       bias added twice                         bias16   bias rounded to 16 bits (dtype16) first
         resrow      residual taken from row m + 1 (the last row wraps)
         relu_first  ReLU applied before the residual         round2   the result rounded to f16 and then to bf16
         acc16       partial sums kept in the 16-bit type dtype16
         lastrow     the last row of a partly filled 128-row tile copied from the row before"""
    xf, Wf, bf = x.float(), W.float(), b.float()
    rows, K = xf.shape
    if mutation == "dropk":
        xf = xf.clone()
        k0 = 8 if K >= 16 else 0
        xf[rows // 2, k0:k0 + 8] = 0.0
    if mutation == "bias16":
        bf = bf.to(TDT[dtype16]).float()
    p = xf[:, None, :] * Wf[None, :, :]                                # [rows, N, K], each product rounded to float32
    if mutation == "acc16":
        acc = fsum(p, "seq", TDT[dtype16]).float()
    else:
        acc = fsum(p, order)
    acc = acc + bf
    if mutation == "bias2":
        acc = acc + bf
    if mutation == "relu_first" and relu:
        acc = torch.relu(acc)
    if r is not None:
        acc = acc + (torch.roll(r, -1, 0) if mutation == "resrow" else r).float()
    if relu and mutation != "relu_first":
        acc = torch.relu(acc)
    if mutation == "round2":
        acc = acc.to(torch.float16).to(torch.bfloat16).float()
    y = acc.to(TDT[out])
    if mutation == "lastrow" and rows % 128 and rows > 1:
        y = y.clone()
        y[rows - 1] = y[rows - 2]
    return y


def mutation_applies(mutation, c):
    if mutation == "resrow":
        return c["res"] and c["rows"] > 1
    if mutation == "relu_first":
        return c["res"] and c["relu"]
    if mutation == "lastrow":
        return c["rows"] % 128 != 0 and c["rows"] > 1
    return True


def cpu_rows(c, budget=6_000_000):
    """Rows of a case the CPU emulation walks: all of them while rows N K stays within `budget` products, else the first
    budget / (N K) (at least 2).  The rows of a linear are independent, so a defect of the arithmetic shows on any of them."""
    wk, _ = weight_keys(c["name"])
    N, K = state_dict(c["dims"])[wk].shape
    return c["rows"] if c["rows"] * N * K <= budget else max(2, budget // (N * K))


# ---- LayerNorm ------------------------------------------------------------------------------------------------------------------------
LN_DIMS = (8, 72, 516, 2048, 2056)
LN_ROWS = (1, 5)
LN_FAMILIES = ["normal", "offset", "lowvar", "constant", "outlier"]
LN_MUTATIONS = ["unbiased", "noeps", "onepass", "swap", "padmean"]


def ln_kernel(d, dtype):
    return LN_VEC if dtype in ("f16", "bf16") and d % 8 == 0 and d <= 2048 else LN_SCALAR


@functools.lru_cache(maxsize=None)
def ln_inputs(family, rows, d, dtype, seed=3):
    """(x [rows, d] in the handle's type, gamma [d], beta [d] float32).  gamma in +-[0.5, 2.5] and beta in [-3, 3]: far from 1 and 0."""
    g = torch.Generator().manual_seed(seed * 1000003 + LN_FAMILIES.index(family) * 7919 + rows * 31 + d)
    n = torch.randn(rows, d, generator=g)
    if family == "normal":
        x = n
    elif family == "offset":                    # a large common offset: a one-pass variance cancels here
        x = 100.0 + n
    elif family == "lowvar":                    # variance near eps
        x = 1.0 + 3e-3 * n
    elif family == "constant":                  # no variance at all
        x = torch.full((rows, d), 0.7) * (1.0 + torch.arange(rows, dtype=torch.float32))[:, None]
    else:                                       # one outlier in a unit row
        x = n.clone()
        x[:, d // 3] = 200.0
    gamma = (0.5 + 2.0 * torch.rand(d, generator=g)) * torch.where(torch.rand(d, generator=g) < 0.5, -1.0, 1.0)
    beta = 6.0 * torch.rand(d, generator=g) - 3.0
    return x.to(TDT[dtype]), gamma, beta


def ln_reference(x, w, b, dtype):
    """-> (ref, bound) in fp64 [rows, d] for the stored rows x."""
    xd, wd, bd = x.double(), w.double(), b.double()
    d = x.shape[1]
    mu = xd.mean(dim=1, keepdim=True)
    var = ((xd - mu) ** 2).mean(dim=1, keepdim=True)
    rs = 1.0 / torch.sqrt(var + LN_EPS)
    ref = (xd - mu) * rs * wd + bd
    bound = (U[dtype] * ref.abs() + (d + 8) * ACC * ((xd - mu).abs() + xd.abs().mean(dim=1, keepdim=True)) * rs * wd.abs()
             + ACC * bd.abs() + TINY[dtype])
    return ref, bound


def emulate_ln(x, w, b, dtype, order="seq", mutation=None):
    """The kernels' steps in float32: mean, centred second moment, 1 / sqrt(var + eps), (x - mean) rstd w + b, one store.
       mutation: unbiased (variance over d - 1), noeps, onepass (E[x^2] - mean^2), swap (gamma and beta), padmean (the sum divided
       by d rounded up to 64, or by d + 8 where d is a multiple of 64)."""
    xf, wf, bf = x.float(), w.float(), b.float()
    if mutation == "swap":
        wf, bf = bf, wf
    d = xf.shape[1]
    dm = ((d + 63) // 64 * 64 if d % 64 else d + 8) if mutation == "padmean" else d
    mean = (fsum(xf, order) / dm)[:, None]
    t = xf - mean
    if mutation == "onepass":
        var = fsum(xf * xf, order) / d - mean[:, 0] * mean[:, 0]
    else:
        var = fsum(t * t, order) / (d - 1 if mutation == "unbiased" else d)
    eps = 0.0 if mutation == "noeps" else LN_EPS
    rstd = (1.0 / torch.sqrt(var + torch.tensor(eps, dtype=torch.float32)))[:, None]
    return (t * rstd * wf + bf).to(TDT[dtype])
