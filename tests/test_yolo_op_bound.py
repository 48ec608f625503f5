"""CPU tests of oracle/yolo_op_bound.py: the per-op bound of the detector passes correct evaluations and fails planted errors.

On maps of at most 24 x 40, with the synthetic checkpoint's weights and random stored inputs, in f16, bf16 and f32:

  * the plain float32 emulation of every op kind (conv 3x3 / 1x1 / stride 2 / model.0 with 3 real input channels, the float32
    prediction rows, the transposed conv, the fused Bottleneck, depthwise with and without the qkv channel mapping, the three
    cascaded pools, the upsample, attention) passes both assertions; so does a conv summed in four K chunks (the split-K order) and the
    emulation of the MFMA attention kernel, which rounds P to the storage type;
  * every planted error of MUTATIONS fails at least one assertion in every storage type.  (`bn_eps` changes every folded weight by
    the relative 3.6e-4 .. 8.3e-4 only, running_var being 0.6 .. 1.4: below bf16's rounding as a scale error, but a tenth of the
    stored bf16 weights land on the neighbouring value, a full 2^-8 away, and assertion 1 sees those.)  The planted pool errors are
    compared for equality, as the device's pools are.
  * for each planted error the table printed by the test says whether the whole-map rel-L2 threshold of tests/test_gpu_yolo.py
    (5e-3 f16, 8e-2 bf16, 2e-5 f32) would have caught it on the op's own output.

Not in the list, because the derived bound allows them (oracle/yolo_op_bound.py says why): P . V normalised by the sum of the rounded
probabilities, and a Bottleneck intermediate that is not rounded to the storage type.  `test_what_the_bound_cannot_tell_apart` shows
both inside the bound.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

from oracle import yolo_op_bound as B

DTYPES = ["f16", "bf16", "f32"]
H, W = 23, 37                    # 851 pixels: 26 whole 32-pixel units and one of 19; three 16-wide tiles, the last 5 wide


@functools.lru_cache(maxsize=None)
def _sd():
    from flope_amd.yolo_weights import synthetic_yolo_state_dict
    return synthetic_yolo_state_dict(0)


def _rand(dt, *shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed * 7919 + sum(shape))
    return B.store(torch.randn(*shape, generator=g) * scale, dt)


def _fails(name, got, j, dt):
    return B.verdict(name, got, j, dt)[0]


# ---- every op kind: the emulation passes ----------------------------------------------------------------------------------------
CONVS = [  # (state_dict name, stride, act, residual, deconv, float32 rows, real Cin)
    ("model.0", 2, True, False, False, False, 3), ("model.1", 2, True, False, False, False, 16), ("model.2.cv2", 1, True, False, False, False, 48),
    ("model.2.m.0.cv2", 1, True, True, False, False, 8), ("model.10.m.0.ffn.1", 1, False, True, False, False, 256),
    ("model.23.cv2.0.2", 1, False, False, False, True, 64), ("model.23.proto.upsample", 1, False, False, True, False, 64),
]


def _conv_case(name, stride, act, has_res, deconv, rows, cin, dt, h=H, w=W):
    sd = _sd()
    wt, b = B.conv_weights(sd, name, dt, deconv)
    x = _rand(dt, 1, cin, h, w, seed=1)
    cout = wt.shape[1] if deconv else wt.shape[0]
    ho, wo = (2 * h, 2 * w) if deconv else ((h - 1) // stride + 1, (w - 1) // stride + 1)
    res = _rand(dt, 1, cout, ho, wo, seed=2) if has_res else None
    return x, wt, b, res


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", CONVS, ids=[c[0] for c in CONVS])
def test_conv_emulations_pass(case, dtype):
    name, stride, act, has_res, deconv, rows, cin = case
    dt = B.TDT[dtype]
    x, wt, b, res = _conv_case(*case, dt)
    j = B.conv_reference(x, wt, b, stride, act, res, dt, deconv, rows)
    assert not _fails(name, j.emu, j, dt)
    if not deconv and cin >= 8:           # the split-K order: four partial sums over the input channels, added in float32
        q = cin // 4
        y = sum(F.conv2d(x[:, i * q:(i + 1) * q].float(), wt[:, i * q:(i + 1) * q], None, stride=stride, padding=wt.shape[-1] // 2) for i in range(4))
        y = y + b.view(1, -1, 1, 1)
        y = F.silu(y) if act else y
        y = y + res if res is not None else y
        got = y if rows else B.store(y, dt)
        fails, rep, _ = B.verdict(name, got, j, dt)
        assert not fails, fails
        print(f"{name} {dtype} split-K order: worst err/bound {rep.max_ratio:.3g}")


def _bneck_case(dt):
    sd = _sd()
    w1, b1 = B.fold_conv(sd, "model.2.m.0.cv1", dt)
    w2, b2 = B.fold_conv(sd, "model.2.m.0.cv2", dt)
    return _rand(dt, 1, 16, H, W, seed=3), w1, b1, w2, b2


@pytest.mark.parametrize("dtype", DTYPES)
def test_bottleneck_dw_pool_up_emulations_pass(dtype):
    dt = B.TDT[dtype]
    sd = _sd()
    j = B.bneck_reference(*_bneck_case(dt), dt)
    assert not _fails("bneck", j.emu, j, dt)
    w, b = B.fold_dw(sd, "model.23.cv3.0.0.0")
    j = B.dw_reference(_rand(dt, 1, 64, H, W, seed=4), w, b, True, None, dt)
    assert not _fails("dw", j.emu, j, dt)
    w, b = B.fold_dw(sd, "model.10.m.0.attn.pe")
    j = B.dw_reference(_rand(dt, 1, 256, 5, 7, seed=5), w, b, False, _rand(dt, 1, 128, 5, 7, seed=6), dt, 64, 128, 64)
    assert not _fails("dw pe", j.emu, j, dt)
    for (h, w_) in ((1, 1), (2, 3), (4, 4), (5, 9), (10, 13)):        # maps smaller than the 5 x 5 window, and larger
        x = _rand(dt, 1, 8, h, w_, seed=7)
        assert not B.exact_failures("pool", B.pool_reference(x), x, B.pool_reference)
        assert not B.exact_failures("up", B.up_reference(x), x, B.up_reference)


# Attention is fed the network's own qkv maps (the CPU oracle's forward with the device's rounding points, then model.10's qkv conv):
# assertion 2 of the MFMA kernel holds on those, not on white noise (oracle/yolo_op_bound.py, "Assertion 2 and the MFMA kernel")
ATTN_FRAMES = {1: (32, 32, 32), 6: (40, 60, 96), 15: (90, 160, 160), 28: (120, 224, 224), 45: (150, 280, 288), 130: (300, 400, 416)}
ATTN_N = list(ATTN_FRAMES)


@functools.lru_cache(maxsize=None)
def _qkv(N, dtype):
    from flope_amd.yolo_weights import synthetic_frame
    from oracle import yolo_ref as Y
    h, w, imgsz = ATTN_FRAMES[N]
    dt = B.TDT[dtype]
    qkv = Y.c2psa_qkv(_sd(), Y.preprocess(synthetic_frame(3, h, w), imgsz), emulate=None if dtype == "f32" else dt)
    assert qkv.shape[2] * qkv.shape[3] == N and qkv.shape[2] <= 24 and qkv.shape[3] <= 40
    return B.store(qkv[0].reshape(qkv.shape[1], N), dt)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N", ATTN_N)
def test_attention_emulations_pass(N, dtype):
    dt = B.TDT[dtype]
    qkv = _qkv(N, dtype)
    scale = 32 ** -0.5
    j = B.attn_reference(qkv, 2, scale, dt, p_rounded=False)
    assert not _fails("attn", j.emu, j, dt)
    if dtype != "f32":                    # the MFMA kernel's steps, P rounded: inside the bound with the u_P A term, and inside assertion 2
        jm = B.attn_reference(qkv, 2, scale, dt, p_rounded=True)
        fails, rep, r2 = B.verdict("attn mfma", B.attn_emulate_mfma(qkv, 2, scale, dt), jm, dt)
        print(f"attention N={N} {dtype}: MFMA emulation worst err/bound {rep.max_ratio:.3g}, relL2 / relL2(emu) {r2:.3g}")
        assert not fails, fails


# ---- planted errors -------------------------------------------------------------------------------------------------------------
def _mut_conv(which, dt):
    """a 3x3 SiLU conv with residual on 23 x 37 -> (Judged, the broken output)"""
    case = ("model.2.m.0.cv2", 1, True, True, False, False, 8)
    x, wt, b, res = _conv_case(*case, dt)
    j = B.conv_reference(x, wt, b, 1, True, res, dt)
    if which == "border_tap":             # one padding cell above the top row holds its neighbour's value instead of zero
        xp = F.pad(x.float(), (1, 1, 1, 1))
        xp[:, :, 0, 6] = x[:, :, 0, 5]
        got = B.store(F.silu(F.conv2d(xp, wt, b)) + res, dt)
    elif which == "tile_last_column":     # column 15 of the first 16-wide tile taken from column 16
        got = j.emu.clone()
        got[..., 15] = got[..., 16]
    elif which == "res_before_silu":
        got = B.conv_emulate(x, wt, b, 1, True, res, dt, res_first=True)
    elif which == "res_dropped_last_unit":
        got = j.emu.clone().reshape(1, -1, H * W)
        first = (H * W - 1) // 32 * 32
        got[..., first:] = B.conv_emulate(x, wt, b, 1, True, None, dt).reshape(1, -1, H * W)[..., first:]
        got = got.reshape(j.emu.shape)
    elif which == "tap_missing":
        w2 = wt.clone()
        w2[:, 5, 2, 0] = 0
        got = B.conv_emulate(x, w2, b, 1, True, res, dt)
    elif which == "bn_eps":
        w2, b2 = B.fold_conv(_sd(), case[0], dt, eps=1e-5)
        got = B.conv_emulate(x, w2, b2, 1, True, res, dt)
    return j, got


def _mut_dw(which, dt):
    w, b = B.fold_dw(_sd(), "model.10.m.0.attn.pe")
    x, add = _rand(dt, 1, 256, 5, 7, seed=5), _rand(dt, 1, 128, 5, 7, seed=6)
    j = B.dw_reference(x, w, b, False, add, dt, 64, 128, 64)
    return j, B.dw_reference(x, w, b, False, add, dt, 64, 128, 56).emu


def _mut_attn(which, dt):
    qkv = _qkv(45, {v: k for k, v in B.TDT.items()}[dt]).clone()
    for h in range(2):                    # one key of the second 32-key block scaled up: the running maximum of about half the queries moves there
        qkv[h * 128 + 32:h * 128 + 64, 40] *= 64.0
    j = B.attn_reference(qkv, 2, 32 ** -0.5, dt, p_rounded=dt != torch.float32)
    sdt = dt if dt != torch.float32 else torch.float32
    return j, B.attn_emulate_mfma(qkv, 2, 32 ** -0.5, sdt, {"last_key_masked": "lastkey", "no_running_max_rescale": "noalpha"}[which])


MUTATIONS = {   # name -> (builder, storage types in which it must fail an assertion)
    "border_tap": (_mut_conv, DTYPES), "tile_last_column": (_mut_conv, DTYPES), "res_before_silu": (_mut_conv, DTYPES),
    "res_dropped_last_unit": (_mut_conv, DTYPES), "tap_missing": (_mut_conv, DTYPES), "bn_eps": (_mut_conv, DTYPES),
    "dw_blk_off_by_8": (_mut_dw, DTYPES), "last_key_masked": (_mut_attn, DTYPES), "no_running_max_rescale": (_mut_attn, DTYPES),
}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("which", list(MUTATIONS))
def test_planted_errors_fail(which, dtype):
    dt = B.TDT[dtype]
    build, must = MUTATIONS[which]
    j, got = build(which, dt)
    fails, rep, r2 = B.verdict(which, got, j, dt)
    whole = B.rel_l2(got, j.ref)
    print(f"{which} {dtype}: {rep.count} of {rep.total} elements over the bound (worst {rep.max_ratio:.3g}), assertion 2 ratio {r2:.3g}; "
          f"rel-L2 of the map {whole:.2e}: the whole-map threshold {B.GRAPH_REL_L2[dtype]:.0e} {'catches' if whole > B.GRAPH_REL_L2[dtype] else 'MISSES'} it")
    if dtype in must:
        assert fails, f"{which} in {dtype} passed both assertions"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("which", ["pool_border_zero", "pool_two_of_three"])
def test_planted_pool_errors_fail(which, dtype):
    dt = B.TDT[dtype]
    x = _rand(dt, 1, 8, 7, 9, seed=9) - 1.0              # negative values at the border: a zero border wins the maximum there
    good = B.pool_reference(x)
    if which == "pool_border_zero":
        cur, outs = x, []
        for _ in range(3):
            cur = F.max_pool2d(F.pad(cur, (2, 2, 2, 2), value=0.0), 5, 1, 0)
            outs.append(cur)
        got = torch.cat(outs, 1)
    else:
        got = good.clone()
        got[:, 16:] = good[:, 8:16]
    whole = B.rel_l2(got, good)
    print(f"{which} {dtype}: rel-L2 of the map {whole:.2e}: the whole-map threshold {'catches' if whole > B.GRAPH_REL_L2[dtype] else 'MISSES'} it")
    assert B.exact_failures(which, got, x, B.pool_reference)


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_what_the_bound_cannot_tell_apart(dtype):
    """Documented blind spots (oracle/yolo_op_bound.py): both stay inside assertion 1 by the bound's own terms."""
    dt = B.TDT[dtype]
    qkv = _qkv(45, dtype)
    j = B.attn_reference(qkv, 2, 32 ** -0.5, dt, p_rounded=True)
    rep = B.check("l from rounded P", B.attn_emulate_mfma(qkv, 2, 32 ** -0.5, dt, "lrounded"), j.ref, j.bound)
    print(f"P.V normalised by the rounded sum, {dtype}: worst err/bound {rep.max_ratio:.3g}")
    assert rep.ok
    x, w1, b1, w2, b2 = _bneck_case(dt)
    j = B.bneck_reference(x, w1, b1, w2, b2, dt)
    mid = F.silu(F.conv2d(x.float(), w1, b1, padding=1))                      # float32, never rounded to the storage type
    rep = B.check("unrounded intermediate", B.conv_emulate(mid, w2, b2, 1, True, x, dt), j.ref, j.bound)
    print(f"Bottleneck intermediate not rounded, {dtype}: worst err/bound {rep.max_ratio:.3g}")
    assert rep.ok


def test_f16_saturation_is_reported_not_masked():
    dt = torch.float16
    x, wt, b, res = _conv_case("model.2.m.0.cv2", 1, True, True, False, False, 8, dt)
    j = B.conv_reference(x * 2048, wt * 64, b, 1, True, res, dt)
    assert any("float16 range" in f for f in _fails("saturating", j.emu, j, dt))


def test_postprocessing_thresholds_keep_three_oracle_detections():
    """tests/test_gpu_yolo_ops.py runs detect() on its three smallest frames at CONF: the oracle alone keeps at least 3 boxes there"""
    import test_gpu_yolo_ops as G
    from oracle import yolo_ref as Y
    assert list(G.CONF) == G.SIZES[:3]
    for size, conf in G.CONF.items():
        img = G._frame(size)
        nw, nh, top, bottom, left, right = Y.letterbox_geometry(size[0], size[1], size[2])
        assert (nh + top + bottom, nw + left + right) == G.LETTERBOXED[G.SIZES.index(size)]
        o = Y.forward_layers(_sd(), Y.preprocess(img, size[2]))
        _, idx = Y.non_max_suppression(Y.decode(o).numpy(), 1, conf, 0.7)
        assert len(idx) >= 3, (size, conf, len(idx))


def test_size_table_geometry():
    import test_gpu_yolo_ops as G
    from oracle import yolo_ref as Y
    for size, lb in zip(G.SIZES, G.LETTERBOXED):
        nw, nh, top, bottom, left, right = Y.letterbox_geometry(size[0], size[1], size[2])
        assert (nh + top + bottom, nw + left + right) == lb, (size, lb)
    assert Y.letterbox_geometry(33, 47, 64)[2:4] == (9, 10)                 # odd padding: 9 rows above, 10 below
    assert [lb[0] // 32 * (lb[1] // 32) for lb in G.LETTERBOXED] == [1, 4, 6, 15, 28, 45, 130]      # attention tokens


def test_op_hook_c_abi_and_info_parser():
    """the per-op hook without a device: NULL handles are refused, and the Python side splits an info line as the walk expects"""
    import ctypes as C
    from flope_amd import _lib
    from flope_amd.yolo import parse_op_info
    lib = _lib.load()
    buf = C.create_string_buffer(256)
    assert lib.flope_yolo_op_count(None) == 0
    assert lib.flope_yolo_op_info(None, 0, buf, len(buf)) == _lib.EINVAL
    assert lib.flope_yolo_forward_ops(None, None, 0, None) == _lib.EINVAL
    d = parse_op_info("kind=bneck name=model.2.m.0 k=3 s=1 act=1 Hi=8 Wi=8 Cin=16 cin_w=16 Ho=8 Wo=8 Cout=8 mode=0 dc=0 res=0 | "
                      "k=3 s=1 act=1 Hi=8 Wi=8 Cin=8 cin_w=8 Ho=8 Wo=8 Cout=16 mode=0 dc=0 res=1 path=bneck.code0.th4")
    assert d["kind"] == "bneck" and d["name"] == "model.2.m.0" and d["Cout"] == 8 and d["cv2"]["Cout"] == 16 and d["cv2"]["res"] == 1
    assert d["path"] == "bneck.code0.th4" and "path" not in d["cv2"]
    a = parse_op_info("kind=attn name=model.10.m.0.attn N=15 heads=2 scale=0.176776692 path=attn.mfma")
    assert a["N"] == 15 and abs(a["scale"] - 32 ** -0.5) < 1e-8 and a["path"] == "attn.mfma"
