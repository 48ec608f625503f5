"""Every op of the detector on its own, element by element, against fp64 within the bounds of oracle/yolo_op_bound.py, on frames
from 32 x 32 up.

The walk: for op i of the engine's program-order list (YoloSeg.ops()), forward_ops(i) runs the letterbox and the ops before it, the
op's input views are read (16-bit values widened, or float32: exact), forward_ops(i + 1) runs it too and its output view is read.
C2PSA updates a map in place, so inputs are only intact before the op ran.  The output must satisfy at EVERY element

    1.  |got - ref| <= bound                                        and got finite
    2.  relL2(got, ref) <= 1.25 relL2(emu, ref)                     (float32 throughout: <= || stat || / || ref ||)

with ref, bound, emu, stat of oracle/yolo_op_bound.py (derivations there; tests/test_yolo_op_bound.py shows what the two assertions
catch that a whole-map norm does not).  Pools and the upsample are compared for equality.  After the walk a whole forward() on the
shared-grid schedule (ymulti_kernel / y32m_multi_kernel) must reproduce every op's output view bit for bit; the in-place map of
C2PSA is compared at its final value.  A forward of another frame runs in between, so that every buffer holds other values when the
compared forward starts: a store the shared grid skips is then a stale value, not the walk's.  Each case first compares the
letterboxed network input with the oracle's preprocess(): equal.

Frames (SIZES): frame / imgsz -> letterboxed size
    32 x 32 / 32     32 x 32     maps 16, 8, 4, 2, 1; P5 is one pixel, attention with N = 1, pools on a 1 x 1 map, 21 anchors
    33 x 47 / 64     64 x 64     odd letterbox padding (9 / 10 rows), P5 2 x 2
    40 x 60 / 96     64 x 96     P5 2 x 3, N = 6
    90 x 160 / 160   96 x 160    Wo = 80, 40, 20, 10, 5; N = 15: one partly filled query group
    120 x 224 / 224  128 x 224   N = 28: one partial key block
    150 x 280 / 288  160 x 288   N = 45: two key blocks, fewer than the prefetch depth
    300 x 400 / 416  320 x 416   the layer-2 map is 80 x 104 = 8320 > 8192: the non-split path with long K, Bottleneck tiles of 8
                                 rows; N = 130: five key blocks, a second, partial prefetch round, a last workgroup with one live wave
Every size runs in f16, bf16 and f32 with default options; the 32, the 96 x 160 and the 320 x 416 one also with f32mfma = 0 (the
float32 checker kernels), tile = 0, bneck = 0, pool_lds = 0, generic_attn = 1 (f16 each) and the `s`-scale checkpoint (the other
Bottleneck codes and NT pairs, four attention heads).  Two added float32 cases reach what these frames do not: 736 x 736 walked up to
model.2.cv2 (two pixel tiles per wave in the MFMA conv) and 1568 x 1568, attention only (2401 tokens: the plain float32 attention
kernel, to which the MFMA one hands over above 2364 tokens, within 4 % of its own LDS limit).  fp64 work is remembered per (op, dtype, digest of the input bytes): most
option sets change no bit upstream.

Post-processing on the three smallest frames: detect() at a confidence at which the oracle alone keeps at least 3 boxes (CONF,
checked on the CPU in tests/test_yolo_op_bound.py), then the decode / NMS checks of tests/test_gpu_yolo.py and the merged mask
against Y.process_mask given the device's own rows, in f16 and f32.

The last test asserts that every kernel path flope_yolo_op_info can name (PATHS) was judged at least once.

MEASURED on one MI355X run of this file (documentation, not thresholds):
    op kind   dtype   worst |got - ref| / bound   worst relL2(got, ref) / yardstick of assertion 2
    conv      f16     0.980                       1.000
    conv      bf16    0.993                       1.000
    conv      f32     0.077                       0.209      (yardstick: || stat || / || ref ||; includes the float32 prediction rows)
    bneck     f16     0.394                       1.003
    bneck     bf16    0.466                       1.000
    dw        f16     0.995                       1.000
    dw        bf16    0.995                       1.000
    dw        f32     0.158                       0.065
    attn      f16     0.963                       1.009
    attn      bf16    0.579                       1.115
    attn      f32     0.051                       0.066
    pool, up  all     equal in every element
(16-bit yardstick: relL2(emu, ref); 1.000 means the device's map has the error norm of the plain float32 evaluation stored once.
0.98 .. 0.995 of the bound in 16-bit storage is the storage rounding itself: half an ulp is the bound's leading term.)
"""
import functools
import hashlib

import numpy as np
import pytest
import torch

from oracle import pipeline_ref as P
from oracle import yolo_op_bound as B
from oracle import yolo_ref as Y

SIZES = [(32, 32, 32), (33, 47, 64), (40, 60, 96), (90, 160, 160), (120, 224, 224), (150, 280, 288), (300, 400, 416)]
LETTERBOXED = [(32, 32), (64, 64), (64, 96), (96, 160), (128, 224), (160, 288), (320, 416)]
THREE = [SIZES[0], SIZES[3], SIZES[6]]
N_WIDTHS, S_WIDTHS = (16, 32, 64, 128, 256), (32, 64, 128, 256, 512)
BIG = (736, 736, 736)       # model.1's map is 184 x 184 = 33856 pixels: the float32 MFMA convs take two pixel tiles per wave from 32768
LONG = (1568, 1568, 1568)   # P5 is 49 x 49 = 2401 tokens: above the 2364 the float32 MFMA attention holds in LDS, below load_weights' 2560
FRAME_SEED = 3
CONF = {SIZES[0]: 0.01, SIZES[1]: 0.01, SIZES[2]: 0.01}       # the oracle alone keeps 4, 13 and 19 detections there


def _c(size, dtype="f16", widths=N_WIDTHS, **opts):
    return (size, dtype, widths, tuple(sorted(opts.items())))


CASES = ([_c(s, d) for s in SIZES for d in ("f16", "bf16", "f32")]
         + [_c(s, "f32", f32mfma=0) for s in THREE]
         + [_c(s, "f16", **{o: v}) for s in THREE for o, v in (("tile", 0), ("bneck", 0), ("pool_lds", 0), ("generic_attn", 1))]
         + [_c(s, "f16", S_WIDTHS) for s in THREE]
         + [_c(BIG, "f32", stop=6),           # stop: walk the first 6 ops only (model.0 .. model.2.cv2); not an engine option
            _c(LONG, "f32", only="attn")])    # only: judge the ops of this kind alone (the plain float32 attention kernel near its LDS limit)

# Every kernel path flope_yolo_op_info names on these cases: <launcher's words>.  16-bit convs: nt<channel tiles>.<1x1|3x3>.
# <splitk|tile|plain>.mode<0 map | 1 float32 prediction rows | 2 transposed-conv scatter>; fused Bottleneck: code = 4 i1 + i2 of the
# (NT1, NT2) pair, th = rows per tile; float32 mode: y32m.nt.mp<pixel tiles per wave>.<splitk|plain>, y32.plain (f32mfma = 0).
PATHS = [
    "attn.generic", "attn.mfma", "bneck.code0.th4", "bneck.code0.th8", "bneck.code1.th4", "bneck.code1.th8", "bneck.code10.th4",
    "bneck.code5.th4", "bneck.code6.th4", "dw", "nt1.1x1.plain.mode1", "nt1.1x1.tile.mode1", "nt1.3x3.plain.mode0",
    "nt1.3x3.splitk.mode0", "nt1.3x3.tile.mode0", "nt2.1x1.plain.mode0", "nt2.1x1.plain.mode1", "nt2.1x1.tile.mode0",
    "nt2.1x1.tile.mode1", "nt2.3x3.plain.mode0", "nt2.3x3.splitk.mode0", "nt2.3x3.tile.mode0", "nt4.1x1.plain.mode0",
    "nt4.1x1.plain.mode1", "nt4.1x1.plain.mode2", "nt4.1x1.splitk.mode0", "nt4.1x1.tile.mode0", "nt4.1x1.tile.mode1",
    "nt4.1x1.tile.mode2", "nt4.3x3.plain.mode0", "nt4.3x3.splitk.mode0", "nt4.3x3.tile.mode0", "pool.lds", "pool.ring", "up",
    "y32.attn", "y32.dw", "y32.plain.mode0", "y32.plain.mode1", "y32.plain.mode2", "y32.pool.lds", "y32.up", "y32m.attn",
    "y32m.nt1.mp1.plain.mode0", "y32m.nt1.mp1.plain.mode1", "y32m.nt1.mp1.splitk.mode0", "y32m.nt1.mp2.plain.mode0",
    "y32m.nt2.mp1.plain.mode0", "y32m.nt2.mp1.plain.mode1", "y32m.nt2.mp1.splitk.mode0", "y32m.nt4.mp1.plain.mode0",
    "y32m.nt4.mp1.plain.mode1", "y32m.nt4.mp1.plain.mode2", "y32m.nt4.mp1.splitk.mode0", "y32m.nt2.mp2.plain.mode0",
    "y32m.nt4.mp2.plain.mode0", "y32.attn.fallback",
]
# Paths of PATHS that no DEFAULT plan of these frames takes: reached by an option or an added case
BY_OPTION = {
    "pool.ring": "the LDS kernel takes every map up to 4608 pixels and load_weights refuses P5 maps above 2560: only with pool_lds = 0",
    "attn.generic": "the MFMA kernel takes N <= 1248 tokens (imgsz ~1150 and up go to the generic kernel): here with generic_attn = 1",
    "y32m.nt2.mp2.plain.mode0": "two pixel tiles per wave from 32768 output pixels: the added 736 x 736 float32 case, walked up to model.2.cv2",
    "y32m.nt4.mp2.plain.mode0": "as above",
    "y32.attn.fallback": "the float32 MFMA attention hands over to the plain kernel above 2364 tokens: the added 1568 x 1568 case, attention only",
}
# What the launchers could name and no loadable plan of the n / s checkpoints takes, with the reason.  Documentation: the coverage test
# only asserts that none of the concrete names below was seen (a name it does not know fails `set(seen) <= set(PATHS)` anyway).
NOT_REACHED = {
    "y32.fallback.mode*": "y32m_geometry refuses only map views that are not 16-byte aligned; channel widths are multiples of 8 (load_weights)",
    "y32.pool.sweep": "the float32 LDS pool takes maps up to 2560 pixels, exactly the P5 size load_weights accepts for C2PSA",
    "nt1.1x1.*.mode0, nt1/nt2.1x1.splitk.*": "no 1x1 Conv of <= 16 outputs, and none of <= 32 outputs with 256 inputs, in the yolo11 n / s graphs",
    "mode1 / mode2 with 3x3": "the prediction-row convs and the transposed conv are 1x1 by construction (Builder::plain, Builder::deconv)",
    "y32m.*.splitk.mode1 / mode2": "head rows and the Proto transposed conv read 64 .. 128 channels: fewer than the 8 k16 steps split-K starts at",
}

_DONE = {}          # case -> {path: ops judged}
_REF_CACHE = {}
_WORST = {}         # (kind, dtype) -> [worst err / bound, worst relL2(got) / yardstick of assertion 2]


def _case_id(c):
    (h, w, imgsz), dtype, widths, opts = c
    return f"{h}x{w}-{imgsz}-{dtype}" + ("-s" if widths == S_WIDTHS else "") + "".join(f"-{k}{v}" for k, v in opts)


@functools.lru_cache(maxsize=None)
def _sd(widths):
    from flope_amd.yolo_weights import synthetic_yolo_state_dict
    return {k: v.float() for k, v in synthetic_yolo_state_dict(0, widths=widths).items() if v.is_floating_point()}


def _frame(size):
    from flope_amd.yolo_weights import synthetic_frame
    return synthetic_frame(FRAME_SEED, size[0], size[1])


def _digest(tensors):
    h = hashlib.blake2b(digest_size=16)
    for t in tensors:
        if t is not None:
            h.update(t.contiguous().numpy().tobytes())
    return h.digest()


def _cached(key, ins, make):
    key = key + (_digest(ins),)
    if key not in _REF_CACHE:
        _REF_CACHE[key] = make()
    return _REF_CACHE[key]


def _walk(case):
    from flope_amd.yolo import YoloSeg
    size, dtype, widths, opts = case
    sd, img, dt = _sd(widths), _frame(size), B.TDT[dtype]
    y = YoloSeg(size[0], size[1], size[2], dtype)
    y.load_state_dict(sd)
    opts = dict(opts)
    stop, only = opts.pop("stop", None), opts.pop("only", None)
    for k, v in opts.items():
        y.set_option(k, v)
    assert y.input_hw == (LETTERBOXED[SIZES.index(size)] if size in SIZES else size[:2])
    ops = y.ops()
    lines, fails, paths = [f"{_case_id(case)}: {len(ops)} ops"], [], {}

    def read(i, what):
        return y.read_tensor(f"op{i}.{what}").cpu()[None]

    def judge(name, kind, path, got, j):
        f, rep, r2 = B.verdict(name, got, j, dt, path)
        fails.extend(f)
        w = _WORST.setdefault((kind, dtype), [0.0, 0.0])
        w[0], w[1] = max(w[0], rep.max_ratio), max(w[1], r2)
        lines.append(f"  {name:28s} {path:32s} {tuple(got.shape[1:])}  max err/bound {rep.max_ratio:6.3f}  relL2 / yardstick {r2:6.3f}")
        paths[path] = paths.get(path, 0) + 1

    # the letterbox (resize, padding rows, BGR -> RGB, / 255, one rounding) is exact
    y.forward_ops(img, 0)
    lb = y.read_tensor("input").cpu()
    if not torch.equal(lb[:3], B.store(Y.preprocess(img, size[2])[0], dt)) or lb[3:].any():
        fails.append("letterbox: the network input differs from the oracle's preprocess()")

    for i, info in enumerate(ops[:stop]):
        kind, name, path = info["kind"], info["name"], info["path"]
        if only is not None and kind != only:
            continue
        key = (kind, name, dtype, widths)
        y.forward_ops(img, i)
        x = read(i, "in")
        if kind == "conv":
            res = read(i, "res") if info["res"] else None
            y.forward_ops(img, i + 1)
            if info["cin_w"] < info["Cin"]:
                assert not x[:, info["cin_w"]:].any(), "model.0: the padding channels of the letterboxed input are not zero"
            judge(name, kind, path, read(i, "out"), _cached(key, (x, res), lambda: B.judge_conv_info(sd, info, x, res, dt)))
        elif kind == "bneck":
            i1, i2 = dict(info, name=name + ".cv1"), dict(info["cv2"], name=name + ".cv2")
            res = read(i, "res")
            assert torch.equal(res, x), "Bottleneck: the residual view is not the input view"
            y.forward_ops(img, i + 1)
            out = read(i, "out")
            if "+" in path:                   # bneck = 0: two conv launches, each judged through its own taps
                mid = read(i, "mid")
                p1, p2 = path.split("+")
                judge(i1["name"], "conv", p1, mid, _cached(key + (1,), (x,), lambda: B.judge_conv_info(sd, i1, x, None, dt)))
                judge(i2["name"], "conv", p2, out, _cached(key + (2,), (mid, x), lambda: B.judge_conv_info(sd, i2, mid, x, dt)))
            else:
                def fused():
                    w1, b1 = B.fold_conv(sd, i1["name"], dt)
                    w2, b2 = B.fold_conv(sd, i2["name"], dt)
                    return B.bneck_reference(x, w1, b1, w2, b2, dt)
                judge(name, kind, path, out, _cached(key, (x,), fused))
        elif kind == "dw":
            add = read(i, "add") if info["add"] else None
            y.forward_ops(img, i + 1)

            def dw():
                w, b = B.fold_dw(sd, name)
                return B.dw_reference(x, w, b, bool(info["act"]), add, dt, info["blk"], info["blk_stride"], info["blk_off"])
            judge(name, kind, path, read(i, "out"), _cached(key, (x, add), dw))
        elif kind in ("pool", "up"):
            y.forward_ops(img, i + 1)
            fn = (lambda t: B.pool_reference(t, info["n"])) if kind == "pool" else B.up_reference
            f = B.exact_failures(f"{name} [{path}]", read(i, "out"), x, fn)
            fails.extend(f)
            lines.append(f"  {name:28s} {path:32s} {(info['H'], info['W'])}  {'EXACT' if not f else 'DIFFERS'}")
            paths[path] = paths.get(path, 0) + 1
        elif kind == "attn":
            y.forward_ops(img, i + 1)
            q = x[0, :, 0]
            rounded = path == "attn.mfma"
            j = _cached(key + (rounded,), (q,), lambda: B.attn_reference(q, info["heads"], info["scale"], dt, rounded))
            judge(name, kind, path, read(i, "out")[0, :, 0], j)
        else:
            raise AssertionError(f"unknown op kind {kind}")

    # the shared-grid schedule: a whole forward must reproduce the program-order walk's final state in every bit.  Between the two
    # every buffer is overwritten by a forward of ANOTHER frame, so that a store the shared grid skips shows as a stale value
    if only is None:
        y.forward_ops(img, len(ops))
        walked = [y.read_tensor(f"op{i}.out") for i in range(len(ops))]
        from flope_amd.yolo_weights import synthetic_frame
        y.forward(synthetic_frame(FRAME_SEED + 1, size[0], size[1]))
        stale = sum(torch.equal(walked[i], y.read_tensor(f"op{i}.out")) for i in range(len(ops)))
        if stale:
            fails.append(f"the forward of another frame left {stale} op outputs bit-identical: the buffers are not overwritten")
        y.forward(img)
        for i, info in enumerate(ops):
            if not torch.equal(walked[i], y.read_tensor(f"op{i}.out")):
                fails.append(f"forward() on the level schedule differs from the program-order walk at op {i} ({info['name']}, {info['path']})")
    y.close()
    print("\n".join(lines))
    _DONE[case] = paths
    return fails


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_every_op_elementwise_within_the_derived_bound(case):
    fails = _walk(case)
    assert not fails, "\n".join(fails)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["f16", "f32"])
@pytest.mark.parametrize("size", SIZES[:3], ids=lambda s: f"{s[0]}x{s[1]}-{s[2]}")
def test_postprocessing_on_the_smallest_frames(size, dtype):
    """decode, NMS, box scaling and the merged mask on maps of a few pixels, given the device's own head rows and proto map"""
    import test_gpu_yolo as T
    from flope_amd.yolo import YoloSeg
    sd, img, conf = _sd(N_WIDTHS), _frame(size), CONF[size]
    y = YoloSeg(size[0], size[1], size[2], dtype)
    y.load_state_dict(sd)
    boxes, sc, cls, anchor, mask = y.detect(img, conf)
    T._check_decode_and_nms(y, img, 1, conf, 0.7, 300, boxes, sc, cls, anchor)
    assert len(anchor) >= 3
    det, idx = Y.non_max_suppression(Y.decode(T._head_rows(y)).numpy(), 1, conf)
    assert anchor.tolist() == idx.tolist()
    mfloat = Y.process_mask(y.read_tensor("proto").cpu(), det[:, 6:], det[:, :4], y.input_hw, return_float=True).numpy()
    ref_lb = (np.clip((mfloat > 0).astype(np.float32).sum(0), 0, 1) * 255).astype(np.uint8)
    got_lb = y.read_tensor("mask_lb").cpu().numpy()[0].astype(np.uint8)
    assert got_lb.shape == ref_lb.shape and set(np.unique(got_lb)) <= {0, 255}
    assert 0.02 < (got_lb > 0).mean() < 0.98 and 0.02 < (ref_lb > 0).mean() < 0.98       # (the oracle alone: 0.06, 0.90, 0.93)
    for yy, xx in np.argwhere(got_lb != ref_lb):             # only where an instance's interpolated value is within round-off of zero
        assert np.abs(mfloat[:, yy, xx]).min() < 1e-5, (yy, xx, mfloat[:, yy, xx])
    # 2e-4 of a 32 x 32 mask is less than one pixel: one is allowed there, and only because the loop above already holds every
    # differing pixel to an interpolated value within 1e-5 of the threshold
    assert (got_lb != ref_lb).mean() < 2e-4 or (got_lb != ref_lb).sum() <= 1
    assert np.array_equal(mask, P.resize_linear_u8(got_lb, (size[1], size[0])))
    y.close()


@pytest.mark.gpu
def test_every_kernel_path_was_judged():
    """Runs last; cases that did not run in this session (a -k selection) are walked here, so the assertion stands alone."""
    for case in CASES:
        if case not in _DONE:
            _walk(case)
    seen = {}
    for paths in _DONE.values():
        for p, n in paths.items():
            seen[p] = seen.get(p, 0) + n
    print("kernel paths judged (ops):", dict(sorted(seen.items())))
    print("worst err / bound and worst relL2(got) / yardstick per (op kind, dtype):")
    for (kind, dtype), (a, b) in sorted(_WORST.items()):
        print(f"    {kind:6s} {dtype:5s} {a:7.3f} {b:7.3f}")
    assert set(seen) <= set(PATHS), f"a kernel path this module does not know: {sorted(set(seen) - set(PATHS))}"
    missing = [p for p in PATHS if not seen.get(p)]
    assert not missing, f"kernel paths no case reached: {missing}"
    default = set()
    for case, paths in _DONE.items():
        if not case[3]:
            default |= set(paths)
    for p, why in BY_OPTION.items():
        assert p in PATHS and p not in default, f"{p} is listed as not reached by a default plan ({why}) but was"
    assert not set(seen) & set(NOT_REACHED), sorted(set(seen) & set(NOT_REACHED))
