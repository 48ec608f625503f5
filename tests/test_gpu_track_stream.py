"""An encoder stream stepped on the device by the device tracker's association (enc.open_stream(..., positions="device"),
st.step_tracker / st.step_assoc, flope_tf_stream_step_tracker / _step_assoc, tf_stream_feed_kernel).  Scenario, the
brute-force rule and the expected token bits: tests/track_stream_cases.py (its CPU half: tests/test_tf_feed_host.py).

  1. bits against a twin host-positioned stream stepped with last_feed()'s tracks and last_tokens()'s rows: every dtype, step_split
     0 / 1, with and without a per-head ALiBi table, capacities 4 and 6 under a window of 4; cache and positions at the end
  2. the feed: last_feed() is the Python rule on last_association(), last_tokens() the float32 of the host-compiled measurement (or
     of filtered_state()), padding columns and rows that feed nothing are zero
  3. rows that feed nothing come back as out_layer.bias over a NaN pre-fill and write no cache row (NaN tokens in them stay unseen)
  4. step_assoc gives step_tracker's bits          6. refusals
  5. overflow                                      7. FlowerModel(tracker="device", track_stream=st)
"""
import numpy as np
import pytest
import torch

import track_cases as TC
import track_stream_cases as SC

pytestmark = pytest.mark.gpu

VEC = (7, 32, 9, 4, 2, 64)            # head_dim 8: the vector path in every dtype
SCALAR = (7, 30, 3, 5, 1, 20)         # head_dim 6: the scalar path
PADDED = (9, 32, 9, 4, 2, 64)         # input_dim 9: two padding columns
PLANS = {"row": 0, "split": 1, "biased": 2}


def _bits(t):
    return t.contiguous().view(torch.int32)


def _sd(dims, seed=46):
    from oracle import tf_encoder_ref as T
    return T.synthetic_state_dict(dims[0], dims[1], dims[2], dims[4], dims[5], seed=seed)


_SDS = {}


def _encoder(dims, dtype="f32", **kw):
    from flope_amd.tf_encoder import TransformerEncoder
    if dims not in _SDS:
        _SDS[dims] = _sd(dims)
    enc = TransformerEncoder(*dims, dtype=dtype, max_tokens=16, **kw)
    enc.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in _SDS[dims].items()})
    return enc


def _tracker(max_tracks=SC.MAX_TRACKS, max_meas=SC.MAX_MEAS):
    from flope_amd.track import DeviceTracker
    return DeviceTracker("cuda", max_tracks=max_tracks, max_meas=max_meas, dist_th=TC.TH_MM, q=TC.Q, r=TC.R, p0=TC.P0)


def _table(enc, alibi):
    from flope_amd.tf_encoder import alibi_distances
    return alibi_distances(SC.WINDOW, [2.0 ** -(h + 1) for h in range(enc.dims[3])]) if alibi else None


def _bias_row(dims):
    return torch.from_numpy(np.asarray(_SDS[dims]["out_layer.bias"], dtype=np.float32))


def _pair(enc, cap, alibi):
    """a device-positioned state and its host-positioned twin: the same window, capacity and table"""
    table = _table(enc, alibi)
    st = enc.open_stream(SC.STREAM_TRACKS, cap, window=SC.WINDOW, bias=table, positions="device", max_rows=SC.MAX_MEAS)
    twin = enc.open_stream(SC.STREAM_TRACKS, cap, window=SC.WINDOW, bias=table)
    return st, twin


def _check_frame(enc, st, twin, y, dims):
    """y [n, out]: fed rows equal, in bits, the twin stepped with the tracks of last_feed() and the rows of last_tokens(); the others are
    out_layer.bias in bits -> (who, where, tokens)"""
    who, where = st.last_feed()
    tok = st.last_tokens()
    fed = who >= 0
    assert len(who) == y.shape[0] == len(tok)
    if fed.any():
        assert [twin.position(int(t)) for t in who[fed]] == where[fed].tolist()
        want = twin.step(torch.from_numpy(tok[fed]).cuda(), who[fed].tolist())
        assert torch.equal(_bits(y[torch.from_numpy(fed).cuda()]), _bits(want)), "a fed row differs from the host-fed stream"
    if (~fed).any():
        rest = y[torch.from_numpy(~fed).cuda()].cpu()
        assert torch.equal(_bits(rest), _bits(_bias_row(dims).expand_as(rest))), "a row that fed nothing is not out_layer.bias"
    return who, where, tok


def _scenario_run(enc, dims, cap, alibi, source="measurement"):
    """the scenario through step_tracker, frame by frame against the twin -> (per frame (y on the host, who, where, tokens, assoc), st, twin, trk)"""
    st, twin = _pair(enc, cap, alibi)
    trk = _tracker()
    out = []
    for fr in SC.scenario().frames:
        trk.update(fr.poses, fr.cam, fr.rel)
        y = torch.full((len(fr.poses), dims[2]), float("nan"), device="cuda")
        assert st.step_tracker(trk, source, out=y) is y
        who, where, tok = _check_frame(enc, st, twin, y, dims)
        out.append((y.cpu(), who, where, tok, trk.last_association()))
    return out, st, twin, trk


def _same_cache(enc, st, twin, dims):
    """the caches hold the same bits: `window` further steps of every track on both states, the same rows"""
    g = torch.Generator().manual_seed(5)
    every = torch.arange(SC.STREAM_TRACKS, dtype=torch.int32, device="cuda")
    assert st.positions == twin.positions
    for _ in range(SC.WINDOW):
        x = torch.randn(SC.STREAM_TRACKS, dims[0], generator=g).cuda()
        a, b = st.step_assoc(x, every), twin.step(x)
        assert torch.equal(_bits(a), _bits(b)), "the caches differ"
    assert st.positions == twin.positions


_F32_ROWS = {}


def _f32_rows(cap):
    """test 1's rows of the float32 encoder without a table: computed once, shared with tests 4 and 7"""
    if cap not in _F32_ROWS:
        enc = _encoder(VEC)
        run, st, twin, trk = _scenario_run(enc, VEC, cap, False)
        _F32_ROWS[cap] = [r[0] for r in run]
        for o in (st, twin, trk, enc):
            o.close()
    return _F32_ROWS[cap]


# ---- 1. bits against the host-fed stream ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alibi", [False, True], ids=["plain", "alibi"])
@pytest.mark.parametrize("split", [0, 1])
@pytest.mark.parametrize("dims", [VEC, SCALAR], ids=["vec", "scalar"])
@pytest.mark.parametrize("dtype", ["f32", "f32m", "f16", "bf16"])
def test_step_tracker_equals_the_host_fed_stream(dtype, dims, split, alibi):
    enc = _encoder(dims, dtype, step_split=split)
    want_feed, want_pos = SC.scenario_feed()
    for cap in SC.CAPACITIES:
        st, twin = _pair(enc, cap, alibi)
        plan = st.step_plan                                            # read, not assumed
        assert plan == twin.step_plan and plan == ("biased" if alibi else plan) and enc.lib.flope_tf_stream_step_plan(st.state) == PLANS[plan]
        if not alibi and split and dims == VEC:
            assert plan == "split"
        st.close(); twin.close()
        run, st, twin, trk = _scenario_run(enc, dims, cap, alibi)
        for (y, who, where, tok, assoc), (w_who, w_where) in zip(run, want_feed):
            assert who.tolist() == w_who.tolist() and where.tolist() == w_where.tolist()
            assert torch.isfinite(y).all()
        assert st.positions == want_pos == twin.positions
        _same_cache(enc, st, twin, dims)
        assert trk.sentinels_changed() == 0
        for o in (st, twin, trk):
            o.close()
    enc.close()


# ---- 2. the feed ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("source", ["measurement", "mean"])
def test_the_feed_and_the_token_rows(source):
    H = SC.load_harness()
    enc = _encoder(PADDED)
    st, twin = _pair(enc, 6, False)
    trk = _tracker()
    pos = [0] * SC.STREAM_TRACKS
    for fr, want_assoc in zip(SC.scenario().frames, SC.scenario_assoc()):
        trk.update(fr.poses, fr.cam, fr.rel)
        y = st.step_tracker(trk, source)
        assoc = trk.last_association()
        assert assoc.tolist() == want_assoc                             # (the tracker itself: tests/test_gpu_track.py)
        w_who, w_where, pos = SC.feed_rule(assoc, 0, SC.STREAM_TRACKS, pos)
        who, where = st.last_feed()
        assert who.dtype == np.int32 and who.tolist() == w_who.tolist() and where.tolist() == w_where.tolist()
        tok = st.last_tokens()
        assert tok.dtype == np.float32 and tok.shape == (len(fr.poses), 9) and y.shape == (len(fr.poses), PADDED[2])
        if source == "measurement":
            want = SC.expected_tokens(H, fr, who, 9)
        else:
            means = trk.filtered_state()
            want = np.zeros_like(tok)
            for m, t in enumerate(who):
                if t >= 0:
                    want[m, :7] = means[t].astype(np.float32)
        assert tok.tobytes() == want.tobytes()
        assert (tok[:, 7:] == 0).all() and (tok[who < 0] == 0).all() and np.abs(tok[who >= 0, :7]).max() > 0
        assert st.positions == pos
    for o in (st, twin, trk, enc):
        o.close()


# ---- 3. rows that feed nothing -------------------------------------------------------------------------------------------------------------
def test_rows_that_feed_nothing_are_the_bias_and_touch_no_cache_row():
    """step_assoc with NaN in every row that feeds nothing (a duplicate, a track out of range, a skipped row): the output rows are
    out_layer.bias over a NaN pre-fill, and neither the positions nor any cache row of the tracks they name has moved -- a NaN token
    in the ring would reach every later row of that track through 0 x NaN"""
    enc = _encoder(VEC)
    st, twin = _pair(enc, 4, False)
    g = torch.Generator().manual_seed(3)
    o = lambda t: -1 - t                                               # noqa: E731
    frames = [[o(0), o(1), o(0), 7, SC.SKIPPED_ASSOC], [1, 1, 0, 0, o(6)], [0, SC.SKIPPED_ASSOC, 0, 1, 1, 6]] * 3      # 9 frames: the ring of 4 wraps
    pos = [0] * SC.STREAM_TRACKS
    for assoc in frames:
        who, _, pos = SC.feed_rule(assoc, 0, SC.STREAM_TRACKS, pos)
        x = torch.randn(len(assoc), VEC[0], generator=g)
        x[torch.from_numpy(who < 0)] = float("nan")
        y = torch.full((len(assoc), VEC[2]), float("nan"), device="cuda")
        st.step_assoc(x.cuda(), torch.tensor(assoc, dtype=torch.int32, device="cuda"), out=y)
        got, _, _ = _check_frame(enc, st, twin, y, VEC)
        assert got.tolist() == who.tolist() and st.positions == pos
        assert torch.isfinite(y).all(), "a NaN token of a row that feeds nothing was seen"
    assert pos[:2] == [9, 9] and pos[2:] == [0] * 4
    _same_cache(enc, st, twin, VEC)
    for o_ in (st, twin, enc):
        o_.close()


# ---- 4. step_assoc -------------------------------------------------------------------------------------------------------------------------
def test_step_assoc_gives_the_bits_of_step_tracker():
    enc = _encoder(VEC)
    for cap in SC.CAPACITIES:
        want = _f32_rows(cap)
        run, st, twin, trk = _scenario_run(enc, VEC, cap, False)
        st.reset()
        assert st.positions == [0] * SC.STREAM_TRACKS
        flag = torch.zeros(1, dtype=torch.int32, device="cuda")
        for (y, who, where, tok, assoc), w in zip(run, want):
            assert torch.equal(_bits(y), _bits(w))
            rows = torch.from_numpy(tok).cuda()
            rows[torch.from_numpy(who < 0)] = 7.5                      # the caller's rows need not be zero where nothing feeds
            got = st.step_assoc(rows, torch.from_numpy(assoc).cuda(), overflow=flag)
            assert torch.equal(_bits(got.cpu()), _bits(w))
            a_who, a_where = st.last_feed()
            assert a_who.tolist() == who.tolist() and a_where.tolist() == where.tolist() and st.last_tokens().tobytes() == tok.tobytes()
        for o in (st, twin, trk):
            o.close()
    enc.close()


# ---- 5. overflow ---------------------------------------------------------------------------------------------------------------------------
def test_overflow_feeds_nothing():
    enc = _encoder(VEC)
    st, twin = _pair(enc, 4, False)
    trk = _tracker(4, 4)
    three, two_more, one_more = TC.overflow_frames()
    trk.update(*three)
    y = st.step_tracker(trk)
    assert st.last_feed()[0].tolist() == [0, 1, 2] and st.positions == [1, 1, 1, 0, 0, 0] and torch.isfinite(y).all()
    for fr in (two_more, one_more):                                    # the frame that overflows, and one behind it (the flag is sticky)
        trk.update(*fr)
        y = torch.full((len(fr.poses), VEC[2]), float("nan"), device="cuda")
        st.step_tracker(trk, out=y)
        who, where = st.last_feed()
        assert who.tolist() == [SC.OVERFLOW] * len(fr.poses) and where.tolist() == [0] * len(fr.poses)
        assert (st.last_tokens() == 0).all() and st.positions == [1, 1, 1, 0, 0, 0]
        assert torch.equal(_bits(y.cpu()), _bits(_bias_row(VEC).expand(len(fr.poses), -1)))
    assert trk.raw_state(4)[4].tolist() == [3, 1]
    trk.reset(); st.reset()
    trk.update(*three)
    st.step_tracker(trk)
    assert st.last_feed()[0].tolist() == [0, 1, 2] and st.positions == [1, 1, 1, 0, 0, 0]
    # the flag as step_assoc takes it
    flag = torch.ones(1, dtype=torch.int32, device="cuda")
    y = st.step_assoc(torch.randn(2, VEC[0]).cuda(), torch.tensor([0, 1], dtype=torch.int32, device="cuda"), overflow=flag)
    assert st.last_feed()[0].tolist() == [SC.OVERFLOW] * 2 and st.positions == [1, 1, 1, 0, 0, 0]
    assert torch.equal(_bits(y.cpu()), _bits(_bias_row(VEC).expand(2, -1)))
    for o in (st, twin, trk, enc):
        o.close()


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    from flope_amd import _lib
    enc = _encoder(VEC)
    st, twin = _pair(enc, 4, False)
    trk = _tracker()
    fr = SC.scenario().frames[0]
    x = torch.randn(3, VEC[0]).cuda()
    a = torch.tensor([0, 1, 2], dtype=torch.int32, device="cuda")
    # the old calls on a device state name the call to use instead; nothing moves
    for call, word in ((lambda: st.step(x, [0, 1, 2]), "step_assoc"), (lambda: st.extend(x[:, None].contiguous(), tracks=[0, 1, 2]), "step_assoc"),
                       (lambda: st.prefill(x[:, None].contiguous(), tracks=[0, 1, 2]), "step_assoc"), (lambda: st.position(0), "read_positions"),
                       (lambda: enc._check_arg(enc.lib.flope_tf_stream_reset(st.state, 0, None)), "reset_device"),
                       (lambda: st.attention(torch.zeros(1, 2, 3 * VEC[1], device="cuda")), "open_window"),
                       (lambda: st.attention_extend(torch.zeros(1, 2, 3 * VEC[1], device="cuda"), [2], [1]), "open_window")):
        with pytest.raises(RuntimeError, match=word):
            call()
    # the new ones on a host state
    for call in (lambda: twin.step_assoc(x, a), lambda: twin.step_tracker(trk), twin.last_feed, twin.last_tokens):
        with pytest.raises(RuntimeError, match="open_device"):
            call()
    for fn in (enc.lib.flope_tf_stream_reset_device(twin.state, None), enc.lib.flope_tf_stream_read_positions(twin.state, None, 0)):
        assert fn == _lib.ESTATE
    # a tracker without an update, the same update twice
    with pytest.raises(RuntimeError, match="no update"):
        st.step_tracker(trk)
    trk.update(fr.poses, fr.cam, fr.rel)
    y = st.step_tracker(trk)
    with pytest.raises(RuntimeError, match="already"):
        st.step_tracker(trk)
    trk.reset()
    with pytest.raises(RuntimeError, match="no update"):
        st.step_tracker(trk)
    assert st.positions == [1, 1, 1, 0, 0, 0] and y.shape == (3, VEC[2])
    # n > max_rows, NULL buffers, a source that is none, n = 0
    small = enc.open_stream(SC.STREAM_TRACKS, 4, window=4, positions="device", max_rows=2)
    with pytest.raises(ValueError, match="max_rows"):
        small.step_assoc(x, a)
    trk.update(fr.poses, fr.cam, fr.rel)
    with pytest.raises(ValueError, match="max_rows"):
        small.step_tracker(trk)
    assert small.positions == [0] * SC.STREAM_TRACKS and small.last_feed()[0].tolist() == []
    sp = torch.cuda.current_stream().cuda_stream
    assert enc.lib.flope_tf_stream_step_assoc(st.state, None, a.data_ptr(), None, 3, y.data_ptr(), sp) == _lib.EINVAL
    assert enc.lib.flope_tf_stream_step_assoc(st.state, x.data_ptr(), None, None, 3, y.data_ptr(), sp) == _lib.EINVAL
    assert enc.lib.flope_tf_stream_step_assoc(st.state, x.data_ptr(), a.data_ptr(), None, 3, None, sp) == _lib.EINVAL
    assert enc.lib.flope_tf_stream_step_assoc(st.state, x.data_ptr(), a.data_ptr(), None, -1, y.data_ptr(), sp) == _lib.EINVAL
    assert enc.lib.flope_tf_stream_step_tracker(st.state, trk.handle, _lib.TF_FEED_MEAS, None, sp) == _lib.EINVAL
    assert enc.lib.flope_tf_stream_step_tracker(st.state, trk.handle, 2, y.data_ptr(), sp) == _lib.EINVAL
    assert enc.lib.flope_tf_stream_step_tracker(st.state, None, _lib.TF_FEED_MEAS, y.data_ptr(), sp) == _lib.EINVAL
    assert enc.lib.flope_tf_stream_step_assoc(st.state, None, None, None, 0, None, sp) == 0            # n = 0: a no-op
    assert st.step_assoc(x[:0], a[:0]).shape == (0, VEC[2])
    assert st.positions == [1, 1, 1, 0, 0, 0] and st.last_feed()[0].tolist() == [0, 1, 2]
    # opening: a window is needed, max_rows 1 .. max_tokens, the table's own refusals
    for kw, word in ((dict(window=0), "window"), (dict(window=4, max_rows=0), "max_rows"), (dict(window=4, max_rows=17), "max_rows"),
                     (dict(window=5), "window"), (dict(window=4, bias=torch.zeros(3)), "distances")):
        with pytest.raises(ValueError, match=word):
            enc.open_stream(SC.STREAM_TRACKS, 4, positions="device", **kw)
    with pytest.raises(ValueError, match="positions"):
        enc.open_stream(2, 4, window=4, positions="gpu")
    # input_dim < 7
    enc5 = _encoder((5, 30, 3, 5, 1, 20))
    st5 = enc5.open_stream(SC.STREAM_TRACKS, 4, window=4, positions="device", max_rows=8)
    with pytest.raises(ValueError, match="below 7"):
        st5.step_tracker(trk)
    assert st5.step_assoc(torch.randn(3, 5).cuda(), a).shape == (3, 3) and st5.positions == [1, 1, 1, 0, 0, 0]      # its own rows are welcome
    # weights not loaded
    from flope_amd.tf_encoder import TransformerEncoder
    bare = TransformerEncoder(*VEC, dtype="f32", max_tokens=16)
    stb = bare.open_stream(2, 4, window=4, positions="device")
    with pytest.raises(RuntimeError, match="weights"):
        stb.step_assoc(x[:2], a[:2])
    # a destroyed handle
    enc5.close()
    with pytest.raises(RuntimeError):
        st5.step_tracker(trk)
    assert enc5.lib.flope_tf_stream_step_assoc(st5.state, x.data_ptr(), a.data_ptr(), None, 3, y.data_ptr(), sp) == _lib.ESTATE
    assert enc5.lib.flope_tf_stream_read_positions(st5.state, None, 0) == _lib.ESTATE
    for o in (st5, stb, bare, small, st, twin, trk, enc):
        o.close()


# ---- 7. FlowerModel ------------------------------------------------------------------------------------------------------------------------
def test_flower_model_steps_the_stream_behind_the_tracker():
    from sunflower.predictor.flower_model import FlowerModel
    enc = _encoder(VEC)
    want = _f32_rows(6)
    want_feed, want_pos = SC.scenario_feed()
    st = enc.open_stream(SC.STREAM_TRACKS, 6, window=SC.WINDOW, positions="device", max_rows=SC.MAX_MEAS)
    fm = FlowerModel(dist_th=TC.TH_MM, tracker="device", track_stream=st)
    plain = FlowerModel(dist_th=TC.TH_MM, tracker="device")
    assert fm.track_rows is None and fm.track_feed is None and plain.track_stream is None
    for fr, w, (w_who, w_where) in zip(SC.scenario().frames, want, want_feed):
        poses = fr.poses[fr.rel != 0] if fr.rel is not None else fr.poses       # (add_poses takes a frame's reliable poses)
        if fr.rel is not None:
            keep = fr.rel != 0
            w, w_who, w_where = w[torch.from_numpy(keep)], w_who[keep], w_where[keep]
        for m in (fm, plain):
            m.add_poses(poses, fr.cam, ignore=True)
        assert fm.track_rows.is_cuda and torch.equal(_bits(fm.track_rows.cpu()), _bits(w))
        who, where = fm.track_feed
        assert who.tolist() == w_who.tolist() and where.tolist() == w_where.tolist()
        assert plain.track_rows is None and plain.track_feed is None
    assert st.positions == want_pos
    # without track_stream nothing changes: the tracker's state is the same, bit for bit
    a, b = fm.device_tracker.read(), plain.device_tracker.read()
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)) and len(a[3]) == SC.MAX_TRACKS
    fm.add_poses(None, SC.CAM, ignore=True)
    fm.add_poses(np.zeros((0, 4, 4)), SC.CAM, ignore=True)             # an empty frame is no update and no step
    assert st.positions == want_pos
    with pytest.raises(ValueError, match="device-positioned"):
        FlowerModel(tracker="device", track_stream=enc.open_stream(2, 4, window=4))
    for o in (fm.device_tracker, plain.device_tracker, st, enc):
        o.close()
