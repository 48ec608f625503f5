"""tests/tf_history_cases.py without a device: the walks tests/test_gpu_tf_history.py uses are legal under the model, the
pair walk holds every ordered pair of KINDS, every random walk holds every kind -- and the checker catches what it is for: check_walk
runs on a pure-Python fake handle whose calls are cheap deterministic functions of (options, arguments, own state), passes on it, and
fails at the right call under each of six deliberate leaks (LEAKS; the role MUTATIONS play in the bound files).
"""
import itertools
import zlib

import numpy as np
import pytest

import tf_history_cases as H

DTYPES = ("f32", "f32m", "f16", "bf16")
LEAKS = ("sticky_window", "sticky_lengths", "stale_rows", "shared_tab", "option_at_open", "freed_mask")


def _v(*key):
    """a finite value that depends on every part of the key"""
    return zlib.crc32(repr(key).encode()) / 2.0 ** 32 + 0.5


class _FakeState:
    def __init__(self, form, options, table):
        self.form = form
        self.tracks, self.capacity, self.window, self.device = H.STREAM_FORMS[form]
        self.pos = table if table is not None else [0] * 8      # leak shared_tab: the handle's one table
        self.hist = [[] for _ in range(self.tracks)]
        self.options_at_open = options


class FakeHandle:
    """The handle interface of tests/tf_history_cases.py in pure Python.  It has what the real one has: options, one workspace of
    MAX_TOKENS rows that every call writes its M rows into, the window and the offsets of the last call, states with a position table and
    their own tokens, masks.  Without a leak nothing of it reaches a result but through the call's own arguments."""
    made = 0

    def __init__(self, options, leak=None):
        FakeHandle.made += 1
        self.o, self.leak = dict(options), leak
        self.ws = np.zeros(H.MAX_TOKENS)
        self.window, self.offsets = 0, None
        self.states, self.masks, self.freed = {}, {}, None
        self.tab = [0] * 8

    def close(self):
        pass

    def _opts(self):
        return tuple(sorted(self.o.items()))

    def _run(self, values):
        """M rows through the workspace"""
        y = np.array(values, dtype=np.float64)
        M = len(y)
        if self.leak == "stale_rows":
            y[0] += self.ws[M:].sum()             # rows >= M are whatever an earlier, larger call left
        self.ws[:M] = y
        return y

    def _batch(self, tag, mode, B, L, seed, mid, ragged):
        window = H.WINDOW if mode == "window" else 0
        if self.leak == "sticky_window" and mode in ("fixed", "ragged", "causal"):
            window = self.window                  # a plain call keeps the previous call's window
        else:
            self.window = window
        lengths = H.lengths_of(B, L, seed) if ragged else (L,) * B
        if ragged:
            self.offsets = lengths
        elif self.leak == "sticky_lengths" and self.offsets is not None:
            lengths = tuple(min(L, self.offsets[b % len(self.offsets)]) for b in range(B))       # a fixed-length call reads the previous ragged offsets
        digest = self.masks[mid] if mode in ("mask", "bias") else None
        rows = self._run([_v(tag, self._opts(), mode, window, digest, seed, b, t, n) for b, n in enumerate(lengths) for t in range(n)])
        y = np.full((B, L), _v("bias"))
        at = 0
        for b, n in enumerate(lengths):
            y[b, :n] = rows[at:at + n]
            at += n
        return {"y": y, "finite": bool(np.isfinite(y).all())}

    def _token(self, s, t, token, options):
        """one token onto track t -> its row: a function of the options, the keys the token sees, and its position"""
        s.hist[t].append(token)
        seen = s.hist[t][-s.window:] if s.window else s.hist[t]
        v = float("nan") if "nan" in seen else _v("row", options, s.form, tuple(seen), s.pos[t])
        s.pos[t] += 1
        return v

    def _stream(self, s, y=None):
        out = {"positions": list(s.pos[:s.tracks]), "step_plan": "split" if self.o["step_split"] else "row"}
        if y is not None:
            out["y"], out["finite"] = y, bool(np.isfinite(y).all())
        return out

    def call(self, c):
        k = c[0]
        if k in H.FORWARDS:
            return self._batch("forward", k[len("forward_"):], c[1], c[2], c[3], c[4], H.is_ragged(c))
        if k == "attention":
            return self._batch("attention", c[1], c[2], c[3], c[4], c[5], H.is_ragged(c))
        if k in ("linear", "layernorm", "linear_ln_act"):
            rows = c[-2]
            y = self._run([_v(c, self._opts(), r) for r in range(rows)])
            return {"y": y, "finite": bool(np.isfinite(y).all())}
        if k == "open_stream":
            self.states[c[1]] = _FakeState(c[2], self._opts(), self.tab if self.leak == "shared_tab" else None)
            return self._stream(self.states[c[1]])
        if k in ("step", "extend", "prefill", "step_assoc") or (k == "poison" and c[1] == "prefill_reset"):
            s = self.states[c[2] if k == "poison" else c[1]]
            options = s.options_at_open if self.leak == "option_at_open" else self._opts()
            if k == "step":
                tracks = range(s.tracks) if c[2] is None else c[2]
                y = self._run([self._token(s, t, ("tok", c[3], r), options) for r, t in enumerate(tracks)])
                return self._stream(s, y)
            if k == "step_assoc":
                vals, fed, feed = [], set(), []
                for m, a in enumerate(c[2]):
                    t = -1 - a if a < 0 else a
                    if a == H.SKIP or t >= s.tracks or t in fed:
                        vals.append(_v("bias"))
                        feed.append(-1)
                        continue
                    if a < 0:
                        s.pos[t], s.hist[t] = 0, []
                    fed.add(t)
                    feed.append(t)
                    vals.append(self._token(s, t, ("tok", c[3], m), options))
                out = self._stream(s, self._run(vals))
                out["feed_tracks"] = np.array(feed)
                return out
            if k == "poison":
                tracks, lengths, toks = range(s.tracks), (min(s.capacity, 4),) * s.tracks, None
            else:
                tracks, lengths, toks = (range(s.tracks) if c[2] is None else c[2]), c[3], c[4]
            vals = []
            for b, (t, n) in enumerate(zip(tracks, lengths)):
                if k != "extend":
                    s.pos[t], s.hist[t] = 0, []
                vals += [self._token(s, t, "nan" if toks is None else ("tok", toks, b, j), options) for j in range(n)]
            y = self._run(vals)
            if k == "poison":
                for t in range(s.tracks):
                    s.pos[t], s.hist[t] = 0, []
                return {"nan": bool(np.isnan(y).all()), "positions": list(s.pos[:s.tracks])}
            return self._stream(s, y)
        if k == "reset":
            s = self.states[c[1]]
            for t in (range(s.tracks) if c[2] is None else c[2]):
                s.pos[t], s.hist[t] = 0, []
            return {"positions": list(s.pos[:s.tracks])}
        if k == "close":
            del self.states[c[1]]
            return {}
        if k in ("make_mask", "make_bias"):
            digest = _v(c[0], c[2], c[3])
            if self.leak == "freed_mask" and self.freed is not None:
                digest, self.freed = self.freed, None     # a closed mask's contents are used by the next one
            self.masks[c[1]] = digest
            return {"L": c[3], "allowed": int(1000 * _v("allowed", c[2], c[3]))}
        if k == "close_mask":
            self.freed = self.masks.pop(c[1])
            return {}
        if k == "set_option":
            old, self.o[c[1]] = self.o[c[1]], c[2]
            return {"old": old}
        if k == "poison":
            self.ws[:] = float("nan")
            return {"nan": True}
        assert k == "other_handle", c
        return {"y": np.array([_v("other", c[1])]), "finite": True}


def _make(leak=None):
    return lambda options: FakeHandle(options, leak)


# ---- the walks ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_the_pair_walk_is_legal_and_holds_every_ordered_pair(dtype):
    walk = H.pair_walk(None, dtype)
    H.check_legal(walk, dtype)
    want = set(itertools.product(H.KINDS, H.KINDS))
    have = H.pairs_of(walk) & want
    print(f"pair_walk[{dtype}]: {len(walk)} calls, {len(have)} of {len(want)} ordered pairs of {len(H.KINDS)} kinds ({100.0 * len(have) / len(want):.0f} %)")
    assert have == want, sorted(want - have)[:5]
    assert walk == H.pair_walk(None, dtype)                      # deterministic
    assert all(isinstance(hash(c), int) and repr(c) for c in walk)


@pytest.mark.parametrize("dtype", H.RANDOM_DTYPES)
@pytest.mark.parametrize("seed", H.RANDOM_SEEDS)
def test_every_random_walk_is_legal_and_holds_every_kind(seed, dtype):
    walk = H.random_walk(seed, H.RANDOM_CALLS, dtype)
    H.check_legal(walk, dtype)
    assert len(walk) == H.RANDOM_CALLS and {H.kind_of(c) for c in walk} == set(H.KINDS)
    assert walk == H.random_walk(seed, H.RANDOM_CALLS, dtype) and walk != H.random_walk(seed + 10, H.RANDOM_CALLS, dtype)


def test_the_walks_interleave_states_and_keep_replays_short():
    walk = H.pair_walk(None, "f16")
    m, most, interleaved, forms = H.Model("f16"), 0, 0, set()
    last = None
    for c in walk:
        sid = m.stream_of(c)
        if sid is not None and c[0] in ("step", "extend", "prefill", "step_assoc"):
            interleaved += last is not None and last != sid and last in m.states
            last = sid
        m.apply(c)
        most = max(most, len(m.states))
        forms |= {s.form for s in m.states.values()}
    assert most == 3 and interleaved > 20 and forms == set(H.STREAM_FORMS)
    assert {c[1] for c in walk if c[0] == "set_option"} == set(H.OPTION_NAMES)
    assert {c[1] for c in walk if c[0] == "attention"} == set(H.ATTN_MODES) and {c[1] for c in walk if c[0] == "linear"} == set(H.LINEAR_FORMS)
    assert {c[1] for c in walk if c[0] == "poison"} == {"forward", "prefill_reset"}
    assert {(c[1], c[2]) for c in walk if c[0] in H.FORWARDS} == set(H.BL) and {c[2] for c in walk if c[0] == "linear"} == set(H.ROWS)
    assert any(c[0] == "reset" and c[2] is not None for c in walk) and any(c[0] == "reset" and c[2] is None for c in walk)


def test_the_model_refuses_what_the_generators_must_not_emit():
    m = H.Model("f16")
    for c in (("open_stream", 0, "linear"), ("make_mask", 0, "random", 33)):
        m.apply(c)
    for _ in range(8):
        m.apply(("step", 0, None, 0))
    refused = [("step", 0, None, 0), ("extend", 0, (1,), (1,), 0), ("step", 1, None, 0), ("step_assoc", 0, (0,), 0), ("open_stream", 0, "window"),
               ("open_stream", 1, "device"), ("forward_mask", 2, 33, 0, 1), ("forward_bias", 2, 33, 0, 0), ("forward_mask", 3, 50, 0, 0),
               ("close_mask", 1), ("make_bias", 0, "alibi", 33), ("set_option", "attn_tiled", 3), ("set_option", "nothing", 1),
               ("linear_ln_act", 0, 1, 0), ("reset", 0, (0, 0)), ("step", 0, (3,), 0), ("close", 2)]
    for c in refused:
        with pytest.raises(H.Illegal):
            m.check(c)
    m.apply(("reset", 0, (1,)))
    m.check(("step", 0, (1,), 0))
    with pytest.raises(H.Illegal):
        m.check(("step", 0, (0, 1), 0))
    m.apply(("close", 0))
    m.apply(("close_mask", 0))
    for c in (("step", 0, None, 0), ("forward_mask", 2, 33, 0, 0)):
        with pytest.raises(H.Illegal):
            m.check(c)


def test_a_snapshot_holds_the_options_in_force_and_the_state_s_own_calls():
    m = H.Model("f32m")
    assert dict(m.snapshot(("layernorm", 1, 0)).options)["f32mfma"] == 1 and dict(H.Model("f32").snapshot(("layernorm", 1, 0)).options)["f32mfma"] == 0
    walk = [("open_stream", 0, "window"), ("open_stream", 1, "linear"), ("step", 0, None, 1), ("set_option", "step_split", 1), ("step", 1, None, 2),
            ("step", 0, (1,), 3)]
    for c in walk:
        m.apply(c)
    s = m.snapshot(("step", 0, None, 4))
    assert [p[0] for p in s.replay] == [walk[0], walk[2], walk[5]]              # its own calls, none of state 1's
    assert [dict(p[1])["step_split"] for p in s.replay] == [0, 0, 1] and dict(s.options)["step_split"] == 1
    m.apply(("reset", 0, (0,)))
    assert len(m.snapshot(("step", 0, None, 4)).replay) == 4                    # a reset of some tracks is one more call of the state
    m.apply(("reset", 0, None))
    assert m.snapshot(("step", 0, None, 4)).replay == (s.replay[0],) and m.positions(0) == [0, 0, 0, 0]
    m.apply(("make_bias", 1, "alibi", 50))
    assert m.snapshot(("forward_bias", 3, 50, 0, 1)).mask == ("make_bias", 1, "alibi", 50) and m.snapshot(("forward_fixed", 3, 50, 0, None)).mask is None


# ---- the checker on the fake handle ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ("f16", "f32m"))
def test_the_fake_handle_passes_every_walk(dtype):
    memo = {}
    walk = H.pair_walk(None, dtype)
    stats = H.check_walk(_make(), walk, dtype, memo)
    assert stats["calls"] == len(walk) and stats["checked"] == sum(1 for c in walk if c[0] not in H.NO_RESULT)
    assert stats["kinds"] == set(H.KINDS) and stats["options"] == set(H.OPTION_NAMES)
    for seed in H.RANDOM_SEEDS:
        walk = H.random_walk(seed, H.RANDOM_CALLS, dtype)
        assert H.check_walk(_make(), walk, dtype, memo)["checked"] == sum(1 for c in walk if c[0] not in H.NO_RESULT)


def test_the_oracle_is_a_fresh_handle_and_a_memoised_value_came_from_one():
    walk = (("forward_fixed", 2, 33, 0, None), ("set_option", "skinny", 1), ("forward_fixed", 2, 33, 0, None), ("set_option", "skinny", 0),
            ("forward_fixed", 2, 33, 0, None))
    memo = {}
    FakeHandle.made = 0
    H.check_walk(_make(), walk, "f16", memo)
    assert FakeHandle.made == 1 + 4               # the walked one; a fresh one per (call, options in force): the last forward is the first's
    snaps = H.check_legal(walk)
    assert snaps[0] == snaps[4] != snaps[2] and (walk[0], snaps[0]) in memo and (walk[2], snaps[2]) in memo
    seen = []

    def make(options):
        seen.append(dict(options))
        return FakeHandle(options)
    H.expected(walk[2], snaps[2], make)
    assert len(seen) == 1 and seen[0]["skinny"] == 1 and sum(seen[0].values()) == 1


# leak -> (the shortest walk that shows it, the index of the call that must differ)
REDUCED = {
    "sticky_window": ((("forward_window", 2, 33, 0, None), ("forward_fixed", 2, 33, 0, None)), 1),
    "sticky_lengths": ((("forward_ragged", 3, 50, 1, None), ("layernorm", 1, 0), ("forward_fixed", 3, 50, 1, None)), 2),
    "stale_rows": ((("linear", "in_proj", 33, 0), ("linear", "in_proj", 1, 0)), 1),
    "shared_tab": ((("open_stream", 0, "window"), ("open_stream", 1, "alibi"), ("step", 0, None, 0), ("step", 1, None, 0)), 3),
    "option_at_open": ((("open_stream", 0, "linear"), ("step", 0, None, 0), ("set_option", "step_split", 1), ("step", 0, None, 1)), 3),
    "freed_mask": ((("make_mask", 2, "random", 33), ("forward_mask", 2, 33, 0, 2), ("close_mask", 2), ("make_mask", 2, "edge", 33),
                    ("forward_mask", 2, 33, 0, 2)), 4),
}


@pytest.mark.parametrize("leak", LEAKS)
def test_each_leak_fails_at_the_call_that_reads_it(leak):
    walk, index = REDUCED[leak]
    H.check_legal(walk)
    assert H.check_walk(_make(), walk)["calls"] == len(walk)                     # the same walk passes without the leak
    with pytest.raises(H.HistoryError) as err:
        H.check_walk(_make(), walk, walked=_make(leak))
    e = err.value
    assert (e.index, e.call, e.previous) == (index, walk[index], walk[index - 1]), str(e)
    assert "differ" in str(e) or "against" in str(e)
    # ... and in the pair walk, and in one random walk at least, with the walked handle leaking and the oracle's handles sound
    long = H.pair_walk(None, "f16")
    with pytest.raises(H.HistoryError) as err:
        H.check_walk(_make(), long, walked=_make(leak))
    assert 0 < err.value.index < len(long) and err.value.call == long[err.value.index]
    caught = 0
    for seed in H.RANDOM_SEEDS:
        try:
            H.check_walk(_make(), H.random_walk(seed, H.RANDOM_CALLS, "f16"), walked=_make(leak))
        except H.HistoryError:
            caught += 1
    assert caught >= 1


def test_a_value_that_is_not_finite_behind_a_poison_is_reported_even_where_the_oracle_agrees():
    walk = (("poison", "forward", None), ("layernorm", 17, 0))
    H.check_walk(_make(), walk)

    class Nan(FakeHandle):
        def call(self, c):
            out = super().call(c)
            if c[0] == "layernorm":
                out["finite"] = False
            return out
    with pytest.raises(H.HistoryError, match="not finite") as err:
        H.check_walk(lambda options: Nan(options), walk)
    assert err.value.index == 1
    with pytest.raises(H.HistoryError) as err:                                   # the poison reaches the next call through the stale rows
        H.check_walk(_make(), walk, walked=_make("stale_rows"))
    assert err.value.index == 1


def test_differences_counts_elements_and_names_records():
    a = {"y": np.arange(6, dtype=np.float32).reshape(2, 3), "kernel": 3}
    b = {"y": a["y"].copy(), "kernel": 5}
    b["y"][1, 2] = np.float32(5.0000005)
    b["y"][0, 0] = -0.0                           # equal as numbers, not in bits
    lines = H.differences(a, b)
    assert lines == ["kernel: 3 against the oracle's 5", "y: 2 of 6 elements differ in bits"], lines
    assert H.differences(a, dict(a)) == [] and H.differences(a, {"y": a["y"]}) != []
    nan = {"y": np.array([np.nan], dtype=np.float32)}
    assert H.differences(nan, {"y": nan["y"].copy()}) == []


# ---- the options in force over the walks -----------------------------------------------------------------------------------------------------
def _in_force(walk, dtype):
    """-> (checked calls, checked calls per option that is on, checked calls with generic = 0, ordered pairs whose B ran with generic = 0
    behind an A that ran with generic = 0)"""
    m, on, checked, plain, pairs, before = H.Model(dtype), dict.fromkeys(H.OPTION_NAMES, 0), 0, 0, set(), None
    for c in walk:
        generic = m.options["generic"]
        if c[0] not in H.NO_RESULT:
            checked += 1
            plain += not generic
            for name in H.OPTION_NAMES:
                on[name] += bool(m.options[name])
        if before is not None and not generic and not before[1]:
            pairs.add((before[0], c[0]))
        before = (c[0], generic)
        m.apply(c)
    return checked, on, plain, pairs


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_dtype_s_own_kernels_are_in_force_for_the_checked_pairs(dtype):
    """"generic" = 1 switches the 16-bit MFMA kernels, tf_cast_pad and the skinny linears off, so it is a short excursion: nearly every
    checked call and all but a few ordered pairs run with it off, and every other option is on for a good part of every walk"""
    want = set(itertools.product(H.KINDS, H.KINDS))
    walks = [("pair", H.pair_walk(None, dtype))]
    if dtype in H.RANDOM_DTYPES:
        walks += [(f"random {seed}", H.random_walk(seed, H.RANDOM_CALLS, dtype)) for seed in H.RANDOM_SEEDS]
    for what, walk in walks:
        checked, on, plain, pairs = _in_force(walk, dtype)
        print(f"{dtype} {what}: {checked} checked calls, {plain} with generic = 0, {len(pairs & want)} ordered pairs wholly with generic = 0; on: {on}")
        assert plain >= 0.96 * checked, (what, plain, checked)
        for name in H.OPTION_NAMES:
            if name == "generic":
                assert 1 <= on[name] <= 0.04 * checked, (what, name, on[name])
            elif name == "f32mfma" and dtype == "f32m":
                assert on[name] >= 0.6 * checked, (what, name, on[name])
            else:
                assert on[name] >= 0.2 * checked, (what, name, on[name], checked)
        if what == "pair":
            missing = want - pairs
            assert len(missing) <= 6 and all("set_option" in p for p in missing), sorted(missing)
            m = H.Model(dtype)
            homes = {tuple(sorted(h.items())) for h in H.regimes(dtype)}
            seen = {k: set() for k in H.KINDS}                 # kind -> the regimes it ran under as it stood in the walk
            for c in walk:
                seen[c[0]].add(tuple(sorted(m.options.items())))
                m.apply(c)
            assert all(len(seen[k] & homes) == 3 for k in H.KINDS if k != "linear_ln_act"), {k: len(v & homes) for k, v in seen.items()}
