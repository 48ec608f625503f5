"""The cases of the encoder's history tests, shared by tests/test_tf_history_host.py and tests/test_gpu_tf_history.py.

The invariant: the result of a call depends on the weights, the options in force at the call, the call's arguments and, for a stream
state, that state's own earlier calls -- on nothing else that ever happened on the handle, on its other states, on its masks, or on
other handles.  Every kernel is deterministic, so the comparison is equality of bits and of integers; there is no tolerance here.

This file needs no device.  It holds
  * call descriptors: plain hashable tuples, (kind, ...), listed in KINDS;
  * Model: a small model of the handle -- option values, open states (form, tracks, capacity, per-track positions, their own calls
    since the last full reset), live masks -- that says which calls are legal and what is in force at a call (Model.snapshot);
  * pair_walk / random_walk: the two generators, which emit legal calls only;
  * expected: the oracle -- the call alone on a fresh handle made with exactly the options in force, for a stream call behind the
    state's own calls replayed under the options each was made with;
  * check_walk: walks one handle and compares every result-bearing call with the oracle.

A handle is anything with call(descriptor) -> dict of named results (arrays compare by their bytes, everything else by ==) and
close(); make_handle(options: dict) makes a fresh one.  tests/test_gpu_tf_history.py wraps flope_amd.TransformerEncoder that way,
tests/test_tf_history_host.py a pure-Python fake with deliberate leaks.

Two deliberate choices of the model.  A state's replay list starts again at a reset of all its tracks (TransformerEncoderStream.reset:
"their stale cache rows are never read"), so the oracle also holds the library to that sentence and a replay stays under a dozen calls.
linear_ln_act is emitted on every handle behind generic = 0, skinny = skinny_ln = 1; a handle whose linear_ln_plan says it has no such
launch (float32) refuses it with ValueError, and only there is that refusal the result both sides must give.
The generators keep one of three option sets in force (regimes) and treat a set_option call as a short excursion, so that the dtype's
own kernels, not the generic ones, are in force for the checked pairs; tests/test_tf_history_host.py counts it.
"""
import itertools
import random
import zlib
from collections import namedtuple

import numpy as np
import torch

KINDS = ("forward_fixed", "forward_ragged", "forward_causal", "forward_window", "forward_mask", "forward_bias",
         "attention", "linear", "layernorm", "linear_ln_act",
         "open_stream", "step", "extend", "prefill", "reset", "step_assoc", "close",
         "make_mask", "make_bias", "close_mask", "set_option", "poison", "other_handle")
NO_RESULT = ("close", "close_mask")                   # everything else bears a result and is checked
FORWARDS = KINDS[:6]

# the run-time options set_option flips, with the values it walks through; "causal" and "window" are stated per call by the wrapper and
# are part of the descriptor (forward_causal / forward_window, attention's modes)
OPTION_VALUES = {"generic": (0, 1), "f32mfma": (0, 1), "attn_tiled": (0, 1, 2), "fused": (0, 1), "window_mfma": (0, 1), "mask_mfma": (0, 1),
                 "bias_mfma": (0, 1), "step_split": (0, 1), "skinny": (0, 1), "skinny_ln": (0, 1), "extend_mfma": (0, 1), "f32mlds": (0, 96)}
OPTION_NAMES = tuple(OPTION_VALUES)
PER_CALL_OPTIONS = {"causal": "forward_causal", "window": "forward_window"}      # option -> the kind that exercises it
WINDOW = 4
MAX_TOKENS = 256

BL = ((1, 1), (2, 33), (3, 50))
ROWS = (1, 17, 33)
LN_ROWS = (1, 17, 32)                                 # linear_ln_act: the skinny launch takes up to 32 rows
ATTN_MODES = ("fixed", "ragged", "causal", "window", "mask", "bias")
LINEAR_FORMS = ("embedding", "in_proj", "out_proj", "linear1", "linear2")
LN_ACT_FORMS = (("layers.0.linear1", "relu"), ("layers.1.in_proj", None), ("layers.0.linear1", "gelu"))
MASK_KINDS = ("random", "edge")                       # tests/tf_attn_mask_bound.py's
BIAS_KINDS = ("holes", "alibi", "edge")               # tests/tf_attn_bias_bound.py's, one plane per head
# form -> (tracks, capacity, window, device positions)
STREAM_FORMS = {"linear": (3, 8, 0, False), "window": (4, 6, WINDOW, False), "alibi": (5, 8, WINDOW, False), "device": (3, 8, WINDOW, True)}
HOST_FORMS = ("linear", "window", "alibi")
MAX_ROWS = 8                                          # a device-positioned state's max_rows
SKIP = -2 ** 31


def _o(t):
    return -1 - t


# hand-built associations for a device-positioned state of 3 tracks: rows that open, match, repeat a track, name one out of range, skip
ASSOCS = ((_o(0), _o(1), _o(0), 7, SKIP), (1, 1, 0, 0, _o(2)), (0, SKIP, 2, 1, 1, 6), (_o(2), 0, 1, 9, 2), (0, 1), (2,))
HOST_SLOTS, DEVICE_SLOT = (0, 1), 2
MASK_SLOTS = (2, 0, 1)
RANDOM_SEEDS, RANDOM_CALLS, RANDOM_DTYPES = (1, 2, 3), 150, ("f16", "f32m")      # the random walks tests/test_gpu_tf_history.py runs
MAX_REPLAY = 8                                        # a state's own calls since its last full reset, before the generators reset it

Snapshot = namedtuple("Snapshot", "options replay mask")     # options: ((name, value), ...); replay: ((descriptor, options), ...) or None; mask: its make descriptor or None


def kind_of(call):
    return call[0]


def is_ragged(call):
    """whether a forward / attention descriptor carries lengths"""
    k = call[0]
    if k == "forward_fixed":
        return False
    if k == "forward_ragged":
        return True
    if k == "attention":
        return call[1] == "ragged" or (call[1] != "fixed" and call[4] % 2 == 1)
    return call[3] % 2 == 1


def lengths_of(B, L, seed):
    """the lengths of a ragged batch: 1 .. L each, the first sequence full so that the batch keeps its L"""
    r = random.Random(seed * 7919 + B * 131 + L)
    return tuple([L] + [r.randint(1, L) for _ in range(B - 1)])


def randn(shape, *key):
    """standard normal float32 from the call's own seed"""
    g = torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))
    return torch.randn(*shape, generator=g)


def default_options(dtype):
    o = {k: 0 for k in OPTION_NAMES}
    if dtype == "f32m":
        o["f32mfma"] = 1
    return o


def regimes(dtype):
    """The option sets the generators keep in force, one after the other: the defaults (the packed MFMA linear, the resident MFMA
    attention, the dtype's f32mfma); every option that picks another kernel on; a mix (attn_tiled = 2, skinny without skinny_ln, the
    other f32mfma).  "generic" is 0 in all three: set_option flips it, like every other option, for one short excursion that the
    generators state back, so the dtype's own kernels are in force for nearly every checked call."""
    base = default_options(dtype)
    on = dict(base, attn_tiled=1, fused=1, window_mfma=1, mask_mfma=1, bias_mfma=1, step_split=1, skinny=1, skinny_ln=1, extend_mfma=1, f32mlds=96)
    mixed = dict(base, attn_tiled=2, fused=1, window_mfma=1, mask_mfma=1, skinny=1, extend_mfma=1, f32mfma=1 - base["f32mfma"])
    return base, on, mixed


def _freeze(options):
    return tuple(sorted(options.items()))


class Illegal(Exception):
    pass


class _State:
    def __init__(self, form, open_call, options):
        self.form = form
        self.tracks, self.capacity, self.window, self.device = STREAM_FORMS[form]
        self.pos = None if self.device else [0] * self.tracks
        self.open = (open_call, options)
        self.hist = []

    def room(self, t):
        return 10 ** 6 if self.window else self.capacity - self.pos[t]


class Model:
    """What the generators and the checker know of a handle: enough to emit legal calls only and to say what is in force at a call."""

    def __init__(self, dtype="f16"):
        self.dtype = dtype
        self.options = default_options(dtype)
        self.states = {}                  # sid -> _State
        self.masks = {}                   # mid -> its make descriptor

    # ---- legality ----------------------------------------------------------------------------------------------------------------
    def _state(self, sid, host=None):
        if sid not in self.states:
            raise Illegal(f"state {sid} is not open")
        s = self.states[sid]
        if host is True and s.device:
            raise Illegal(f"state {sid} is device-positioned: step_assoc only")
        if host is False and not s.device:
            raise Illegal(f"state {sid} is host-positioned")
        return s

    def _mask(self, mid, want):
        if mid not in self.masks:
            raise Illegal(f"mask {mid} is not live")
        if self.masks[mid][0] != want:
            raise Illegal(f"mask {mid} was made by {self.masks[mid][0]}")
        return self.masks[mid]

    def check(self, call):
        """Illegal unless `call` is a legal call now"""
        k = call[0]
        if k not in KINDS:
            raise Illegal(f"unknown kind {k!r}")
        if k in FORWARDS or k == "attention":
            mode = call[1] if k == "attention" else k[len("forward_"):]
            B, L, seed, mid = call[-4:]
            if (B, L) not in BL:
                raise Illegal(f"(B, L) = {(B, L)}")
            if mode in ("mask", "bias"):
                if self._mask(mid, "make_" + mode)[3] != L:
                    raise Illegal(f"mask {mid} was made for L = {self.masks[mid][3]}, the call has {L}")
                if self.masks[mid][2] == "edge" and is_ragged(call):
                    raise Illegal("a shorter sequence under the edge mask has a row without an allowed key: refused")
            elif mid is not None:
                raise Illegal("a mask slot on a call without a mask")
            if B * L > MAX_TOKENS:
                raise Illegal("more than max_tokens rows")
        elif k == "linear":
            if call[1] not in LINEAR_FORMS or not 1 <= call[2] <= MAX_TOKENS:
                raise Illegal(str(call))
        elif k == "linear_ln_act":
            if not (self.options["skinny"] and self.options["skinny_ln"]) or self.options["generic"] or not 1 <= call[2] <= 32:
                raise Illegal("linear_ln_act needs skinny = skinny_ln = 1, generic = 0 and 1 .. 32 rows")
        elif k == "open_stream":
            sid, form = call[1], call[2]
            if sid in self.states:
                raise Illegal(f"state {sid} is open")
            if (form == "device") != (sid == DEVICE_SLOT) or form not in STREAM_FORMS:
                raise Illegal(f"form {form} in slot {sid}")
            if len(self.states) >= 3:
                raise Illegal("three states are open")
        elif k == "step":
            s = self._state(call[1], host=True)
            for t in self._tracks(s, call[2]):
                if s.room(t) < 1:
                    raise Illegal(f"track {t} of state {call[1]} is full")
        elif k in ("extend", "prefill"):
            s = self._state(call[1], host=True)
            tracks, lengths = self._tracks(s, call[2]), call[3]
            if len(tracks) != len(lengths) or min(lengths) < 1:
                raise Illegal(str(call))
            for t, n in zip(tracks, lengths):
                if (s.room(t) if k == "extend" else (10 ** 6 if s.window else s.capacity)) < n:
                    raise Illegal(f"track {t} of state {call[1]} has no room for {n}")
            if len(tracks) * max(lengths) > MAX_TOKENS:
                raise Illegal("more than max_tokens rows")
        elif k == "reset":
            s = self._state(call[1])
            if s.device and call[2] is not None:
                raise Illegal("a device-positioned state resets all its tracks")
            if call[2] is not None:
                self._tracks(s, call[2])
        elif k == "step_assoc":
            self._state(call[1], host=False)
            if not 1 <= len(call[2]) <= MAX_ROWS:
                raise Illegal("rows outside 1 .. max_rows")
        elif k == "close":
            self._state(call[1])
        elif k in ("make_mask", "make_bias"):
            if call[1] in self.masks:
                raise Illegal(f"mask {call[1]} is live")
            if call[3] not in [L for _, L in BL] or call[2] not in (MASK_KINDS if k == "make_mask" else BIAS_KINDS):
                raise Illegal(str(call))
        elif k == "close_mask":
            if call[1] not in self.masks:
                raise Illegal(f"mask {call[1]} is not live")
        elif k == "set_option":
            if call[1] not in OPTION_VALUES or call[2] not in OPTION_VALUES[call[1]]:
                raise Illegal(f"option {call[1]} = {call[2]} would be refused")
        elif k == "poison":
            if call[1] == "prefill_reset":
                self._state(call[2], host=True)
            elif call[1] != "forward":
                raise Illegal(str(call))

    @staticmethod
    def _tracks(s, tracks):
        tracks = tuple(range(s.tracks)) if tracks is None else tuple(tracks)
        if len(set(tracks)) != len(tracks) or not tracks or min(tracks) < 0 or max(tracks) >= s.tracks:
            raise Illegal(f"tracks {tracks} of a state of {s.tracks}")
        return tracks

    # ---- what is in force ----------------------------------------------------------------------------------------------------------
    def stream_of(self, call):
        k = call[0]
        if k in ("open_stream", "step", "extend", "prefill", "reset", "step_assoc", "close"):
            return call[1]
        if k == "poison" and call[1] == "prefill_reset":
            return call[2]
        return None

    def snapshot(self, call):
        """what the oracle needs beside the call: the options in force, the state's own calls so far, the mask the call names"""
        sid = self.stream_of(call)
        replay = None
        if sid is not None and call[0] != "open_stream":
            s = self.states[sid]
            replay = (s.open,) + tuple(s.hist)
        elif call[0] == "open_stream":
            replay = ()
        mask = self.masks.get(call[-1]) if (call[0] in FORWARDS or call[0] == "attention") and call[-1] is not None else None
        return Snapshot(_freeze(self.options), replay, mask)

    def positions(self, sid):
        """per-track positions of a host-positioned state (None for a device-positioned one: only the device knows)"""
        s = self.states[sid]
        return None if s.device else list(s.pos)

    # ---- the call's effect ---------------------------------------------------------------------------------------------------------
    def apply(self, call):
        self.check(call)
        k = call[0]
        here = (call, _freeze(self.options))
        if k == "open_stream":
            self.states[call[1]] = _State(call[2], call, _freeze(self.options))
        elif k == "close":
            del self.states[call[1]]
        elif k in ("make_mask", "make_bias"):
            self.masks[call[1]] = call
        elif k == "close_mask":
            del self.masks[call[1]]
        elif k == "set_option":
            self.options[call[1]] = call[2]
        elif k == "step":
            s = self.states[call[1]]
            for t in self._tracks(s, call[2]):
                s.pos[t] += 1
            s.hist.append(here)
        elif k in ("extend", "prefill"):
            s = self.states[call[1]]
            for t, n in zip(self._tracks(s, call[2]), call[3]):
                s.pos[t] = s.pos[t] + n if k == "extend" else n
            s.hist.append(here)
        elif k == "step_assoc":
            self.states[call[1]].hist.append(here)
        elif k == "reset" or (k == "poison" and call[1] == "prefill_reset"):
            s = self.states[call[1] if k == "reset" else call[2]]
            tracks = None if k == "poison" else call[2]
            if tracks is None or len(tracks) == s.tracks:
                s.hist = []                       # a reset of every track: the replay list starts again (module docstring)
                if not s.device:
                    s.pos = [0] * s.tracks
            else:
                for t in tracks:
                    s.pos[t] = 0
                s.hist.append(here)


# ---- the generators ------------------------------------------------------------------------------------------------------------------
class _Gen:
    """Emits calls into `walk` through a Model, so that nothing illegal can be emitted; `ensure_*` emit the calls a kind needs first."""

    def __init__(self, dtype, seed):
        self.m = Model(dtype)
        self.r = random.Random(seed)
        self.walk = []
        self.n = 0                                # a counter the rotating choices read
        self.forms = itertools.cycle(HOST_FORMS)
        self.optnames = itertools.cycle(OPTION_NAMES)
        self.home = dict(self.m.options)          # the regime in force (regimes): normalize() states it again
        self.away = 0                             # calls since an option last left the regime

    def normalize(self):
        for name in OPTION_NAMES:
            if self.m.options[name] != self.home[name]:
                self.emit(("set_option", name, self.home[name]))

    def emit(self, call):
        self.m.apply(call)
        self.walk.append(call)

    # -- resources: ("s", sid) a stream slot, ("m", mid) a mask slot; a tag says what lives there: "host", "device", "mask", "bias", None
    def tag(self, res):
        t, i = res
        if t == "s":
            return None if i not in self.m.states else ("device" if self.m.states[i].device else "host")
        return None if i not in self.m.masks else self.m.masks[i][0][len("make_"):]

    def open_res(self, res, tag):
        t, i = res
        self.n += 1
        if t == "s":
            self.emit(("open_stream", i, "device" if i == DEVICE_SLOT else next(self.forms)))
        elif tag == "bias":
            self.emit(("make_bias", i, BIAS_KINDS[self.n % len(BIAS_KINDS)], BL[self.n % 3][1]))
        else:
            self.emit(("make_mask", i, MASK_KINDS[self.n % len(MASK_KINDS)], BL[self.n % 3][1]))

    def close_res(self, res):
        self.emit(("close", res[1]) if res[0] == "s" else ("close_mask", res[1]))

    def ensure(self, res, need):
        """need: "free", "any", or a tag"""
        cur = self.tag(res)
        if need == "free":
            if cur is not None:
                self.close_res(res)
        elif need == "any":
            if cur is None:
                self.open_res(res, self.default_tag(res))
        elif cur != need:
            if cur is not None:
                self.close_res(res)
            self.open_res(res, need)

    def ensure_room(self, sid):
        """a state the next calls use has room for them and a short replay list"""
        s = self.m.states.get(sid)
        if s is None:
            return
        if len(s.hist) >= MAX_REPLAY or (not s.device and not s.window and max(s.pos) > s.capacity - 4):
            self.emit(("reset", sid, None))

    # -- what a kind needs and leaves: (resource type, candidates, need, gives); gives "same" keeps the tag, a callable takes the slot
    def needs(self, kind, variant):
        if kind == "open_stream":
            return "s", (0, 1, 2), "free", lambda i: "device" if i == DEVICE_SLOT else "host"
        if kind in ("step", "extend", "prefill") or (kind == "poison" and variant % 2 == 1):
            return "s", HOST_SLOTS, "host", "same"
        if kind == "step_assoc":
            return "s", (DEVICE_SLOT,), "device", "same"
        if kind == "reset":
            return "s", (0, 1, 2), "any", "same"
        if kind == "close":
            return "s", (0, 1, 2), "any", None
        if kind in ("make_mask", "make_bias"):
            return "m", MASK_SLOTS, "free", lambda i, k=kind: k[len("make_"):]
        if kind == "close_mask":
            return "m", MASK_SLOTS, "any", None
        mode = ATTN_MODES[variant % len(ATTN_MODES)] if kind == "attention" else kind[len("forward_"):] if kind in FORWARDS else None
        if mode in ("mask", "bias"):
            return "m", MASK_SLOTS, mode, "same"
        return None

    def build(self, kind, variant, slot, avoid=()):
        """the descriptor of a call of `kind` on `slot` under the model as it stands"""
        r, m = self.r, self.m
        seed = r.randrange(4)
        if kind in FORWARDS or kind == "attention":
            mode = ATTN_MODES[variant % len(ATTN_MODES)] if kind == "attention" else kind[len("forward_"):]
            if mode in ("mask", "bias"):
                if m.masks[slot][2] == "edge":
                    seed &= ~1                    # fixed-length only: row 0 of the edge mask allows key L - 1 alone
                L = m.masks[slot][3]
                B = dict((l, b) for b, l in BL)[L]
            else:
                B, L = BL[r.randrange(3)]
                slot = None
            return (kind, mode, B, L, seed, slot) if kind == "attention" else (kind, B, L, seed, slot)
        if kind == "linear":
            return (kind, LINEAR_FORMS[variant % len(LINEAR_FORMS)], ROWS[r.randrange(3)], seed)
        if kind == "layernorm":
            return (kind, ROWS[r.randrange(3)], seed)
        if kind == "linear_ln_act":
            return (kind, variant % len(LN_ACT_FORMS), LN_ROWS[r.randrange(3)], seed)
        if kind == "open_stream":
            return (kind, slot, "device" if slot == DEVICE_SLOT else next(self.forms))
        if kind in ("step", "extend", "prefill", "reset"):
            s = m.states[slot]
            tracks = None
            if r.random() < 0.6 and not s.device:
                tracks = tuple(sorted(r.sample(range(s.tracks), r.randint(1, s.tracks))))
            if kind == "step":
                return (kind, slot, tracks, seed)
            if kind == "reset":
                return (kind, slot, tracks)
            ts = tuple(range(s.tracks)) if tracks is None else tracks
            top = (lambda t: min(3, s.room(t))) if kind == "extend" else (lambda t: s.capacity + 1 if s.window else s.capacity - 3)
            return (kind, slot, tracks, tuple(r.randint(1, top(t)) for t in ts), seed)
        if kind == "step_assoc":
            return (kind, slot, ASSOCS[variant % len(ASSOCS)], seed)
        if kind == "close":
            return (kind, slot)
        if kind in ("make_mask", "make_bias"):
            kinds = MASK_KINDS if kind == "make_mask" else BIAS_KINDS
            return (kind, slot, kinds[variant % len(kinds)], BL[r.randrange(3)][1])
        if kind == "close_mask":
            return (kind, slot)
        if kind == "set_option":
            name = next(self.optnames)
            while name in avoid:
                name = next(self.optnames)
            vals = OPTION_VALUES[name]
            return (kind, name, vals[(vals.index(m.options[name]) + 1) % len(vals)])
        if kind == "poison":
            return (kind, "prefill_reset", slot) if variant % 2 == 1 else (kind, "forward", None)
        assert kind == "other_handle", kind
        return (kind, seed)

    def prepare_options(self, kind):
        if kind == "linear_ln_act":
            for name, value in (("generic", 0), ("skinny", 1), ("skinny_ln", 1)):
                if self.m.options[name] != value:
                    self.emit(("set_option", name, value))
                    self.away = 0

    @staticmethod
    def default_tag(res):
        t, i = res
        return ("device" if i == DEVICE_SLOT else "host") if t == "s" else ("bias" if i == 1 else "mask")

    def leaves(self, need, slot):
        """the tag a call with these needs leaves in `slot` once its own need has been ensured"""
        res = (need[0], slot)
        if callable(need[3]):
            return need[3](slot)
        if need[3] is None:
            return None
        return (self.tag(res) or self.default_tag(res)) if need[2] == "any" else need[2]

    def pair(self, A, B, idx):
        """the calls that make (A, B) legal, then A, then B directly behind it"""
        va, vb = idx, idx // 3 + 1
        na, nb = self.needs(A, va), self.needs(B, vb)
        ca = [None] if na is None else list(na[1])
        cb = [None] if nb is None else list(nb[1])
        ca, cb = ca[idx % len(ca):] + ca[:idx % len(ca)], cb[(idx // 2) % len(cb):] + cb[:(idx // 2) % len(cb)]
        choice = None
        for ta, tb in itertools.product(ca, cb):
            if na is None or nb is None or na[0] != nb[0] or ta != tb:
                choice = (ta, tb, False)
                break
            left = self.leaves(na, ta)                # both name one slot: what A leaves there must be what B needs
            if (left is None) if nb[2] == "free" else (left is not None) if nb[2] == "any" else (left == nb[2]):
                choice = (ta, tb, True)
                break
        assert choice is not None, (A, B)
        ta, tb, shared = choice
        self.normalize()
        self.prepare_options(A)
        self.prepare_options(B)
        if nb is not None and not shared:
            self.ensure((nb[0], tb), nb[2])
        if na is not None:
            self.ensure((na[0], ta), na[2])
        for n_, t_ in ((na, ta), (nb, tb)):
            if n_ is not None and n_[0] == "s":
                self.ensure_room(t_)
        self.emit(self.build(A, va, ta, avoid=("generic", "skinny", "skinny_ln") if B == "linear_ln_act" else ()))
        self.emit(self.build(B, vb, tb))


def pair_walk(dims=None, dtype="f16"):
    """One walk in which, for every ordered pair (A, B) of KINDS, a call of kind B stands directly behind a call of kind A, on one handle
    that is never re-created: every pair also inherits all the history in front of it.  `dims` does not change it: the descriptors
    name forms and row counts, the handle's adapter sizes the tensors."""
    g = _Gen(dtype, 20251)
    pairs = list(enumerate(itertools.product(range(len(KINDS)), repeat=2)))
    for r, home in enumerate(regimes(dtype)):     # a third of the pairs under each regime, every kind as A and as B under all three
        g.home = home
        for idx, (a, b) in pairs:
            if (a + b) % 3 == r:
                g.pair(KINDS[a], KINDS[b], idx)
    return tuple(g.walk)


def random_walk(seed, n, dtype="f16"):
    """A seeded legal walk of n calls that holds every kind at least once"""
    g = _Gen(dtype, seed)
    r = random.Random(seed + 1)
    first = list(KINDS)
    r.shuffle(first)
    todo = first + [KINDS[r.randrange(len(KINDS))] for _ in range(n)]
    homes = regimes(dtype)
    for idx, kind in enumerate(todo):
        if len(g.walk) >= n:
            break
        g.home = homes[(seed + 3 * len(g.walk) // n) % 3]        # a third of the walk under each regime
        g.away += 1
        if g.away >= 3:                           # an excursion lasts two calls
            g.normalize()
        if kind == "set_option":
            g.away = 0
        variant = r.randrange(12)
        need = g.needs(kind, variant)
        slot = None
        g.prepare_options(kind)
        if need is not None:
            cands = list(need[1])
            r.shuffle(cands)
            fit = [c for c in cands if (need[2] == "free" and g.tag((need[0], c)) is None) or (need[2] == "any" and g.tag((need[0], c)) is not None) or
                   g.tag((need[0], c)) == need[2]]
            slot = fit[0] if fit else cands[0]
            g.ensure((need[0], slot), need[2])
            if need[0] == "s":
                g.ensure_room(slot)
        g.emit(g.build(kind, variant, slot))
    walk = tuple(g.walk[:n])
    assert len(walk) == n and set(kind_of(c) for c in walk) == set(KINDS), "random_walk: n is too small to hold every kind"
    return walk


def pairs_of(walk):
    return {(kind_of(a), kind_of(b)) for a, b in zip(walk, walk[1:])}


def check_legal(walk, dtype="f16"):
    """Runs the model over the walk; Illegal at the first call it would not have emitted.  -> the snapshots, one per call"""
    m = Model(dtype)
    snaps = []
    for i, call in enumerate(walk):
        try:
            m.check(call)
        except Illegal as e:
            raise Illegal(f"call {i} {call}: {e}") from None
        snaps.append(m.snapshot(call))
        m.apply(call)
        if len(m.states) > 3:
            raise Illegal(f"call {i} {call}: more than three states are open")
        for s in m.states.values():
            if len(s.hist) > MAX_REPLAY + 2:
                raise Illegal(f"call {i} {call}: a replay list of {len(s.hist)} calls")
    return snaps


# ---- the oracle ----------------------------------------------------------------------------------------------------------------------
def _state_options(h, have, want):
    for (name, v0), (name1, v1) in zip(have, want):
        assert name == name1
        if v0 != v1:
            h.call(("set_option", name, v1))


def expected(call, snap, make_handle, memo=None):
    """The oracle: `call` on a fresh handle made with exactly the options in force -- alone, behind the make of the mask it names, or,
    for a stream call, behind the state's own calls replayed each under the options recorded when it was made.  `memo`: a dict that
    keeps results by (call, snapshot); a memoised value still came from a fresh handle."""
    key = (call, snap)
    if memo is not None and key in memo:
        return memo[key]
    first = snap.replay[0][1] if snap.replay else snap.options
    h = make_handle(dict(first))
    try:
        have = first
        for past, options in (snap.replay or ()):
            _state_options(h, have, options)
            have = options
            h.call(past)
        _state_options(h, have, snap.options)
        if snap.mask is not None:
            h.call(snap.mask)
        out = h.call(call)
    finally:
        h.close()
    if memo is not None:
        memo[key] = out
    return out


# ---- the checker ---------------------------------------------------------------------------------------------------------------------
def _as_bytes(v):
    return np.ascontiguousarray(v).view(np.uint8)


def differences(got, want):
    """[] where the two results are the same; otherwise one line per named result that differs"""
    out = []
    if set(got) != set(want):
        return [f"the results named differ: {sorted(got)} against {sorted(want)}"]
    for name in sorted(want):
        a, b = got[name], want[name]
        if isinstance(b, np.ndarray) or isinstance(a, np.ndarray):
            if not (isinstance(a, np.ndarray) and isinstance(b, np.ndarray)) or a.shape != b.shape or a.dtype != b.dtype:
                out.append(f"{name}: {getattr(a, 'dtype', type(a))} {getattr(a, 'shape', '')} against {getattr(b, 'dtype', type(b))} {getattr(b, 'shape', '')}")
            elif not np.array_equal(_as_bytes(a), _as_bytes(b)):
                n = int((_as_bytes(a).reshape(a.size, -1) != _as_bytes(b).reshape(b.size, -1)).any(axis=1).sum()) if a.size else 0
                out.append(f"{name}: {n} of {a.size} elements differ in bits")
        elif a != b:
            out.append(f"{name}: {a!r} against the oracle's {b!r}")
    return out


class HistoryError(AssertionError):
    def __init__(self, index, call, previous, lines):
        self.index, self.call, self.previous, self.lines = index, call, previous, lines
        super().__init__(f"call {index} {call} behind {previous} differs from the same call on a fresh handle: " + "; ".join(lines))


def check_walk(make_handle, walk, dtype="f16", memo=None, walked=None):
    """Walks one handle made by make_handle(default options) through `walk` and compares every result-bearing call with `expected`.
    HistoryError at the first difference: its index, the call, the previous call, and how many elements or which record differ.  A result
    named "finite" must be True on every call but a poison; a host-positioned state's "positions" must also be the model's.
    `walked`: another factory for the handle that is walked (the oracle's handles stay make_handle's).
    -> {"calls", "checked", "kinds", "options"}"""
    m = Model(dtype)
    h = (walked or make_handle)(dict(m.options))
    stats = {"calls": 0, "checked": 0, "kinds": set(), "options": set()}
    try:
        for i, call in enumerate(walk):
            previous = walk[i - 1] if i else None
            m.check(call)
            snap = m.snapshot(call)
            got = h.call(call)
            stats["calls"] += 1
            stats["kinds"].add(kind_of(call))
            if call[0] == "set_option":
                stats["options"].add(call[1])
            m.apply(call)
            if call[0] in NO_RESULT:
                continue
            lines = differences(got, expected(call, snap, make_handle, memo))
            if call[0] != "poison" and got.get("finite", True) is not True:
                lines.append("a value that is not finite")
            sid = m.stream_of(call)
            if "positions" in got and sid in m.states and m.positions(sid) is not None and list(got["positions"]) != m.positions(sid):
                lines.append(f"positions {got['positions']} against the model's {m.positions(sid)}")
            if lines:
                raise HistoryError(i, call, previous, lines)
            stats["checked"] += 1
    finally:
        h.close()
    return stats
