"""The encoder handle after any history, on the device: the result of a call -- the returned tensor in bits and what the
call records -- is the result of the same call on a fresh handle made with the options in force, for a stream call behind that state's
own calls alone.  tests/tf_history_cases.py holds the descriptors, the model, the two generators, the oracle and the checker; this file
wraps flope_amd.TransformerEncoder in the small handle interface they are written against and walks it.

Handles (max_tokens = 256): TOY (16, 32, 9, 4, 2, 64) in f32 and f32m -- the generic and rowwave linears, the generic attention, `fused`
-- and WIDE (16, 128, 9, 2, 2, 256) in f16 and bf16 -- the MFMA linear and attention, skinny, skinny_ln, step_split, extend_mfma and
mask_mfma / bias_mfma / window_mfma at head_dim 64 --, each in the default architecture and in norm_first + gelu + final_norm.

  1. test_pair_walk: every ordered pair of the 23 kinds on one long-lived handle, every result-bearing call checked
  2. test_random_walks: three seeded walks of 150 calls on WIDE f16 and TOY f32m
  3. test_walk_on_a_side_stream: one of those walks wholly on another stream, each input written there behind a large matmul into a
     buffer whose NaN pre-fill is complete; the oracle values are the default stream's
  4. every call but a poison returns finite values (checked by check_walk on every call, so also behind every poison)
  5. every pair walk reached the kernels its handle exists for (REACHED, by the ids its calls returned), every random walk the dtype's own
     linear and attention kernels; a 16-bit walk's linear_ln_act calls all launched (a refusal is the result only where linear_ln_plan
     says there is no such launch)
  6. the last test: every kind and every option name was exercised in every dtype

What a call records and this file compares: forward -- last_forward_fused, last_ln, and under a compiled mask last_attn_kernel;
attention -- last_attn_kernel; linear / linear_ln_act -- last_linear_kernel; layernorm -- last_ln_kernel; a stream call -- the state's
positions, step_plan, extend_plan() and the encoder's last_ln; step_assoc also last_feed() and last_tokens(); make_mask / make_bias -- L,
allowed, planes, tile_stats; set_option -- the value it returns (the previous one).
One exclusion: last_ln is documented as the counts "of the last forward / stream call that ran kernel by kernel", so behind a forward
that ran as the single launch (last_forward_fused) it still holds an earlier call's counts and is not compared there.
There is no tolerance in this file: every comparison is equality of bits or of integers.
"""
import functools

import numpy as np
import pytest
import torch

import tf_arch_cases as AC
import tf_attn_bias_bound as BB
import tf_attn_mask_bound as MB
import tf_history_cases as H

pytestmark = pytest.mark.gpu

TOY = (16, 32, 9, 4, 2, 64)
WIDE = (16, 128, 9, 2, 2, 256)
OTHER = (8, 64, 5, 2, 1, 128)                   # the second encoder of kind other_handle
ARCHS = {"post": AC.DEFAULT, "pre": {"norm_first": True, "activation": "gelu", "final_norm": True}}
TDT = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32, "f32m": torch.float32}
PAIR_PARAMS = [(TOY, "f32"), (TOY, "f32m"), (WIDE, "f16"), (WIDE, "bf16")]
RANDOM_ON = [(WIDE, "f16"), (TOY, "f32m")]
GENERIC, MFMA64, TILED, ATTN_F32M, MASKED, MASKED16, BIASED, BIASED16 = range(8)       # FLOPE_TF_ATTN_*
LIN_GENERIC, LIN_MFMA, LIN_F32M, SKINNY, SKINNY_LN = 0, 3, 4, 5, 6                       # FLOPE_TF_LIN_*
# what a walk must have reached on the device, by dtype: the kernels the handle exists for, under the options that pick them
REACHED = {
    "16": {("linear_kernel", LIN_MFMA), ("linear_kernel", SKINNY), ("linear_ln_act", SKINNY_LN), ("attn_kernel", MFMA64), ("attn_kernel", TILED),
           ("attn_kernel", MASKED), ("attn_kernel", MASKED16), ("attn_kernel", BIASED), ("attn_kernel", BIASED16), ("forward_attn_kernel", MASKED16),
           ("forward_attn_kernel", BIASED16), ("extend_plan", "mfma"), ("extend_plan", "row"), ("fused", False)},
    "32": {("linear_kernel", LIN_GENERIC), ("linear_kernel", LIN_F32M), ("attn_kernel", GENERIC), ("attn_kernel", ATTN_F32M), ("attn_kernel", MASKED),
           ("attn_kernel", BIASED), ("forward_attn_kernel", MASKED), ("forward_attn_kernel", BIASED), ("fused", True), ("fused", False),
           ("extend_plan", "split"), ("extend_plan", "row")},
    "all": {("step_plan", "split"), ("step_plan", "biased"), ("step_plan", "row"), ("extend_plan", "biased")},
}
SEEDS, N_RANDOM = H.RANDOM_SEEDS, H.RANDOM_CALLS
assert tuple(t for _, t in RANDOM_ON) == H.RANDOM_DTYPES

_MEMO = {}                                      # (dims, dtype, arch) -> check_walk's memo of oracle results
_SEEN = {}                                      # dtype -> {"kinds", "options", "facts"}: what the walks of this session exercised
_TOTAL = {"calls": 0, "checked": 0}


@functools.lru_cache(maxsize=None)
def _state_dict(dims, final_norm):
    return AC.state_dict(dims, final_norm)


def _host(t):
    """(the tensor's bits as a numpy array, whether every value is finite)"""
    c = t.detach().cpu().contiguous()
    return c.view(torch.int16 if c.element_size() == 2 else torch.int32).numpy(), bool(torch.isfinite(c).all())


class Handle:
    """tests/tf_history_cases.py's handle interface over one TransformerEncoder: call(descriptor) -> the named results"""

    def __init__(self, dims, dtype, arch, options, side=None):
        from flope_amd.tf_encoder import TransformerEncoder
        self.dims, self.dtype, self.arch, self.side = dims, dtype, ARCHS[arch], side
        self.enc = TransformerEncoder(*dims, dtype=dtype, max_tokens=H.MAX_TOKENS, **self.arch)
        self.enc.load_state_dict(_state_dict(dims, self.arch["final_norm"]))
        for name, value in options.items():
            if value != H.default_options(dtype)[name]:
                self.enc.set_option(name, value)
        self.states, self.masks, self.other = {}, {}, None
        self.facts = set()
        if side is not None:
            with torch.cuda.stream(side):
                self.big = torch.randn(2048, 2048, device="cuda")

    # an input goes to the device here.  On a side stream: into a buffer whose pre-fill (NaN; SKIP for an association) is complete, by a
    # copy queued on that stream behind a large matmul, so that a launch or copy of the call on any other stream meets the pre-fill
    def up(self, t):
        if self.side is None:
            return t.cuda()
        buf = torch.empty(t.shape, dtype=t.dtype, device="cuda")
        buf.fill_(float("nan") if t.dtype.is_floating_point else H.SKIP)
        self.side.synchronize()
        self.big @ self.big
        buf.copy_(t.pin_memory(), non_blocking=True)
        return buf

    def call(self, c):
        if self.side is None:
            return self._call(c)
        with torch.cuda.stream(self.side):
            return self._call(c)

    def close(self):
        for s in self.states.values():
            s.close()
        for m in self.masks.values():
            m.close()
        if self.other is not None:
            self.other.close()
        self.enc.close()

    # ---- the kinds -------------------------------------------------------------------------------------------------------------------
    def _modes(self, mode, mid):
        if mode == "causal":
            return {"is_causal": True}
        if mode == "window":
            return {"is_causal": True, "window": H.WINDOW}
        if mode in ("mask", "bias"):
            return {"mask": self.masks[mid]}
        return {}

    def _stream_result(self, s, y=None):
        out = {"positions": list(s.positions), "step_plan": s.step_plan, "extend_plan": s.extend_plan()}
        self.facts |= {("step_plan", out["step_plan"]), ("extend_plan", out["extend_plan"])}
        if y is not None:
            out["y"], out["finite"] = _host(y)
            out["last_ln"] = self.enc.last_ln
        return out

    def _call(self, c):
        enc, k = self.enc, c[0]
        i, d, o, heads, nl, ff = self.dims
        tdt = TDT[self.dtype]
        if k in H.FORWARDS:
            mode = k[len("forward_"):]
            B, L, seed, mid = c[1:]
            kw = self._modes(mode, mid)
            if H.is_ragged(c):
                kw["lengths"] = list(H.lengths_of(B, L, seed))
            y = enc.forward(self.up(H.randn((B, L, i), "forward", B, L, seed)), **kw)
            out = {"fused": bool(enc.last_forward_fused)}
            out["y"], out["finite"] = _host(y)
            if not out["fused"]:
                out["last_ln"] = enc.last_ln      # (the exclusion of the header)
            if mode in ("mask", "bias"):
                out["attn_kernel"] = enc.last_attn_kernel
                self.facts.add(("forward_attn_kernel", out["attn_kernel"]))
            self.facts.add(("fused", out["fused"]))
            return out
        if k == "attention":
            mode, B, L, seed, mid = c[1:]
            kw = self._modes(mode, mid)
            qkv = H.randn((B, L, 3 * d), "attention", B, L, seed).to(tdt)
            if H.is_ragged(c):
                kw["lengths"] = list(H.lengths_of(B, L, seed))
                qkv = torch.cat([qkv[b, :n] for b, n in enumerate(kw["lengths"])]).contiguous()
            y = enc.attention(self.up(qkv), **kw)
            out = {"attn_kernel": enc.last_attn_kernel}
            out["y"], out["finite"] = _host(y)
            self.facts.add(("attn_kernel", out["attn_kernel"]))
            return out
        if k == "linear":
            form, rows, seed = c[1:]
            name = {"embedding": "embedding", "in_proj": "layers.0.in_proj", "out_proj": "layers.0.out_proj", "linear1": "layers.1.linear1",
                    "linear2": "layers.1.linear2"}[form]
            N, K = enc._linear_dims(name)
            x = H.randn((rows, K), "linear", form, rows, seed)
            x = self.up(x if form == "embedding" else x.to(tdt))
            res = self.up(H.randn((rows, N), "linear-res", form, rows, seed).to(tdt)) if form in ("out_proj", "linear2") else None
            y = enc.linear(name, x, res=res, act=self.arch["activation"] if form == "linear1" else None)
            out = {"linear_kernel": enc.last_linear_kernel}
            out["y"], out["finite"] = _host(y)
            self.facts.add(("linear_kernel", out["linear_kernel"]))
            return out
        if k in ("layernorm", "linear_ln_act"):
            rows, seed = c[-2:]
            x = self.up(H.randn((rows, d), "ln", rows, seed).to(tdt))
            w = self.up(1.0 + 0.5 * H.randn((d,), "ln-w", seed))
            b = self.up(0.5 * H.randn((d,), "ln-b", seed))
            if k == "layernorm":
                y = enc.layernorm(x, w, b)
                out = {"ln_kernel": enc.last_ln_kernel}
                out["y"], out["finite"] = _host(y)
                return out
            name, act = H.LN_ACT_FORMS[c[1]]
            plan = enc.linear_ln_plan(name, rows)
            self.facts.add(("linear_ln_plan", plan))
            if plan != SKINNY_LN:                 # the plan says this handle has no such launch: the refusal is the result, and only then
                with pytest.raises(ValueError):
                    enc.linear_ln_act(name, x, w, b, act)
                return {"refused": "ValueError", "plan": plan}
            y, normed = enc.linear_ln_act(name, x, w, b, act)
            out = {"linear_kernel": enc.last_linear_kernel, "plan": plan}
            out["y"], f0 = _host(y)
            out["normed"], f1 = _host(normed)
            out["finite"] = f0 and f1
            self.facts.add(("linear_ln_act", out["linear_kernel"]))
            return out
        if k == "open_stream":
            from flope_amd.tf_encoder import alibi_distances
            sid, form = c[1:]
            tracks, cap, window, device = H.STREAM_FORMS[form]
            kw = {"positions": "device", "max_rows": H.MAX_ROWS} if device else {}
            if form == "alibi":
                kw["bias"] = alibi_distances(window, [2.0 ** -(h + 1) for h in range(heads)])
            self.states[sid] = enc.open_stream(tracks, cap, window=window, **kw)
            return self._stream_result(self.states[sid])
        if k == "step":
            s, tracks, seed = self.states[c[1]], c[2], c[3]
            n = s.tracks if tracks is None else len(tracks)
            y = s.step(self.up(H.randn((n, i), "step", n, seed)), tracks=None if tracks is None else list(tracks))
            return self._stream_result(s, y)
        if k in ("extend", "prefill"):
            s, tracks, lengths, seed = self.states[c[1]], c[2], c[3], c[4]
            x = self.up(H.randn((len(lengths), max(lengths), i), k, lengths, seed))
            y = getattr(s, k)(x, lengths=list(lengths), tracks=None if tracks is None else list(tracks))
            return self._stream_result(s, y)
        if k == "reset":
            s = self.states[c[1]]
            s.reset(None if c[2] is None else list(c[2]))
            return {"positions": list(s.positions)}
        if k == "step_assoc":
            s, assoc, seed = self.states[c[1]], c[2], c[3]
            x = self.up(H.randn((len(assoc), i), "step_assoc", len(assoc), seed))
            y = s.step_assoc(x, self.up(torch.tensor(assoc, dtype=torch.int32)))
            out = self._stream_result(s, y)
            out["feed_tracks"], out["feed_positions"] = s.last_feed()
            out["tokens"] = s.last_tokens().view(np.int32)
            return out
        if k == "close":
            self.states.pop(c[1]).close()
            return {}
        if k in ("make_mask", "make_bias"):
            mid, kind, L = c[1:]
            if k == "make_mask":
                m = enc.make_mask(MB.to_torch_mask(MB.make_allowed(kind, L)))
            else:
                m = enc.make_bias(BB.make_bias(kind, L, heads))
            self.masks[mid] = m
            return {"L": m.L, "allowed": m.allowed, "planes": m.planes, "tile_stats": tuple(sorted(m.tile_stats.items()))}
        if k == "close_mask":
            self.masks.pop(c[1]).close()
            return {}
        if k == "set_option":
            return {"old": enc.set_option(c[1], c[2])}
        if k == "poison":
            nan = float("nan")
            if c[1] == "forward":                 # every workspace row holds NaN afterwards; all of it inside the handle's own allocations
                y = enc.forward(self.up(torch.full((1, H.MAX_TOKENS, i), nan)))
                return {"nan": bool(torch.isnan(y).all().item())}
            s = self.states[c[2]]
            L = min(s.capacity, 4)
            y = s.prefill(self.up(torch.full((s.tracks, L, i), nan)))
            isnan = bool(torch.isnan(y).all().item())
            s.reset()
            return {"nan": isnan, "positions": list(s.positions)}
        assert k == "other_handle", c
        if self.other is None:
            from flope_amd.tf_encoder import TransformerEncoder
            self.other = TransformerEncoder(*OTHER, dtype=self.dtype, max_tokens=64)
            self.other.load_state_dict(_state_dict(OTHER, False))
        out = {}
        out["y"], out["finite"] = _host(self.other.forward(self.up(H.randn((2, 9, OTHER[0]), "other", c[1]))))
        return out


def _walk(dims, dtype, arch, walk, side=False):
    """check_walk over `walk` on one handle; the module's records take what it exercised"""
    facts = set()

    def make(options, side_stream=None):
        h = Handle(dims, dtype, arch, options, side_stream)
        h.facts = facts
        return h
    walked = None
    if side:
        stream = torch.cuda.Stream()

        def walked(options):
            return make(options, stream)
    stats = H.check_walk(make, walk, dtype, _MEMO.setdefault((dims, dtype, arch), {}), walked=walked)
    torch.cuda.synchronize()
    seen = _SEEN.setdefault(dtype, {"kinds": set(), "options": set(), "facts": set()})
    seen["kinds"] |= stats["kinds"]
    seen["options"] |= stats["options"]
    seen["facts"] |= facts
    _TOTAL["calls"] += stats["calls"]
    _TOTAL["checked"] += stats["checked"]
    print(f"{dims} {dtype} {arch}{' side stream' if side else ''}: {stats['calls']} calls, {stats['checked']} checked against a fresh handle")
    stats["facts"] = facts
    return stats


def _reached(dtype, facts, pre=False):
    """the kernels a whole walk on this dtype must have reached (the single launch is the default architecture's alone)"""
    want = REACHED["16" if dtype in ("f16", "bf16") else "32"] | REACHED["all"]
    if pre:
        want = want - {("fused", True)}
    assert want <= facts, (dtype, sorted(want - facts, key=repr))


@pytest.mark.parametrize("arch", list(ARCHS))
@pytest.mark.parametrize("dims,dtype", PAIR_PARAMS, ids=[("toy-" if d == TOY else "wide-") + t for d, t in PAIR_PARAMS])
def test_pair_walk(dims, dtype, arch):
    """every ordered pair of kinds on one long-lived handle; every result-bearing call is checked, none skipped"""
    walk = H.pair_walk(dims, dtype)
    stats = _walk(dims, dtype, arch, walk)
    assert stats["calls"] == len(walk)
    assert stats["checked"] == sum(1 for c in walk if c[0] not in H.NO_RESULT)
    assert stats["kinds"] == set(H.KINDS) and stats["options"] == set(H.OPTION_NAMES)
    _reached(dtype, stats["facts"], pre=arch == "pre")
    if dtype in ("f16", "bf16"):                  # every linear_ln_act of a 16-bit walk launched: none was the refusal
        assert {f for f in stats["facts"] if f[0] == "linear_ln_plan"} == {("linear_ln_plan", SKINNY_LN)}


def _hot(dtype, facts):
    """a walk of 150 calls holds few calls of each kind, so it is held to the dtype's own linear and attention kernels only"""
    if dtype in ("f16", "bf16"):
        assert facts & {("linear_kernel", LIN_MFMA), ("linear_kernel", SKINNY)} and facts & {("attn_kernel", MFMA64), ("attn_kernel", TILED)}, sorted(facts, key=repr)
        assert ("linear_ln_plan", SKINNY_LN) in facts and not {f for f in facts if f[0] == "linear_ln_plan" and f[1] != SKINNY_LN}
    else:
        assert ("linear_kernel", LIN_F32M) in facts or ("attn_kernel", ATTN_F32M) in facts, sorted(facts, key=repr)


@pytest.mark.parametrize("seed", SEEDS)
def test_random_walks(seed):
    for dims, dtype in RANDOM_ON:
        walk = H.random_walk(seed, N_RANDOM, dtype)
        stats = _walk(dims, dtype, "post", walk)
        assert stats["checked"] == sum(1 for c in walk if c[0] not in H.NO_RESULT)
        _hot(dtype, stats["facts"])


def test_walk_on_a_side_stream():
    """a launch or a copy on another stream than the caller's reads an input that is still its pre-fill, or returns before its result"""
    dims, dtype = RANDOM_ON[0]
    walk = H.random_walk(SEEDS[0], N_RANDOM, dtype)
    stats = _walk(dims, dtype, "post", walk, side=True)
    assert stats["checked"] == sum(1 for c in walk if c[0] not in H.NO_RESULT)
    _hot(dtype, stats["facts"])


def test_every_kind_and_option_was_exercised_in_every_dtype():
    """Runs last; a dtype whose pair walk did not run in this session (a -k selection) is walked here, so the assertion stands alone."""
    for dims, dtype in PAIR_PARAMS:
        if dtype not in _SEEN or _SEEN[dtype]["kinds"] != set(H.KINDS):
            _walk(dims, dtype, "post", H.pair_walk(dims, dtype))
    for dims, dtype in PAIR_PARAMS:
        seen = _SEEN[dtype]
        assert seen["kinds"] == set(H.KINDS), (dtype, set(H.KINDS) - seen["kinds"])
        assert seen["options"] == set(H.OPTION_NAMES), (dtype, set(H.OPTION_NAMES) - seen["options"])      # causal, window: kinds forward_causal / forward_window
        print(dtype, sorted(seen["facts"], key=repr))
        _reached(dtype, seen["facts"])
    print(f"{_TOTAL['calls']} calls walked, {_TOTAL['checked']} checked against a fresh handle")
