"""The float32 MFMA attention of the encoder (tf_attn_f32m<NT, VARLEN, CAUSAL>, dtype="f32m", kernel id 3) on the device,
alone: every output element of enc.attention against fp64 within the derived bound of tests/tf_attn_f32m_bound.py (assertion 1)
and the relative L2 error within the bound's statistical form (assertion 2), on the smallest shapes at which each piece of the
kernel can go wrong --

  1. fixed length and is_causal over the shape table (every NT, part-used head-dim tiles next to the tile-edge lengths, a tile pair,
     a second score trip, a second value trip), three data kinds on the small shapes;
  2. ragged batches, lengths [1, 17, 64, 5, 33] and the reverse, plain and causal, every NT; each sequence = the sequence alone, in bits;
  3. the largest L the host rule still sends to this kernel (asked of the harness, per NT), and one key more: the generic kernel,
     judged by the row bound of tests/tf_attn_mask_bound.py.

The rows behind the input are NaN and those behind the output a sentinel, so a read past the batch shows up as NaN and a write past
it in the sentinel, without any fault being provoked; two runs give equal bits.  The last test asserts that every (NT, instantiation)
pair was judged.  Every test prints its figures (-s).
"""
import ctypes as C
import os
import subprocess

import pytest
import torch

import tf_attn_f32m_bound as FB
import tf_attn_mask_bound as MB

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GENERIC, F32M = 0, 3
SENTINEL = 1234.0
H = 2                                  # of the ragged and the limit shapes


def _plan():
    path = os.path.join(ROOT, "tests", "host_harness", "libflope_host_tf_attn.so")
    if not os.path.exists(path):
        subprocess.check_call(["make", "-C", ROOT, "tests/host_harness/libflope_host_tf_attn.so"])
    return C.CDLL(path)


PLAN = _plan()
JUDGED = {}                            # (NT, instantiation) -> (worst err / bound, worst relL2 / yardstick)


def _note(hd, inst, r1, r2):
    key = (FB.nt_of(hd), inst)
    old = JUDGED.get(key, (0.0, 0.0))
    JUDGED[key] = (max(old[0], r1), max(old[1], r2))


def _handle(heads, hd, max_tokens):
    """A handle for attention() alone: no layers, no weights."""
    from flope_amd.tf_encoder import TransformerEncoder
    return TransformerEncoder(16, heads * hd, 9, heads, 0, 64, dtype="f32m", max_tokens=max_tokens)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _run_guarded(enc, flat, want, **kw):
    """flat [rows, 3 d] at the head of a tensor whose tail rows are NaN, the output at the head of one whose tail is the sentinel;
    two runs.  -> the output [rows, d] (a copy)"""
    rows, d3 = flat.shape
    d = d3 // 3
    big = torch.full((rows + 64, d3), float("nan"), device="cuda")
    big[:rows] = flat.cuda()
    obig = torch.full((rows + 64, d), SENTINEL, device="cuda")
    shape = kw.pop("shape", None)
    view = (lambda t, w: t[:rows]) if shape is None else (lambda t, w: t[:rows].view(shape[0], shape[1], w))
    enc.attention(view(big, d3), out=view(obig, d), **kw)
    assert enc.last_attn_kernel == want
    torch.cuda.synchronize()
    first = obig.clone()
    assert torch.isfinite(first[:rows]).all(), "a non-finite output: rows past the batch were read, or a padded key was not masked"
    assert (first[rows:] == SENTINEL).all(), "a store past the last token"
    obig[:rows] = SENTINEL
    enc.attention(view(big, d3), out=view(obig, d), **kw)
    torch.cuda.synchronize()
    assert torch.equal(_bits(obig), _bits(first)), "two runs differ"
    assert torch.isnan(big[rows:]).all()
    return first[:rows].clone()


def _assert_both(got, j, what, hd, inst):
    r1, where, r2 = FB.verdict(got, j)
    print(f"{what}: max err / bound {r1:.4f} at {where}, relL2 / yardstick {r2:.4f}")
    _note(hd, inst, r1, r2)
    assert r1 <= 1.0, (what, where)                        # assertion 1
    assert r2 <= 1.0, what                                 # assertion 2


@pytest.mark.parametrize("causal", [False, True], ids=["fixed", "causal"])
@pytest.mark.parametrize("case", FB.CASES, ids=FB.case_id)
def test_every_element_within_the_bound_of_fp64(case, causal):
    B, L, heads, hd, kind = case
    qkv = FB.make_qkv(kind, B, L, heads, hd)
    enc = _handle(heads, hd, B * L)
    got = _run_guarded(enc, qkv.reshape(B * L, -1), F32M, shape=(B, L), is_causal=causal)
    _assert_both(got.view(B, L, -1), FB.reference(case, causal), f"{FB.case_id(case)} causal={int(causal)}", hd, "causal" if causal else "fixed")
    enc.close()


@pytest.mark.parametrize("causal", [False, True], ids=["ragged", "ragged-causal"])
@pytest.mark.parametrize("reverse", [False, True], ids=["fwd", "rev"])
@pytest.mark.parametrize("hd,kind", FB.RAGGED_CASES)
def test_ragged_batches(hd, kind, reverse, causal):
    lengths = FB.RAGGED[::-1] if reverse else FB.RAGGED
    seqs = FB.make_ragged(kind, lengths, H, hd)
    T, d = sum(lengths), H * hd
    enc = _handle(H, hd, T)
    got = _run_guarded(enc, torch.cat(seqs), F32M, lengths=list(lengths), is_causal=causal)
    _assert_both(got, FB.reference_ragged(kind, lengths, H, hd, causal), f"hd={hd} {kind} lengths={lengths} causal={int(causal)}", hd,
                 "ragged-causal" if causal else "ragged")
    row0 = 0
    for n, seq in zip(lengths, seqs):
        alone = enc.attention(seq.cuda().view(1, n, 3 * d), is_causal=causal)
        assert enc.last_attn_kernel == F32M
        diff = int((_bits(alone[0]) != _bits(got[row0:row0 + n])).sum())
        assert diff == 0, f"the sequence of length {n} at row {row0} differs in {diff} elements from itself alone"
        row0 += n
    enc.close()


# head_dim (NT 1, 4, 8), causal
@pytest.mark.parametrize("hd,causal", [(4, False), (4, True), (36, False), (128, False)])
def test_the_longest_sequence_the_kernel_takes(hd, causal):
    L = FB.lds_limit(PLAN, hd)
    case = FB.Case(1, L, H, hd, "normal")
    qkv = FB.make_qkv("normal", 1, L, H, hd)
    enc = _handle(H, hd, L)
    got = _run_guarded(enc, qkv[0], F32M, shape=(1, L), is_causal=causal)
    _assert_both(got.view(1, L, -1), FB.reference(case, causal), f"{FB.case_id(case)} causal={int(causal)} (the LDS limit)", hd,
                 "causal" if causal else "fixed")
    enc.close()


@pytest.mark.parametrize("hd", [4, 128])
def test_one_key_more_is_handed_to_the_generic_kernel(hd):
    L = FB.lds_limit(PLAN, hd) + 1
    assert PLAN.tf_attn_pick(2, hd, L, 0, 1, 0, 1) == GENERIC
    qkv = FB.make_qkv("normal", 1, L, H, hd)
    enc = _handle(H, hd, L)
    for kind in ("clear", "causal"):
        got = _run_guarded(enc, qkv[0], GENERIC, shape=(1, L), is_causal=kind == "causal")
        ref, bound = MB.reference_of(qkv, MB.make_allowed(kind, L), H, "f32")
        r, where = MB.ratio(got.view(1, L, -1), ref, bound)
        print(f"hd={hd} L={L} {kind} on the generic kernel: max err / row bound {r:.4f} at {where}")
        assert r <= 1.0, (kind, where)
    enc.close()


def test_every_instantiation_was_judged():
    """runs last in this module: NT 1 / 2 / 4 / 8 x fixed / causal / ragged / ragged-causal"""
    for key in sorted(JUDGED):
        print(f"NT {key[0]} {key[1]}: worst max err / bound {JUDGED[key][0]:.4f}, worst relL2 / yardstick {JUDGED[key][1]:.4f}")
    missing = [(nt, inst) for nt in (1, 2, 4, 8) for inst in ("fixed", "causal", "ragged", "ragged-causal") if (nt, inst) not in JUDGED]
    assert not missing, missing
