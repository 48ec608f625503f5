"""A compiled mask on the 16-bit MFMA attention (option "mask_mfma", tf_attn_tiled_masked in flope_amd/csrc/tf_encoder.hip; DESIGN.md
38) on the test side: what tests/test_tf_mask16_host.py, tests/test_tf_mask16_bound.py (CPU) and tests/test_gpu_tf_mask16.py (device)
compare against.  tests/tf_attn_bound.py and tests/tf_attn_mask_bound.py are imported as they are; nothing here is fitted to an output.

  tile_map       the mask's tile map by brute force in numpy: per query block of 128 rows the ascending list of 64-key blocks that hold an
                 allowed pair, each with colany (64 bools) and the class of its 4 x 2 (wave, 32-key step) tiles (0 none, 1 some, 2 all,
                 rows and keys below L only)
  reference_of   fp64 masked attention from the 16-bit inputs as given, and tf_attn_bound's element-wise bound evaluated on the masked P
                 and A = P |v|, with a_i the largest |score| bound over the keys query i is allowed.  The operation counts of the bound
                 (n keys summed, ceil(n / 32) steps) stay those of the query's whole sequence of n tokens: a query sums at most n keys in
                 at most that many steps, so every term is an upper bound of the query's own.  The guard of the step (msafe: 0 subtracted
                 where the running maximum is still -inf) rounds nothing -- exp2(-inf) is exactly 0 -- so the bound has no term for it
  emulate        the walk of tf_attn_tiled_masked in torch float32: the entry list of the query block (under a length: its prefix), the
                 ring stage by trip index, rows staged as zeros where colany is clear or the row lies past the sequence, the class of a
                 wave's step, the word and bit of each lane, msafe -- and eight broken copies of it (MUTATIONS)
"""
import math

import numpy as np
import torch

import tf_attn_bound as AB
import tf_attn_mask_bound as MB

MUTATIONS = ["noword", "nextword", "bitmap", "some0", "some2", "noguard", "nocolany", "stagekb"]
NONE, SOME, ALL = 0, 1, 2
QB, KB = 128, 64

LENGTHS = (1, 33, 65, 129, 257)           # one key; one key into a second step; into a second block; a stage used twice; a third query block
HEAD_DIMS = (32, 64, 96, 128)
KINDS = ("random", "prefix", "band", "edge")      # tf_attn_mask_bound.make_allowed's: 40 % masked, prefix-LM, +-3 frames, the edge rows
DEAD_KEY = 40                             # `dead`: a key no query allows, inside a loaded block beside allowed keys


def gap_mask(L=257):
    """Query block 0 lists key blocks 0, 2 and 4: trip index and block index differ, and stage 0 is used by trips 0 and 2 across the gap.
    Rows 16 .. 31 see nothing in the first step their wave takes (keys 0 .. 31), key 32 is their first.  Query block 1 lists blocks 1 and
    3, row 256 sees keys 0 and 256."""
    assert L == 257
    g = torch.Generator().manual_seed(11)
    r = torch.rand(L, L, generator=g) < 0.4
    a = torch.zeros(L, L, dtype=torch.bool)
    for rows, blocks, sure in ((slice(0, 128), (0, 2, 4), 32), (slice(128, 256), (1, 3), 64)):
        for kblock in blocks:
            a[rows, kblock * KB:(kblock + 1) * KB] = r[rows, kblock * KB:(kblock + 1) * KB]
        a[rows, sure] = True
    a[16:32, 0:32] = False
    a[256, 0] = a[256, 256] = True
    return a


def dead_mask(L):
    """tf_attn_mask_bound's random mask with column DEAD_KEY cleared: no query allows that key (its own row sees key 0 instead)"""
    a = MB.make_allowed("random", L).clone()
    a[:, DEAD_KEY] = False
    a[DEAD_KEY, 0] = True
    return a


def poison(qkv, keys, value=float("nan")):
    """qkv [B, L, 3 d] with k and v of the given keys set to `value`"""
    d = qkv.shape[-1] // 3
    out = qkv.clone()
    out[:, keys, d:] = value
    return out


def tile_map(allowed):
    """allowed: bool [L, L] -> per query block the list of (kblock, colany [64] bool, cls [4][2] ints), ascending in kblock"""
    a = np.asarray(allowed, dtype=bool)
    L = a.shape[0]
    out = []
    for qb in range((L + QB - 1) // QB):
        lst = []
        for kblock in range((L + KB - 1) // KB):
            sub = a[qb * QB:(qb + 1) * QB, kblock * KB:(kblock + 1) * KB]
            if not sub.any():
                continue
            colany = np.zeros(KB, dtype=bool)
            colany[:sub.shape[1]] = sub.any(axis=0)
            cls = [[NONE, NONE] for _ in range(4)]
            for w in range(4):
                for s in range(2):
                    t = sub[32 * w:32 * w + 32, 32 * s:32 * s + 32]
                    if t.size:
                        cls[w][s] = ALL if t.all() else SOME if t.any() else NONE
            lst.append((kblock, colany, cls))
        out.append(lst)
    return out


def tile_stats(allowed):
    """what flope_tf_mask_tiles reports, from tile_map"""
    tm = tile_map(allowed)
    flat = [c for lst in tm for _, _, cls in lst for row in cls for c in row]
    return {"query_blocks": len(tm), "blocks_listed": sum(len(lst) for lst in tm), "steps_none": flat.count(NONE), "steps_some": flat.count(SOME),
            "steps_all": flat.count(ALL)}


def reference_of(qkv, allowed, H, dtype, lengths=None):
    """(O, bound) in fp64, both [B, L, d]: tf_attn_bound.reference_of's formula on the masked P, A and a_i of each sequence (lengths: under
    the mask's corner); rows behind a length are 0 with bound 0"""
    qkv = qkv.cpu().double()
    B, L, d3 = qkv.shape
    d = d3 // 3
    hd = d // H
    uT = AB.U_T[dtype]
    O = torch.zeros(B, L, d, dtype=torch.float64)
    Bd = torch.zeros(B, L, d, dtype=torch.float64)
    for b, n in enumerate(MB._lens(B, L, lengths)):
        ok = allowed[:n, :n]
        q, k, v = (qkv[b, :n, t * d:(t + 1) * d].reshape(n, H, hd).permute(1, 0, 2) for t in range(3))      # [H, n, hd]
        P = torch.softmax((q @ k.transpose(-1, -2) / math.sqrt(hd)).masked_fill(~ok[None], float("-inf")), dim=-1)
        o = P @ v
        A = P @ v.abs()
        a = (AB.LOG2E / math.sqrt(hd)) * (q.abs() @ k.abs().transpose(-1, -2)).masked_fill(~ok[None], 0.0).amax(dim=-1, keepdim=True)
        ns = (n + 31) // 32
        e = math.log(2.0) * (hd + 8) * AB.U32 * a + (4 * ns + 8) * AB.U32
        E = 2 * e + 2 * (n + ns + 10) * AB.U32
        bound = (uT + E) * A
        bound = bound + uT * (o.abs() + bound)
        if dtype == "f16":
            bound = bound + (n * 2.0 ** -25 * v.abs().amax(dim=(-1, -2), keepdim=True) + 2.0 ** -25)
        O[b, :n] = o.permute(1, 0, 2).reshape(n, d)
        Bd[b, :n] = bound.permute(1, 0, 2).reshape(n, d)
    return O, Bd


ratio = MB.ratio


def _words(allowed):
    """bool [L, L] -> the mask's words as python ints [L][ceil(L / 32)], padding bits zero"""
    a = np.asarray(allowed, dtype=bool)
    L = a.shape[0]
    nw = (L + 31) // 32
    pad = np.zeros((L, nw * 32), dtype=np.uint64)
    pad[:, :L] = a
    return (pad.reshape(L, nw, 32) << np.arange(32, dtype=np.uint64)).sum(axis=2)


def _lane_bits(word_col, mutation):
    """words [nq] -> seen [nq, 32] by KEY of the step: key kb + 16 u + 4 g + q tests bit 16 u + 4 g + q of the lane's word -- the key's own
    offset; `bitmap`: bit 8 g + 4 u + q, the lane's eight values taken as consecutive bits"""
    key = np.arange(32)
    bit = key
    if mutation == "bitmap":
        u, g, q = key // 16, (key % 16) // 4, key % 4
        bit = 8 * g + 4 * u + q
    return torch.from_numpy(((word_col[:, None] >> bit[None, :].astype(np.uint64)) & np.uint64(1)).astype(bool))


def emulate(qkv, allowed, H, dtype, lengths=None, mutation=None, rows="wave"):
    """tf_attn_bound.emulate's operations (running maximum, exp2, P rounded to T, float32 accumulators, one reciprocal, output rounding)
    per wave of 32 queries on the walk of tf_attn_tiled_masked -> [B, L, d] in T (rows behind a length: 0).  mutation: None, or one defect
         noword    the mask word ignored in a "some" step (the step's test of the bit left out)
         nextword  the word of step kb / 32 + 1 loaded
         bitmap    bit 8 g + 4 u + q instead of 16 u + 4 g + q
         some0     a "some" step skipped like a "none" step
         some2     a "some" step taken like an "all" step (the kernel's class branch; the walk of `noword`, reached another way)
         noguard   the running maximum itself subtracted, -inf included (exp2(-inf - -inf))
         nocolany  a row whose colany bit is clear staged as it is (shows with NaN in a key nobody allows)
         stagekb   the stage read taken from kblock & 1 while the writes go by trip index
    rows: how many query rows one float32 matrix product of the emulation holds -- "wave": the wave's own (as the per-wave emulations
    of tf_attn_window16_bound and tf_attn_causal_bound), "sequence": all rows of the sequence, the wave's taken out of the result (as
    tf_attn_bound.emulate).  A row of a product depends on no other row; the count only decides which routine the CPU library runs (a
    one-row product takes another one), so it matters for comparisons in bits with those emulations and for nothing else."""
    dt = AB.TDT[dtype]
    qkv = qkv.cpu()
    B, L, d3 = qkv.shape
    d = d3 // 3
    hd = d // H
    tm = tile_map(allowed)
    words = _words(allowed)
    nw = words.shape[1]
    scale = torch.tensor(AB.LOG2E, dtype=torch.float32) / torch.sqrt(torch.tensor(float(hd)))
    ninf = torch.tensor(float("-inf"))
    out = torch.zeros(B, L, d, dtype=dt)
    for b, n in enumerate(MB._lens(B, L, lengths)):
        x = qkv[b, :n].float()
        q, k, v = (x[:, t * d:(t + 1) * d].reshape(n, H, hd).permute(1, 0, 2).contiguous()[None] for t in range(3))      # [1, H, n, hd]
        res = torch.empty(1, H, n, hd)
        for qb in range((n + QB - 1) // QB):
            entries = [e for e in tm[qb] if e[0] * KB < n]                   # the corner's prefix
            stages = [None, None]
            state = {}
            for w in range(4):
                q0 = qb * QB + 32 * w
                if q0 < n:
                    nq = min(32, n - q0)
                    state[w] = [torch.full((1, H, nq), float("-inf")), torch.zeros(1, H, nq), torch.zeros(1, H, nq, hd)]
            for trip, (kblock, colany, cls) in enumerate(entries):
                krows = torch.arange(kblock * KB, kblock * KB + KB)
                keep = krows < n
                if mutation != "nocolany":
                    keep = keep & torch.from_numpy(colany)
                src = krows.clamp(max=n - 1)
                z = torch.zeros(())
                stages[trip & 1] = (torch.where(keep[:, None], k[:, :, src], z), torch.where(keep[:, None], v[:, :, src], z))
                st = stages[kblock & 1] if mutation == "stagekb" else stages[trip & 1]
                if st is None:
                    st = (torch.zeros(1, H, KB, hd), torch.zeros(1, H, KB, hd))
                for w, (m, l, o) in state.items():
                    q0 = qb * QB + 32 * w
                    nq = m.shape[-1]
                    for s in range(2):
                        kb = kblock * KB + 32 * s
                        c = cls[w][s]
                        if kb >= n or c == NONE or (c == SOME and mutation == "some0"):
                            continue
                        keys = torch.arange(kb, kb + 32)
                        seen = (keys < n)[None, :].expand(nq, 32)
                        if c == SOME and mutation not in ("noword", "some2"):
                            wi = kb // 32 + (1 if mutation == "nextword" else 0)
                            col = words[q0:q0 + nq, wi] if wi < nw else np.zeros(nq, dtype=np.uint64)
                            seen = seen & _lane_bits(col, mutation)
                        kt = st[0][:, :, 32 * s:32 * s + 32].transpose(-1, -2)
                        sc = ((q @ kt)[:, :, q0:q0 + nq] if rows == "sequence" else q[:, :, q0:q0 + nq] @ kt) * scale
                        sc = torch.where(seen, sc, ninf)
                        mnew = torch.maximum(m, sc.amax(dim=-1))
                        msafe = mnew if mutation == "noguard" else torch.where(mnew == ninf, torch.zeros(()), mnew)
                        alpha = torch.exp2(m - msafe)
                        p = torch.exp2(sc - msafe[..., None])
                        l = l * alpha + p.sum(dim=-1)
                        pt = p.to(dt).float()
                        if rows == "sequence":
                            pf = torch.zeros(1, H, n, 32)
                            pf[:, :, q0:q0 + nq] = pt
                            o = o * alpha[..., None] + (pf @ st[1][:, :, 32 * s:32 * s + 32])[:, :, q0:q0 + nq]
                        else:
                            o = o * alpha[..., None] + pt @ st[1][:, :, 32 * s:32 * s + 32]
                        m = mnew
                    state[w] = [m, l, o]
            for w, (m, l, o) in state.items():
                q0 = qb * QB + 32 * w
                res[:, :, q0:q0 + m.shape[-1]] = o * (1.0 / l)[..., None]
        out[b, :n] = AB.merge_heads(res.to(dt))[0]
    return out
