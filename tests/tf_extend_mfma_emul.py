"""Option "extend_mfma"  on the test side: the shapes tests/test_tf_extend_mfma_host.py (CPU) and
tests/test_gpu_tf_extend_mfma.py (device) share, and the walk of tf_attn16_extend emulated in torch float32 with the operations of
tf_attn_causal_bound.emulate / tf_attn_window16_bound.emulate.  The bound modules are imported as they are; no shape, bound or tolerance
here is fitted to an output.  One helper is there for the CPU's sake alone: _mm_rows computes each query's matrix products inside a
product of the aligned emulations' shape, because a CPU matrix product may sum in another order for another row count.  The bit
comparison with the aligned emulations therefore proves the WALK (steps, masks, key sources), not that a row's arithmetic is
independent of its neighbours; that rests on the device tests (tests/test_gpu_tf_extend_mfma.py, part b).

  LINEAR, RAGGED, WINDOWED   the shapes of the element-wise device test, as (cached, chunk, H, head_dim) and (W, capacity, cached, chunk,
                             H, head_dim)
  track_qkv                  the q | k | v rows of one whole track, cached + chunk tokens
  pre_call_cache             what the track's cache holds in front of the call: row j (a ring: j % capacity) holds key j for the keys
                             below `cached` that are still there, every other row a `stale` filler (finite garbage, or NaN)
  emulate                    the kernel's walk: query blocks of 128 chunk rows, waves at q0 = cached + 128 y + 32 w, ABSOLUTE 64-key
                             blocks and 32-key steps, a key row taken by the key-source rule (zeros / cache row / chunk row), the mask
                             on absolute positions -- and six broken copies of it (MUTATIONS)
"""
import torch

import tf_attn_bound as AB

# (cached, chunk, H, head_dim): smallest; two query tiles and a step inside the chunk; the cache / chunk split inside a step and the chunk
# across a step boundary; across a 64-key block and both ring stages; two query blocks (grid y = 2); a long cache
LINEAR = [(0, 1, 2, 32), (0, 33, 1, 64), (31, 2, 2, 64), (63, 66, 2, 64), (100, 130, 1, 96), (500, 12, 2, 64)]
# one call of three sequences: cached, chunk per sequence; H, head_dim
RAGGED = ((0, 65, 200), (7, 1, 40), 2, 128)
# (W, capacity, cached, chunk, H, head_dim): a wrapped ring at capacity == W (the append hazard's case); a wrapped ring; a chunk longer
# than the ring; one key; a window of a step and a key
WINDOWED = [(70, 70, 150, 45, 2, 64), (70, 96, 150, 45, 2, 64), (70, 70, 150, 100, 2, 64), (1, 16, 20, 20, 2, 32), (33, 64, 30, 70, 1, 128)]

MUTATIONS = ["alignedlast", "relmask", "nowrap", "stalechunk", "boundary", "nozero"]


def all_cases():
    """every shape of the device list as (W, capacity, cached, chunk, H, head_dim); W = 0: a linear state of capacity cached + chunk"""
    out = [(0, c + m, c, m, H, hd) for c, m, H, hd in LINEAR]
    out += [(0, c + m, c, m, RAGGED[2], RAGGED[3]) for c, m in zip(RAGGED[0], RAGGED[1])]
    return out + list(WINDOWED)


def track_qkv(cached, chunk, H, hd, dtype, seed=5):
    """[1, cached + chunk, 3 H hd] in T: tf_attn_bound.make_qkv's rows for that length"""
    return AB.make_qkv(1, cached + chunk, H, hd, dtype, seed)


def window_lo(p, W):
    return p - W + 1 if W > 0 and p >= W else 0


def pre_call_cache(k, v, cached, capacity, W, stale="garbage", rows=None):
    """k, v [B, H, L, hd] float32 -> kc, vc [B, H, rows, hd]: the cache in front of the call.  A ring keeps the last `capacity` keys below
    `cached`, key j in row j % capacity; a linear cache key j in row j.  Every other row holds the filler: "garbage" = finite values of
    the keys' size that belong to no key (what an older track or an older lap of the ring left), "nan" = NaN -- and then a ring's rows
    whose key lies below the window of the call's first query, which no query of the call sees, hold NaN too."""
    B, H, _, hd = k.shape
    rows = capacity if rows is None else rows
    g = torch.Generator().manual_seed(977 + cached * 31 + capacity)
    if stale == "nan":
        kc = torch.full((B, H, rows, hd), float("nan"))
        vc = torch.full((B, H, rows, hd), float("nan"))
    else:
        kc = (3.0 * torch.randn(B, H, rows, hd, generator=g)).half().float()
        vc = (3.0 * torch.randn(B, H, rows, hd, generator=g)).half().float()
    first = max(0, cached - capacity) if W > 0 else 0
    if stale == "nan":
        first = max(first, window_lo(cached, W))
    for j in range(first, cached):
        r = j % capacity if W > 0 else j
        kc[:, :, r] = k[:, :, j]
        vc[:, :, r] = v[:, :, j]
    return kc, vc


def _mm_rows(rows, qi, L, other):
    """rows [B, H, nq, K] @ other [B, H, K, N], each row computed inside a product of the shape the aligned emulations use for it: the
    32-query group of the whole track that holds query qi (min(32, L - group start) rows, the others zero here).  On the device a query's
    MFMA row does not depend on its neighbours; a CPU matrix product may pick another summation order for another row count (a
    single row is a matrix-vector product), and the bit comparison with the aligned emulations is about the walk, not about that."""
    B, H, _, K = rows.shape
    out = torch.empty(B, H, rows.shape[2], other.shape[-1])
    for a0 in range(int(qi[0]) & ~31, int(qi[-1]) + 1, 32):
        sel = ((qi >= a0) & (qi < a0 + 32)).nonzero().flatten()
        a = torch.zeros(B, H, min(32, L - a0), K)
        a[:, :, qi[sel] - a0] = rows[:, :, sel]
        out[:, :, sel] = (a @ other)[:, :, qi[sel] - a0]
    return out


def emulate(qkv, H, dtype, cached, W=0, capacity=None, mutation=None, stale="garbage"):
    """qkv [B, L, 3 d]: whole tracks of L tokens, of which rows `cached` .. L - 1 are the call's chunk -> the chunk's rows [B, L - cached,
    d] in T, by the kernel's walk.  mutation: None, or one defect
         alignedlast  a wave takes the steps up to (q0 & ~31) + 31 instead of q0 + 31: its last step is dropped when q0 is unaligned
         relmask      the causal / window mask taken on the chunk-relative query index
         nowrap       a cached key of a ring read from row j, not j % capacity (rows past the capacity: another track's)
         stalechunk   a chunk key read from the cache slot the append will write, which still holds what was there
         boundary     the cache / chunk boundary off by one: key `cached` read from the cache
         nozero       keys outside [lo_wg, Labs) not written as zeros: the cache row at that place as it is"""
    dt = AB.TDT[dtype]
    q, k, v = (t.float().contiguous() for t in AB.split_heads(qkv.cpu(), H))
    B, _, L, hd = q.shape
    pos0, ln = cached, L - cached
    capacity = L if capacity is None else capacity
    assert W > 0 or capacity >= L
    Labs = pos0 + ln
    rows = max(capacity, L + 192)                                     # room for the broken copies' reads past the capacity
    kc, vc = pre_call_cache(k, v, cached, capacity, W, stale, rows)
    slot = (lambda j: j % capacity) if W > 0 else (lambda j: j)
    zero = torch.zeros(B, H, hd)
    scale = torch.tensor(AB.LOG2E, dtype=torch.float32) / torch.sqrt(torch.tensor(float(hd)))
    ninf = torch.tensor(float("-inf"))
    out = torch.empty(B, H, ln, hd)
    for y in range((ln + 127) // 128):
        lo_wg = window_lo(pos0 + 128 * y, W)
        last_q = pos0 + min(128 * y + 127, ln - 1)

        def key_row(j):
            """(k row, v row) of key j in LDS: the key-source rule"""
            if j < lo_wg or j >= Labs:
                if mutation == "nozero":
                    return kc[:, :, slot(j)], vc[:, :, slot(j)]
                return zero, zero
            first_own = pos0 + 1 if mutation == "boundary" else pos0
            if j >= first_own and mutation != "stalechunk":
                return k[:, :, j], v[:, :, j]                         # chunk row j - pos0 of the packed qkv
            r = j if mutation == "nowrap" else slot(j)
            return kc[:, :, r], vc[:, :, r]

        images = {}
        for t in range(lo_wg // 64, last_q // 64 + 1):
            rws = [key_row(64 * t + r) for r in range(64)]
            images[t] = (torch.stack([a for a, _ in rws], dim=2), torch.stack([b for _, b in rws], dim=2))
        for w in range(4):
            i0 = 128 * y + 32 * w
            if i0 >= ln:
                break
            q0 = pos0 + i0
            nq = min(32, ln - i0)
            qi = torch.arange(q0, q0 + nq)
            qm = qi - pos0 if mutation == "relmask" else qi
            qw = q[:, :, q0:q0 + nq]
            m = torch.full((B, H, nq), float("-inf"))
            l = torch.zeros(B, H, nq)
            o = torch.zeros(B, H, nq, hd)
            top = (q0 & ~31) + 31 if mutation == "alignedlast" else q0 + 31
            for t in sorted(images):
                for kb in (64 * t, 64 * t + 32):
                    if kb >= Labs or kb > top or (W > 0 and kb + 31 < window_lo(q0, W)):
                        continue
                    ki, vi = (im[:, :, kb - 64 * t:kb - 64 * t + 32] for im in images[t])
                    keys = torch.arange(kb, kb + 32)
                    x = _mm_rows(qw, qi, L, ki.transpose(-1, -2)) * scale
                    seen = (keys[None, :] <= qm[:, None]) & (keys < Labs)[None, :]
                    if W > 0:
                        seen = seen & (keys[None, :] > qm[:, None] - W)
                    x = torch.where(seen, x, ninf)
                    mnew = torch.maximum(m, x.amax(dim=-1))
                    msafe = torch.where(mnew == ninf, torch.zeros(()), mnew) if W > 0 else mnew
                    alpha = torch.exp2(m - msafe)
                    p = torch.exp2(x - msafe[..., None])
                    l = l * alpha + p.sum(dim=-1)
                    o = o * alpha[..., None] + _mm_rows(p.to(dt).float(), qi, L, vi)
                    m = mnew
            out[:, :, i0:i0 + nq] = o * (1.0 / l)[..., None]
    return AB.merge_heads(out.to(dt))
