"""Inputs whose FINAL (grouped) row order is chosen row by row, for the head
counts k_bucket_finish hands to the segmented reduce.

Every distinct key gets its own h32, so the finish route's order is simply the
stable order by h32 = (bucket << 8 | byte 0): a layout is a list of run
lengths in final order plus the final rows at which a new bucket starts, and
the keys follow from bucket_keys.keys_for_hashes. Runs of equal keys are put
against the edges the kernels distinguish: the 2048-row finish tile, the
4096-row tile and the 8-row chunk of the segmented reduce.

Pure numpy; checked in test_finish_heads_keys.py.
"""
import numpy as np

import bucket_keys as bk

FT = bk.FT          # finish tile
SEG_TILE = 2 * FT   # segmented-reduce tile
CHUNK = 8

SIZES = (3 * FT + 37, 5 * FT - 3)   # 4 and 5 finish tiles; neither a multiple of 8
BUCKET_TARGETS = (48, 64, 80, 33, 100)   # a bucket closes at the first run start past its target

OP_SUM_I64, OP_COUNT, OP_SUM_F64, OP_MIN_I64, OP_MAX_I64 = range(5)


def special_runs(n):
    """(first final row, rows, starts a bucket) of the planted runs, ascending;
    test_finish_heads_keys.py checks them against the edges"""
    runs = [(7, 2, False),               # 2 rows across the chunk edge at row 8
            (100, 9, False),             # 9 rows across the chunk edge at row 104
            (FT - 20, 40, False),        # straddles the finish-tile edge at 2048
            (2 * FT - 17, 40, False)]    # straddles 4096, a seg-tile edge as well
    if n == 3 * FT + 37:
        runs += [(3 * FT - 1, 1, False),     # head (and only row) on a tile's last row
                 (3 * FT, 9, True)]          # head on a tile's first row, a bucket starts there
    else:
        assert n == 5 * FT - 3
        runs += [(3 * FT - 1, 3, False),     # head on a tile's last row, goes on into the next
                 (4 * FT, 9, True)]          # head on a tile's first row, a bucket starts there
    return runs


class FinalLayout:
    """k: input rows; final_k: the keys in final order; run_lens / run_start:
    the runs in final order; bucket_start: final rows where a bucket starts"""

    def __init__(self, k, final_k, run_lens, bucket_start):
        self.k = k
        self.n = len(k)
        self.final_k = final_k
        self.run_lens = run_lens
        self.run_start = np.concatenate([[0], np.cumsum(run_lens)[:-1]]).astype(np.int64)
        self.bucket_start = bucket_start


def run_lengths(n, special):
    lens, pos = [], 0
    for s, length, _ in special:
        assert s >= pos
        lens += [1] * (s - pos) + [length]
        pos = s + length
    assert pos <= n
    return np.asarray(lens + [1] * (n - pos), dtype=np.int64)


def bucket_breaks(run_start, run_lens, forced):
    """indices of the runs that open a bucket"""
    opens, cur, t = [0], 0, 0
    for i in range(1, len(run_start)):
        if int(run_start[i]) in forced or run_start[i] - cur >= BUCKET_TARGETS[t % len(BUCKET_TARGETS)]:
            opens.append(i)
            cur = int(run_start[i])
            t += 1
    return np.asarray(opens, dtype=np.int64)


def build(n, seed, runs=True, minus1=True):
    """FinalLayout of n rows; runs=False keeps every key distinct (SUM_F64)"""
    special = special_runs(n) if runs else []
    lens = run_lengths(n, special)
    start = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    opens = bucket_breaks(start, lens, {s for s, _, b in special if b})
    nbk = len(opens)
    run_bucket = np.searchsorted(opens, np.arange(len(lens)), side="right") - 1
    bucket_rows = np.add.reduceat(lens, opens)
    assert bucket_rows.max() <= bk.BUCKET_CAP
    h_m1 = int(bk.hash_u64(np.array([-1]))[0])
    b_m1, c_m1 = (h_m1 >> 8) & 0xFFFFFF, h_m1 & 0xFF
    for attempt in range(64):
        rng = np.random.RandomState(seed + 1000 * attempt)
        ids = set([b_m1]) if minus1 else set()
        while len(ids) < nbk:
            ids.update(rng.randint(0, 1 << 24, size=nbk - len(ids)).tolist())
        ids = np.sort(np.fromiter(ids, dtype=np.int64))
        byte0 = np.empty(len(lens), dtype=np.int64)
        hi32 = bk.draw_hi32(rng, len(lens))
        ok = True
        for b in range(nbk):
            mine = np.flatnonzero(run_bucket == b)
            if minus1 and ids[b] == b_m1:
                # key -1 sorts where its byte 0 falls: that run must be a plain row
                others = rng.choice(np.setdiff1d(np.arange(256), [c_m1]), size=len(mine) - 1,
                                    replace=False)
                c = np.sort(np.concatenate([others, [c_m1]]))
                at = mine[int(np.flatnonzero(c == c_m1)[0])]
                if lens[at] != 1:
                    ok = False
                    break
                hi32[at] = h_m1 >> 32
            else:
                c = np.sort(rng.choice(256, size=len(mine), replace=False))
            byte0[mine] = c
        if ok:
            break
    assert ok, "no bucket draw put key -1 on a single-row run"
    run_h = bk.make_h64(ids[run_bucket], byte0, hi32)
    h32 = run_h & np.uint64(0xFFFFFFFF)
    assert (np.diff(h32.astype(np.int64)) > 0).all(), "runs must ascend in h32, all distinct"
    single = lens == 1
    held = [np.repeat(run_h[i], lens[i]) for i in np.flatnonzero(~single)]
    k = bk.keys_for_hashes(bk.place(run_h[single], held, rng))
    final_k = bk.keys_for_hashes(np.repeat(run_h, lens))
    return FinalLayout(k, final_k, lens, start[opens])


def values_for(op, n, seed):
    """int64 values: full range for the sum (it wraps), extremes among +-2^40
    for min and max; f64 values for SUM_F64"""
    rng = np.random.RandomState(seed)
    if op == OP_SUM_F64:
        return rng.uniform(-1.0, 1.0, size=n)
    if op == OP_SUM_I64:
        return rng.randint(np.iinfo(np.int64).min, np.iinfo(np.int64).max, size=n, dtype=np.int64)
    v = rng.randint(-(1 << 40), 1 << 40, size=n, dtype=np.int64)
    v[rng.randint(0, n, size=16)] = np.iinfo(np.int64).min
    v[rng.randint(0, n, size=16)] = np.iinfo(np.int64).max
    return v


def reduce_in_order(op, gk, vals):
    """segmented reduce of grouped rows (gk, vals), output in their order"""
    starts = np.flatnonzero(np.concatenate([[True], gk[1:] != gk[:-1]]))
    lens = np.diff(np.concatenate([starts, [len(gk)]]))
    if op == OP_COUNT:
        return gk[starts], lens.astype(np.int64)
    if op == OP_SUM_I64:
        return gk[starts], np.add.reduceat(vals.view(np.uint64), starts).view(np.int64)
    if op == OP_MIN_I64:
        return gk[starts], np.minimum.reduceat(vals, starts)
    if op == OP_MAX_I64:
        return gk[starts], np.maximum.reduceat(vals, starts)
    assert (lens == 1).all()     # f64: one row per key, the sum is the row
    return gk[starts], vals[starts]
