"""Inputs with a KNOWN grouped layout for the segmented-reduce tests.

The seg_reduce kernels (k_head_count + k_seg_emit<OP,PK> + k_f64_seg_combine)
pick their code path from where a run of equal keys falls relative to an 8-row
chunk, a 64-chunk wave and a 4096-row tile of the GROUPED rows. This module
builds shuffled inputs whose grouped order is predictable, says which of those
paths a layout reaches (`coverage`), and holds plain numpy reference reducers.

Pure numpy: used by the CPU test (test_seg_layout.py) and the GPU tests
(test_gpu_segreduce.py, test_gpu_groupsort_paths.py).

Grouped order, by strategy of group_sort_u64:
  narrow (<= 5 active key bytes): stable LSD radix over the active bytes, so
      runs appear in ascending (unsigned) key order;
  hash   (wide keys, n <= 2^30): four stable passes over the low four bytes of
      splitmix64(key), so runs appear in ascending h32(key). When all h32 are
      distinct the cleanup kernel has nothing to move and the order is exact.
Both sorts are stable, so inside a run the rows keep their input order.
"""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vega_amd.shuffle import hash_u64_np  # noqa: E402

CHUNK = 8        # SEG_IPT rows per thread
WAVE = 64 * CHUNK   # 512 rows per wave
TILE = 4096      # SEG_B * SEG_IPT rows per workgroup

OP_SUM_I64, OP_COUNT, OP_SUM_F64, OP_MIN_I64, OP_MAX_I64 = range(5)
OPS = {"SUM_I64": OP_SUM_I64, "COUNT": OP_COUNT, "SUM_F64": OP_SUM_F64,
       "MIN_I64": OP_MIN_I64, "MAX_I64": OP_MAX_I64}

I64_MIN = np.iinfo(np.int64).min
I64_MAX = np.iinfo(np.int64).max


def h32(keys):
    return hash_u64_np(np.asarray(keys, dtype=np.int64)) & np.uint64(0xFFFFFFFF)


def active_bytes(keys):
    """byte positions in which the keys take more than one value"""
    u = np.asarray(keys, dtype=np.int64).view(np.uint64)
    return [p for p in range(8)
            if len(np.unique((u >> np.uint64(8 * p)) & np.uint64(0xFF))) > 1]


# --------------------------------------------------------------------------
# layout builder

class Layout:
    """k, row_run: shuffled input rows (key, index of the run the row is in);
    order: run indices in predicted grouped order; glens: run lengths in that
    order; gpos: the grouped position of every input row; pos_in_run: rank of
    the row inside its run (== its rank in the grouped run: stable sorts)."""

    def __init__(self, k, row_run, order, run_lens, strategy):
        self.k = k
        self.row_run = row_run
        self.order = order
        self.strategy = strategy
        self.run_lens = run_lens
        self.glens = run_lens[order]
        n = len(k)
        by_run = np.argsort(row_run, kind="stable")
        first = np.concatenate([[0], np.cumsum(run_lens)[:-1]])
        self.pos_in_run = np.empty(n, dtype=np.int64)
        self.pos_in_run[by_run] = np.arange(n) - first[row_run[by_run]]
        gstart = np.empty(len(run_lens), dtype=np.int64)
        gstart[order] = np.concatenate([[0], np.cumsum(self.glens)[:-1]])
        self.gstart = gstart   # grouped first row of run i (indexed by run)
        self.gpos = gstart[row_run] + self.pos_in_run
        self.keys = None       # filled by build()

    @property
    def n(self):
        return len(self.k)


def build(run_lens, keys, rng, strategy):
    """Shuffled rows with run i = run_lens[i] copies of keys[i], plus the
    predicted grouped order of the runs under `strategy` ("narrow"/"hash")."""
    run_lens = np.asarray(run_lens, dtype=np.int64)
    keys = np.asarray(keys, dtype=np.int64)
    assert len(run_lens) == len(keys) and (run_lens > 0).all()
    assert len(np.unique(keys)) == len(keys), "run keys must be distinct"
    if strategy == "narrow":
        assert len(active_bytes(keys)) <= 5
        order = np.argsort(keys.view(np.uint64), kind="stable")
    elif strategy == "hash":
        assert len(active_bytes(keys)) > 5
        hh = h32(keys)
        assert len(np.unique(hh)) == len(hh), "h32 collision: redraw the keys"
        order = np.argsort(hh, kind="stable")
    else:
        raise ValueError(strategy)
    row_run = np.repeat(np.arange(len(keys), dtype=np.int64), run_lens)
    row_run = row_run[rng.permutation(len(row_run))]
    lay = Layout(keys[row_run], row_run, order, run_lens, strategy)
    lay.keys = keys
    return lay


def draw_wide_keys(count, rng, h32_below=None, lo=1 << 40, hi=1 << 62):
    """`count` distinct keys in [lo, hi) with pairwise distinct h32 (redrawn
    until they are); with h32_below, every h32 is smaller than that bound"""
    out = np.empty(0, dtype=np.int64)
    while len(out) < count:
        c = rng.randint(lo, hi, size=4 * count + 64, dtype=np.int64)
        if h32_below is not None:
            c = c[h32(c) < np.uint64(h32_below)]
        out = np.concatenate([out, c])
        _, first = np.unique(out, return_index=True)
        out = out[np.sort(first)]
        _, first = np.unique(h32(out), return_index=True)
        out = out[np.sort(first)]
    return out[:count]


# --------------------------------------------------------------------------
# which kernel paths a grouped layout reaches

COVERAGE_KEYS = (
    "start_at_chunk_start", "end_at_chunk_end", "start_at_tile_start",
    "start_on_tile_last_row", "cross_tile_edge", "cross_wave_edge_in_tile",
    "headfree_chunks_ge2", "headfree_chunks_ge64", "headfree_chunks_ge512",
    "fast_chunk_even_slot", "fast_chunk_odd_slot", "distinct_chunk_continues",
)


def coverage(lens):
    """Counts of runs / chunks per kernel path for run lengths `lens` given in
    grouped order. A "head" is the first row of a run. The row after the last
    one counts as a head (the kernel treats the end of the data that way)."""
    lens = np.asarray(lens, dtype=np.int64)
    n = int(lens.sum())
    e = np.cumsum(lens)          # one past the last row
    s = e - lens                 # first row
    last = e - 1
    waves_in = last // WAVE - s // WAVE      # multiples of 512 in (s, last]
    tiles_in = last // TILE - s // TILE      # multiples of 4096 in (s, last]
    headfree = np.maximum(0, e // CHUNK - (s // CHUNK + 1))
    head = np.zeros(n + 1, dtype=bool)
    head[s] = True
    head[n] = True
    slot = np.cumsum(head[:n]) - 1           # output slot of each row's run
    full = n // CHUNK
    allheads = head[:full * CHUNK].reshape(full, CHUNK).all(axis=1)
    c0 = np.arange(full) * CHUNK
    next_head = head[c0 + CHUNK]
    fast = allheads & next_head
    odd = (slot[c0] & 1) == 1
    return {
        "start_at_chunk_start": int((s % CHUNK == 0).sum()),
        "end_at_chunk_end": int((e % CHUNK == 0).sum()),
        "start_at_tile_start": int((s % TILE == 0).sum()),
        "start_on_tile_last_row": int((s % TILE == TILE - 1).sum()),
        "cross_tile_edge": int((tiles_in > 0).sum()),
        "cross_wave_edge_in_tile": int((waves_in - tiles_in > 0).sum()),
        "headfree_chunks_ge2": int((headfree >= 2).sum()),
        "headfree_chunks_ge64": int((headfree >= 64).sum()),
        "headfree_chunks_ge512": int((headfree >= 512).sum()),
        "fast_chunk_even_slot": int((fast & ~odd).sum()),
        "fast_chunk_odd_slot": int((fast & odd).sum()),
        "distinct_chunk_continues": int((allheads & ~next_head).sum()),
        "n_mod_chunk": n % CHUNK,
    }


# --------------------------------------------------------------------------
# reference reducers (stable argsort + reduceat)

def _runs(k):
    k = np.asarray(k, dtype=np.int64)
    order = np.argsort(k, kind="stable")
    ks = k[order]
    starts = np.flatnonzero(np.concatenate([[True], ks[1:] != ks[:-1]])) \
        if len(ks) else np.empty(0, dtype=np.int64)
    return order, ks, starts


def reduce_ref(op, k, v=None):
    """(keys ascending, reduced values) for the integer ops"""
    order, ks, starts = _runs(k)
    if len(ks) == 0:
        return ks, np.empty(0, dtype=np.int64)
    if op == OP_COUNT:
        return ks[starts], np.diff(np.concatenate([starts, [len(ks)]])).astype(np.int64)
    vs = np.asarray(v, dtype=np.int64)[order]
    if op == OP_SUM_I64:   # uint64 so that the sum wraps like the kernel's
        out = np.add.reduceat(vs.view(np.uint64), starts).view(np.int64)
    elif op == OP_MIN_I64:
        out = np.minimum.reduceat(vs, starts)
    elif op == OP_MAX_I64:
        out = np.maximum.reduceat(vs, starts)
    else:
        raise ValueError(op)
    return ks[starts], out


def sum_f64_ref(k, v):
    """(keys ascending, math.fsum per key, sum|v| per key, rows per key)"""
    order, ks, starts = _runs(k)
    vs = np.asarray(v, dtype=np.float64)[order]
    parts = np.split(vs, starts[1:])
    fs = np.array([math.fsum(p.tolist()) for p in parts], dtype=np.float64)
    sabs = np.array([math.fsum(np.abs(p).tolist()) for p in parts], dtype=np.float64)
    lens = np.diff(np.concatenate([starts, [len(ks)]])).astype(np.int64)
    return ks[starts], fs, sabs, lens


def exact_int_sums(k, v):
    """(keys ascending, per-key sums as unbounded Python ints): an independent
    statement of SUM_I64 before wrapping (split 32/32 so int64 never overflows)"""
    order, ks, starts = _runs(k)
    vs = np.asarray(v, dtype=np.int64)[order]
    hi = np.add.reduceat(vs >> 32, starts)
    lo = np.add.reduceat(vs & 0xFFFFFFFF, starts)
    return ks[starts], [int(h) * (1 << 32) + int(l) for h, l in zip(hi, lo)]


def sorted_pairs(k, v):
    return sorted(zip(np.asarray(k).tolist(), np.asarray(v).tolist()))


# --------------------------------------------------------------------------
# the fixed inputs of the GPU tests

def _filler(out, upto):
    """append short runs (cycling lengths, so heads land on every chunk phase)
    until the layout is exactly `upto` rows long"""
    cyc = (1, 2, 3, 5, 7, 9, 4, 17, 1, 6, 11)
    pos = sum(out)
    i = 0
    assert pos <= upto
    while pos < upto:
        ln = min(cyc[i % len(cyc)], upto - pos)
        out.append(ln)
        pos += ln
        i += 1


# named rows of the hand-placed SoA layout; test_seg_layout.py checks each
SOA_MARKS = {}


def soa_run_lens(tail_rows):
    """Hand-placed run lengths, in grouped (= key) order; key = run index.
    tail_rows 0 -> n % 8 == 0, 3 -> n % 8 == 3."""
    L = []
    m = SOA_MARKS
    L += [1] * 8                 # rows 0..7: fast chunk, first slot 0 (even)
    m["fast_even"] = 0
    L += [8]                     # rows 8..15: a run of exactly one chunk
    m["one_chunk_run"] = 8
    L += [1] * 8                 # rows 16..23: fast chunk, first slot 9 (odd)
    m["fast_odd"] = 16
    L += [1] * 7 + [12]          # rows 24..31 all heads; the last run goes on to row 42
    m["distinct_continues"] = 24
    L += [3, 2]                  # rows 43..47
    _filler(L, 512)
    L += [512]                   # rows 512..1023: a run of exactly one wave
    m["one_wave_run"] = 512
    _filler(L, 1524)
    L += [30]                    # rows 1524..1553: crosses the wave edge at 1536
    m["cross_wave"] = 1524
    _filler(L, 1605)
    L += [600]                   # rows 1605..2204: > 64 whole head-free chunks
    m["long_in_tile"] = 1605
    _filler(L, 4090)
    L += [5]                     # rows 4090..4094
    L += [1]                     # row 4095: starts and ends on the tile's last row
    m["tile_last_row_len1"] = 4095
    L += [4096]                  # rows 4096..8191: exactly one tile
    m["one_tile_run"] = 4096
    L += [1] * 8                 # rows 8192..8199: fast chunk at a tile start
    _filler(L, 8292)
    L += [16384 + 37 - 8292]     # rows 8292..16420: tile 3 holds no head at all
    m["headless_tile_run"] = 8292
    _filler(L, 20479)
    L += [10]                    # rows 20479..20488: starts on a tile's last row
    m["tile_last_row_cross"] = 20479
    _filler(L, 20536)
    L += [1] * 8                 # rows 20536..20543: fast chunk that ends the data
    m["fast_at_end"] = 20536
    assert sum(L) == 20544
    if tail_rows:
        assert tail_rows == 3
        L += [1, 2]              # guarded tail chunk with two heads
    return np.asarray(L, dtype=np.int64)


# hash-layout menu: 155,365 rows in 3,691 runs
HASH_MENU = ([1] * 3400
             + [ln for ln in (2, 3, 7, 8, 9, 15, 16, 17, 63, 64, 65, 511, 512, 513)
                for _ in range(20)]
             + [ln for ln in (4095, 4096, 4097) for _ in range(3)]
             + [9000, 70001])
H32_MINUS1 = 0x1B652C20      # h32(-1); checked in test_seg_layout.py
HASH_SEED = {True: 1, False: 3}  # per variant; coverage asserted in test_seg_layout.py


def soa_layout(tail_rows):
    lens = soa_run_lens(tail_rows)
    rng = np.random.RandomState(100 + tail_rows)
    return build(lens, np.arange(len(lens), dtype=np.int64), rng, "narrow")


def hash_layout(with_minus1):
    """wide keys laid out in h32 order. with_minus1: the LAST grouped run is a
    9-row run of key -1 (~0, the kernel's pad value); every other key's h32 is
    below h32(-1)."""
    lens = np.asarray(HASH_MENU, dtype=np.int64)
    rng = np.random.RandomState(HASH_SEED[with_minus1])
    if with_minus1:
        keys = draw_wide_keys(len(lens), rng, h32_below=H32_MINUS1)
        nine = int(np.flatnonzero(lens == 9)[0])
        keys[nine] = -1
    else:
        keys = draw_wide_keys(len(lens), rng)
    return build(lens, keys, rng, "hash")


# --------------------------------------------------------------------------
# values

# what the MIN/MAX values plant in a run, by class
(CL_PLAIN, CL_MIN_FIRST, CL_MAX_FIRST, CL_MIN_LAST, CL_MAX_LAST,
 CL_MIN_LATER_CHUNK, CL_MAX_LATER_CHUNK, CL_ALL_MAX, CL_ALL_MIN) = range(9)


def minmax_classes(lay):
    """class per run: cycles through the classes, except that the runs which
    cross a tile edge carry their extremum deep inside (alternately MIN and
    MAX, longest run first), so that it can sit in a later tile"""
    nr = len(lay.run_lens)
    cls = (np.arange(nr) * 5 + 1) % 9
    crossing = np.flatnonzero(lay.gstart // TILE != (lay.gstart + lay.run_lens - 1) // TILE)
    crossing = crossing[np.argsort(-lay.run_lens[crossing], kind="stable")]
    cls[crossing[0::2]] = CL_MIN_LATER_CHUNK
    cls[crossing[1::2]] = CL_MAX_LATER_CHUNK
    return cls


def later_chunk_pos(lay):
    """per run: a position inside the run whose GROUPED row lies in another
    chunk than the run's first row (2/3 into the run), or -1 if there is none"""
    pos = (lay.run_lens * 2) // 3
    ok = (lay.gstart + pos) // CHUNK != lay.gstart // CHUNK
    return np.where(ok, pos, -1)


def values_minmax(lay, rng):
    v = rng.randint(-(1 << 40), 1 << 40, size=lay.n, dtype=np.int64)
    cls = minmax_classes(lay)[lay.row_run]
    p = lay.pos_in_run
    ln = lay.run_lens[lay.row_run]
    later = later_chunk_pos(lay)[lay.row_run]
    v[(cls == CL_MIN_FIRST) & (p == 0)] = I64_MIN
    v[(cls == CL_MAX_FIRST) & (p == 0)] = I64_MAX
    v[(cls == CL_MIN_LAST) & (p == ln - 1)] = I64_MIN
    v[(cls == CL_MAX_LAST) & (p == ln - 1)] = I64_MAX
    v[(cls == CL_MIN_LATER_CHUNK) & (p == later)] = I64_MIN
    v[(cls == CL_MAX_LATER_CHUNK) & (p == later)] = I64_MAX
    v[cls == CL_ALL_MAX] = I64_MAX
    v[cls == CL_ALL_MIN] = I64_MIN
    return v


def values_sum_i64(lay, rng):
    """full-range values: runs of a few rows already wrap past 2^63"""
    return rng.randint(I64_MIN, I64_MAX, size=lay.n, dtype=np.int64)


def values_f64_integral(lay, rng):
    """integer-valued doubles, |v| <= 2^30: per-key sum|v| < 2^53 for runs
    shorter than 2^23 rows, so the sum is exact in any order"""
    return rng.randint(-(1 << 30), (1 << 30) + 1, size=lay.n).astype(np.float64)


def values_f64_mixed(lay, rng):
    """mixed sign, magnitudes spread over nine decades"""
    return rng.standard_normal(lay.n) * 10.0 ** rng.randint(-3, 6, size=lay.n)
