"""k_bucket_finish orders all the buckets that meet a tile in block-wide steps:
16-bit counters per (bucket, hash byte 0), FIN_GROUP buckets at a time. The
inputs here sit on what that adds: more buckets per tile than the counters
hold, counters at their limits, buckets against the tile and slack edges,
equal-h32 runs of every kind the cleanup rule tells apart. Every case runs
vega_dev_group_rows_i64 on the four-pass route (1) and the finish route (2)
and wants the same rows, row for row; values are the input row index.

Each input is described bucket by bucket (rows as (hash byte 0, key label) in
input order); test_inputs_have_their_shape checks, without a GPU, that the
keys hash to those buckets, digits and runs, and where they lie.
"""
import functools

import numpy as np
import pytest

import bucket_keys as bk
import finish_heads_keys as fh
import seg_layout as sl

FT = bk.FT
CAP = bk.BUCKET_CAP
GROUP = 56          # FIN_GROUP: buckets the counter array holds
SENTINEL = 0x5A5A5A5A5A5A5A5A


# ---- inputs ----

def fill(count, rng, avoid=()):
    """`count` rows of distinct keys on distinct digits outside `avoid`"""
    d = rng.choice(np.setdiff1d(np.arange(256), list(avoid)), size=count, replace=False)
    return [(int(x), ("f", i)) for i, x in enumerate(d)]


def run(digit, labels):
    """an equal-h32 run: one digit, keys by label, in input order"""
    return [(digit, ("r", digit, ch)) for ch in labels]


def from_buckets(buckets, seed):
    """Layout whose hash order has these buckets, in this order. Rows of equal
    h32 keep their order in the input; everything else is shuffled."""
    rng = np.random.RandomState(seed)
    nb = len(buckets)
    ids = np.sort(rng.choice(1 << 24, size=nb, replace=False))
    nkeys = 0
    hi_of = {}
    b_all, d_all, hi_all = [], [], []
    for bi, rows in enumerate(buckets):
        for digit, label in rows:
            key = (bi, label)
            if key not in hi_of:
                hi_of[key] = nkeys
                nkeys += 1
            b_all.append(ids[bi])
            d_all.append(digit)
            hi_all.append(hi_of[key])
    n = len(b_all)
    # distinct high words, spread: an odd multiplier is a bijection mod 2^32
    hi = (np.asarray(hi_all, dtype=np.uint64) * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)
    h64 = bk.make_h64(np.asarray(b_all), np.asarray(d_all), hi)
    pos = rng.permutation(n)
    h32 = (h64 & np.uint64(0xFFFFFFFF))
    order = np.argsort(h32, kind="stable")          # rows of equal h32, in spec order
    bounds = np.flatnonzero(np.concatenate([[True], h32[order][1:] != h32[order][:-1], [True]]))
    for s, e in zip(bounds[:-1], bounds[1:]):
        if e - s > 1:
            pos[order[s:e]] = np.sort(pos[order[s:e]])
    k = np.empty(n, dtype=np.uint64)
    k[pos] = h64
    lay = bk.Layout(bk.keys_for_hashes(k), [len(r) for r in buckets], [])
    lay.spec = buckets
    return lay


def around(n, fixed, seed):
    """buckets of the cycle's lengths, distinct keys, with the given row lists
    as buckets starting at the given rows: fixed = [(start, rows)]"""
    rng = np.random.RandomState(seed)
    lens = bk.lengths_with(n, [(s, len(rows)) for s, rows in fixed])
    starts = bk.bucket_starts(lens)
    special = {int(np.flatnonzero(starts == s)[0]): rows for s, rows in fixed}
    assert len(special) == len(fixed)
    return from_buckets([special.get(i) or fill(length, rng) for i, length in enumerate(lens)],
                        seed)


def group_loop(per_bucket):
    """3 FT + 77 rows; 1 row per bucket, or 2-3 with pairs and triples of equal
    h32 (AB, AA, ABC, AAB) among them: dozens of counter groups per tile"""
    n = 3 * FT + 77
    rng = np.random.RandomState(7)
    buckets, left, i = [], n, 0
    shapes = ("AB", "AA", "ABC", "AAB", "ABA")
    while left:
        length = 1 if per_bucket == 1 else min(2 + i % 2, left)
        if length >= 2 and i % 3 == 0:
            sh = shapes[(i // 3) % len(shapes)][:length]
            rows = run(int(rng.randint(256)), sh)
            rows += fill(length - len(rows), rng, avoid=[rows[0][0]])
        else:
            rows = fill(length, rng)
        buckets.append(rows)
        left -= length
        i += 1
    return from_buckets(buckets, 8)


N2 = 2 * FT + 100


def cases():
    """name -> (layout builder, route the finish request must end on)"""
    c = {
        "group_loop_1": (lambda: group_loop(1), 2),
        "group_loop_2_3": (lambda: group_loop(2), 2),
        # counter limits: one bucket at row 700 of a 2-tile input
        "cap_one_key_one_digit": (lambda: around(N2, [(700, run(9, "A" * 256))], 21), 2),
        "cap_two_keys_one_h32": (lambda: around(N2, [(700, run(9, "A" * 128 + "B" * 128))], 22), 2),
        "over_cap_257": (lambda: around(N2, [(700, run(9, "A" * 257))], 23), 1),
        "cap_all_digits": (lambda: around(N2, [(700, [(d, ("f", d)) for d in range(256)])], 24), 2),
        "cap_255_and_1": (lambda: around(N2, [(700, run(254, "A" * 255) + [(255, ("f", 0))])], 25), 2),
        "cap_255_and_1_top": (lambda: around(N2, [(700, run(3, "A" * 255) + [(4, ("f", 0))])], 26), 2),
    }
    # a 256-row bucket across the edge between tiles 0 and 1; 1 | 255 also ends
    # on the last row a closed bucket of tile 0 can have, 255 | 1 starts on the
    # first one of tile 1
    for left in (1, 128, 255):
        c[f"edge_{left}_{CAP - left}"] = (
            lambda left=left: around(N2, [(FT - left, fill(CAP, np.random.RandomState(left)))],
                                     30 + left), 2)
    c["edge_back_to_back_a"] = (lambda: around(N2, [
        (FT - 255, fill(CAP, np.random.RandomState(1))),
        (FT + 1, fill(CAP, np.random.RandomState(2)))], 41), 2)
    c["edge_back_to_back_b"] = (lambda: around(N2, [
        (FT - 255 - CAP, fill(CAP, np.random.RandomState(3))),
        (FT - 255, fill(CAP, np.random.RandomState(4)))], 42), 2)
    # one row longer than the slack closes (and than the cap)
    c["edge_open_right"] = (lambda: around(N2, [(FT - 1, run(0, "A" * 257))], 43), 1)
    c["edge_open_left"] = (lambda: around(N2, [(FT - 256, run(0, "A" * 257))], 44), 1)
    # span ends: first and last tile of 2- and 3-tile inputs
    for n in (2 * FT - 1, 2 * FT + 1, 3 * FT - 1, 3 * FT + 1):
        c[f"span_{n}"] = (lambda n=n: bk.build(bk.lengths_with(n, []), np.random.RandomState(n)), 2)
    # equal-h32 runs in the first, a middle and the last bucket meeting tile 1
    places = {"first": FT - 10, "middle": FT + 1000, "last": 2 * FT - 50}

    def with_run(labels, where, seed):
        rng = np.random.RandomState(seed)
        fixed = [(places[p], run(17, labels) + fill(100 - len(labels), rng, avoid=[17]))
                 for p in where]
        return around(3 * FT + 5, fixed, seed)
    c["run_ABA"] = (lambda: with_run("ABA", places, 51), 2)
    c["run_dirty_64"] = (lambda: with_run(("ABC" * 22)[:64], places, 52), 2)
    for p in places:
        c[f"run_dirty_65_{p}"] = (lambda p=p: with_run(("ABC" * 22)[:65], [p], 53), 1)
    return c


CASES = cases()


@functools.lru_cache(maxsize=None)
def layout(name):
    lay = CASES[name][0]()
    lay.k.setflags(write=False)
    return lay


# ---- without a GPU: the inputs are what they claim ----

def hash_order_shape(k):
    """bucket lengths in hash order, and per bucket {digit: [keys in input order]}"""
    h = bk.hash_u64(k)
    h32 = (h & np.uint64(0xFFFFFFFF)).astype(np.int64)
    o = np.argsort(h32, kind="stable")
    b = h32[o] >> 8
    starts = np.flatnonzero(np.concatenate([[True], b[1:] != b[:-1]]))
    return o, starts, np.diff(np.concatenate([starts, [len(k)]]))


@pytest.mark.parametrize("name", sorted(CASES))
def test_inputs_have_their_shape(name):
    lay = layout(name)
    o, starts, lens = hash_order_shape(lay.k)
    assert lens.tolist() == lay.lens and (np.sort(bk.bucket_of(lay.k)) == bk.bucket_of(lay.k[o])).all()
    if hasattr(lay, "spec"):
        digit = (bk.hash_u64(lay.k[o]) & np.uint64(0xFF)).astype(np.int64)
        for s, rows in zip(starts, lay.spec):
            assert sorted(digit[s:s + len(rows)].tolist()) == sorted(d for d, _ in rows)
            # a digit's rows, in input order, repeat keys exactly as the labels do
            for d in {d for d, _ in rows if sum(x == d for x, _ in rows) > 1}:
                labels = [lab for x, lab in rows if x == d]
                keys = lay.k[o[s:s + len(rows)][digit[s:s + len(rows)] == d]]
                assert len(keys) == len(labels)
                same_l = [[a == b for b in labels] for a in labels]
                same_k = (keys[:, None] == keys[None, :]).tolist()
                assert same_l == same_k


def test_claimed_positions():
    """where the special buckets lie against the tile and slack edges, and how
    many buckets meet a tile"""
    for name, per in (("group_loop_1", 1), ("group_loop_2_3", 3)):
        lens = layout(name).lens
        assert sum(lens) == 3 * FT + 77 and max(lens) == per
        assert FT // max(lens) > 10 * GROUP     # many turns of the group loop per tile
    for name in ("cap_one_key_one_digit", "cap_two_keys_one_h32", "cap_all_digits",
                 "cap_255_and_1", "cap_255_and_1_top", "over_cap_257"):
        lay = layout(name)
        at = bk.bucket_starts(lay.lens).tolist().index(700)
        assert lay.lens[at] == (257 if name == "over_cap_257" else 256)
        assert max(lay.lens[:at] + lay.lens[at + 1:]) <= CAP
    hist = np.bincount([d for d, _ in layout("cap_255_and_1").spec[
        bk.bucket_starts(layout("cap_255_and_1").lens).tolist().index(700)]], minlength=256)
    assert hist[254] == 255 and hist[255] == 1
    for left in (1, 128, 255):
        lay = layout(f"edge_{left}_{CAP - left}")
        at = bk.bucket_starts(lay.lens).tolist().index(FT - left)
        assert lay.lens[at] == CAP
    # 1 | 255: the next bucket's first row is the last staged row of tile 0
    lay = layout("edge_1_255")
    assert FT - 1 + CAP == FT + bk.BUCKET_CAP - 1 and (FT - 1 + CAP) in bk.bucket_starts(lay.lens)
    for name, s in (("edge_open_right", FT - 1), ("edge_open_left", FT - 256)):
        lay = layout(name)
        assert lay.lens[bk.bucket_starts(lay.lens).tolist().index(s)] == CAP + 1
    for name, ss in (("edge_back_to_back_a", (FT - 255, FT + 1)),
                     ("edge_back_to_back_b", (FT - 255 - CAP, FT - 255))):
        lay = layout(name)
        st = bk.bucket_starts(lay.lens).tolist()
        assert all(lay.lens[st.index(s)] == CAP for s in ss)
    for name in ("run_ABA", "run_dirty_64"):
        st = bk.bucket_starts(layout(name).lens).tolist()
        assert all(s in st for s in (FT - 10, FT + 1000, 2 * FT - 50))


# ---- on the GPU ----

def group_rows(k, v, route):
    import torch
    from vega_amd import gpu
    kt = torch.from_numpy(np.array(k)).cuda()
    vt = torch.from_numpy(np.array(v)).cuda()
    ok, ov = torch.empty_like(kt), torch.empty_like(vt)
    taken = gpu.dev_group_rows(kt, vt, route, ok, ov, gpu.alloc_ws(len(k)))
    return ok.cpu().numpy(), ov.cpu().numpy(), taken


@functools.lru_cache(maxsize=None)
def route1(name):
    lay = layout(name)
    r = group_rows(lay.k, lay.v, 1)
    assert r[2] == 1
    return r


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_finish_matches_four_pass_route(name):
    lay = layout(name)
    r1 = route1(name)
    r2 = group_rows(lay.k, lay.v, 2)
    assert r2[2] == CASES[name][1]
    assert (r2[0] == r1[0]).all(), f"keys differ at rows {np.flatnonzero(r2[0] != r1[0])[:8]}"
    assert (r2[1] == r1[1]).all(), f"values differ at rows {np.flatnonzero(r2[1] != r1[1])[:8]}"
    # a permutation of the input with equal keys adjacent
    assert (lay.k[r2[1]] == r2[0]).all() and (np.sort(r2[1]) == lay.v).all()
    assert 1 + int((r2[0][1:] != r2[0][:-1]).sum()) == len(np.unique(lay.k))


@pytest.mark.gpu
@pytest.mark.parametrize("op", ["SUM_I64", "COUNT", "MIN_I64", "MAX_I64"])
def test_sort_reduce_on_group_loop_input(op):
    """through the public entry, into sentinel-filled outputs; the oracle is
    the finish route's rows (the sample decides the automatic route)"""
    import torch
    from vega_amd import gpu
    opn = sl.OPS[op]
    lay = layout("group_loop_2_3")
    gk, gv, taken = group_rows(lay.k, lay.v, 2)
    assert taken == 2
    assert (gk == route1("group_loop_2_3")[0]).all() and (gv == route1("group_loop_2_3")[1]).all()
    v = fh.values_for(opn, lay.n, seed=17 + opn)
    kt = torch.from_numpy(np.array(lay.k)).cuda()
    vt = torch.from_numpy(np.array(v).view(np.int64)).cuda()
    out_k = torch.full_like(kt, SENTINEL)
    out_v = torch.full_like(kt, SENTINEL)
    nout = gpu.dev_sort_reduce(kt, vt, opn, out_k, out_v, gpu.alloc_ws(lay.n))
    torch.cuda.synchronize()
    ek, ev = fh.reduce_in_order(opn, gk, v[gv])
    assert nout == len(ek) and nout < lay.n
    assert (out_k[:nout].cpu().numpy() == ek).all()
    assert (out_v[:nout].cpu().numpy() == ev.view(np.int64)).all()
    assert (out_v[nout:].cpu().numpy() == SENTINEL).all(), "stores beyond the last segment"
