"""CPU checks of tests/seg_layout.py: the coverage counter against a per-row
walk, the reference reducers against pyref / the C oracle, and — what keeps
the GPU tests honest — that every fixed input they use really reaches the
kernel paths it is meant to reach."""
import numpy as np
import pytest

import oracle_ctypes as oc
import pyref
import seg_layout as sl


# ---------------- coverage vs a brute-force walk ----------------

def coverage_walk(lens):
    lens = [int(x) for x in lens]
    n = sum(lens)
    c = dict.fromkeys(sl.COVERAGE_KEYS, 0)
    heads = set()
    s = 0
    for ln in lens:
        e = s + ln
        heads.add(s)
        c["start_at_chunk_start"] += s % 8 == 0
        c["end_at_chunk_end"] += (e - 1) % 8 == 7
        c["start_at_tile_start"] += s % 4096 == 0
        c["start_on_tile_last_row"] += s % 4096 == 4095
        # an edge is crossed when a row after the first starts a tile / wave
        c["cross_tile_edge"] += any(r % 4096 == 0 for r in range(s + 1, e))
        c["cross_wave_edge_in_tile"] += any(r % 512 == 0 and r % 4096 != 0
                                            for r in range(s + 1, e))
        hf = 0
        for ch in range(s // 8, e // 8 + 1):
            rows = range(8 * ch, 8 * ch + 8)
            hf += all(s < r < e for r in rows)
        c["headfree_chunks_ge2"] += hf >= 2
        c["headfree_chunks_ge64"] += hf >= 64
        c["headfree_chunks_ge512"] += hf >= 512
        s = e
    slot = -1
    for ch in range(n // 8):
        rows = range(8 * ch, 8 * ch + 8)
        first_slot = slot + 1 if 8 * ch in heads else slot
        slot += sum(r in heads for r in rows)
        if not all(r in heads for r in rows):
            continue
        nxt = 8 * ch + 8
        if nxt == n or nxt in heads:
            c["fast_chunk_odd_slot" if first_slot & 1 else "fast_chunk_even_slot"] += 1
        else:
            c["distinct_chunk_continues"] += 1
    c["n_mod_chunk"] = n % 8
    return c


HAND_LAYOUTS = {
    "one_row": [1],
    "one_chunk_distinct": [1] * 8,
    "distinct_then_more": [1] * 16 + [3],
    "odd_slot_fast": [3, 5] + [1] * 8 + [2],
    "distinct_continues": [1] * 7 + [9] + [1] * 8,
    "run_is_chunk": [8, 8, 16, 7, 1, 4],
    "tile_edges": [4095, 1, 4096, 1, 4094, 2, 10],
    "wave_edges": [500, 24, 512, 511, 1, 1030, 5],
    "long": [3, 4096 + 4096 + 20, 77, 8 * 70 + 1],
}


@pytest.mark.parametrize("name", sorted(HAND_LAYOUTS))
def test_coverage_matches_walk_hand_made(name):
    lens = HAND_LAYOUTS[name]
    assert sl.coverage(lens) == coverage_walk(lens)


def test_coverage_hand_counted():
    # rows 0..7 distinct (slot 0), next row a head -> one even fast chunk;
    # rows 8..15 one run: starts at a chunk start, ends at a chunk end
    c = sl.coverage([1] * 8 + [8] + [1] * 8 + [3])
    assert c["fast_chunk_even_slot"] == 1
    assert c["fast_chunk_odd_slot"] == 1        # rows 16..23, first slot 9
    assert c["start_at_chunk_start"] == 4       # rows 0, 8, 16, 24
    assert c["end_at_chunk_end"] == 3           # rows 7, 15, 23
    assert c["distinct_chunk_continues"] == 0
    assert c["n_mod_chunk"] == 3
    c = sl.coverage([4095, 2, 4095 + 512 * 8])
    assert c["start_on_tile_last_row"] == 1 and c["cross_tile_edge"] == 2
    assert c["headfree_chunks_ge512"] == 1 and c["headfree_chunks_ge64"] == 2


def test_coverage_matches_walk_random_and_fixed():
    rng = np.random.RandomState(5)
    for _ in range(3):
        lens = rng.choice([1, 1, 1, 1, 2, 3, 7, 8, 9, 64, 513, 4097], size=120)
        assert sl.coverage(lens) == coverage_walk(lens)
    for tail in (0, 3):
        lens = sl.soa_run_lens(tail)
        assert sl.coverage(lens) == coverage_walk(lens)


# ---------------- reducers vs pyref / the C oracle ----------------

@pytest.mark.parametrize("bits", [3, 10, 64])
def test_reducers_match_pyref_and_oracle(bits):
    rng = np.random.RandomState(bits)
    n = 5000
    if bits == 64:
        k = rng.randint(sl.I64_MIN, sl.I64_MAX, size=n, dtype=np.int64)
        k[::3] = k[1::3][: len(k[::3])]      # some duplicates among wide keys
    else:
        k = rng.randint(0, 1 << bits, size=n, dtype=np.int64)
    v = rng.randint(sl.I64_MIN, sl.I64_MAX, size=n, dtype=np.int64)

    rk, rv = sl.reduce_ref(sl.OP_SUM_I64, k, v)
    assert dict(zip(rk.tolist(), rv.tolist())) == pyref.reduce_by_key(k, v)
    ok, ov = oc.reduce_by_key_i64(k, v, 4, 4)
    assert sl.sorted_pairs(rk, rv) == sl.sorted_pairs(ok, ov)
    ek, ev = sl.exact_int_sums(k, v)
    assert (ek == rk).all()
    assert [((x + (1 << 63)) % (1 << 64)) - (1 << 63) for x in ev] == rv.tolist()

    ck, cv = sl.reduce_ref(sl.OP_COUNT, k)
    assert dict(zip(ck.tolist(), cv.tolist())) == pyref.group_count(k)
    ok, ov = oc.group_count_i64(k, v, 4, 4)
    assert sl.sorted_pairs(ck, cv) == sl.sorted_pairs(ok, ov)

    groups = pyref.group_by_key(k, v)
    mk, mv = sl.reduce_ref(sl.OP_MIN_I64, k, v)
    assert dict(zip(mk.tolist(), mv.tolist())) == {g: min(x) for g, x in groups.items()}
    mk, mv = sl.reduce_ref(sl.OP_MAX_I64, k, v)
    assert dict(zip(mk.tolist(), mv.tolist())) == {g: max(x) for g, x in groups.items()}

    f = rng.standard_normal(n) * 10.0 ** rng.randint(-3, 6, size=n)
    fk, fs, sabs, lens = sl.sum_f64_ref(k, f)
    assert (fk == ck).all() and (lens == cv).all()
    ok, ov = oc.reduce_by_key_f64(k, f, 4, 4)
    ref = dict(zip(ok.tolist(), ov.tolist()))
    for key, s, a, ln in zip(fk.tolist(), fs.tolist(), sabs.tolist(), lens.tolist()):
        # the oracle sums sequentially: within the any-order bound of fsum
        assert abs(ref[key] - s) <= ln * 2.0 ** -52 * a
        assert a >= abs(s)


def test_reducers_empty_and_single():
    e = np.empty(0, dtype=np.int64)
    for op in (sl.OP_SUM_I64, sl.OP_COUNT, sl.OP_MIN_I64, sl.OP_MAX_I64):
        rk, rv = sl.reduce_ref(op, e, e)
        assert len(rk) == 0 and len(rv) == 0
    rk, rv = sl.reduce_ref(sl.OP_SUM_I64, [7], [sl.I64_MIN])
    assert rk.tolist() == [7] and rv.tolist() == [sl.I64_MIN]


# ---------------- the builder ----------------

def _check_prediction(lay, sort_key):
    """sorting the input rows stably by `sort_key` must give exactly the
    predicted grouped rows: runs in `order`, rows of a run in input order"""
    grouped = np.argsort(sort_key, kind="stable")
    assert (lay.k[grouped] == np.repeat(lay.keys[lay.order], lay.glens)).all()
    assert (lay.gpos[grouped] == np.arange(lay.n)).all()
    # a run's rows keep their input order
    assert (lay.pos_in_run[grouped] ==
            np.arange(lay.n) - np.repeat(np.cumsum(lay.glens) - lay.glens, lay.glens)).all()


def test_build_narrow_and_hash_predictions():
    rng = np.random.RandomState(9)
    lens = rng.choice([1, 2, 3, 9, 40], size=300)
    lay = sl.build(lens, rng.permutation(300).astype(np.int64) * 7, rng, "narrow")
    _check_prediction(lay, lay.k.view(np.uint64))
    assert (lay.run_lens[lay.row_run] == np.bincount(lay.row_run)[lay.row_run]).all()
    keys = sl.draw_wide_keys(300, rng)
    lay = sl.build(lens, keys, rng, "hash")
    _check_prediction(lay, sl.h32(lay.k))
    with pytest.raises(AssertionError):      # narrow keys are no hash layout
        sl.build(lens, np.arange(300), rng, "hash")
    with pytest.raises(AssertionError):      # wide keys are no narrow layout
        sl.build(lens, keys, rng, "narrow")


def test_build_rejects_h32_collisions():
    # two keys of equal h32: found by search over a small range
    cand = np.arange(1 << 40, (1 << 40) + 400_000, dtype=np.int64)
    hh = sl.h32(cand)
    o = np.argsort(hh, kind="stable")
    dup = np.flatnonzero(hh[o][1:] == hh[o][:-1])
    assert len(dup), "expected a 32-bit collision among 400k keys"
    a, b = cand[o[dup[0]]], cand[o[dup[0] + 1]]
    bad = np.concatenate([[a, b], sl.draw_wide_keys(50, np.random.RandomState(1))])
    with pytest.raises(AssertionError, match="h32 collision"):
        sl.build([2] * 52, bad, np.random.RandomState(0), "hash")
    drawn = sl.draw_wide_keys(2000, np.random.RandomState(0), h32_below=1 << 28)
    assert len(np.unique(sl.h32(drawn))) == 2000 and (sl.h32(drawn) < (1 << 28)).all()
    assert (drawn >= (1 << 40)).all() and (drawn < (1 << 62)).all()


# ---------------- the fixed inputs of the GPU tests ----------------

def _all_conditions(cov, n_mod):
    for key in sl.COVERAGE_KEYS:
        assert cov[key] > 0, key
    assert cov["n_mod_chunk"] == n_mod


@pytest.mark.parametrize("tail", [0, 3])
def test_soa_input_reaches_every_path(tail):
    lay = sl.soa_layout(tail)
    assert lay.n <= 21_000 and lay.n % 8 == tail
    assert lay.keys.max() < (1 << 16) and len(sl.active_bytes(lay.k)) == 2
    _check_prediction(lay, lay.k.view(np.uint64))
    _all_conditions(sl.coverage(lay.glens), tail)
    # the hand-placed runs sit where the comments in soa_run_lens say
    e = np.cumsum(lay.glens)
    s = e - lay.glens
    at = {int(a): int(b) for a, b in zip(s, lay.glens)}
    slot = {int(a): i for i, a in enumerate(s)}
    m = sl.SOA_MARKS
    for row in range(m["fast_even"], m["fast_even"] + 9):
        assert row in at                                  # 8 heads + the next
    assert slot[m["fast_even"]] % 2 == 0
    assert at[m["one_chunk_run"]] == 8 and m["one_chunk_run"] % 8 == 0
    for row in range(m["fast_odd"], m["fast_odd"] + 9):
        assert row in at
    assert slot[m["fast_odd"]] % 2 == 1
    d = m["distinct_continues"]
    assert all(r in at for r in range(d, d + 8)) and d + 8 not in at
    assert at[m["one_wave_run"]] == 512 and m["one_wave_run"] % 512 == 0
    assert at[m["tile_last_row_len1"]] == 1        # starts and ends at row 4095
    assert m["tile_last_row_len1"] == 4095 and 4090 in at and at[4090] == 5
    assert at[4096] == 4096                        # exactly tile 1; ends at 8191
    assert 8192 in at                              # a run starts at a tile start
    h = m["headless_tile_run"]                     # no head in tile 3 at all
    assert h < 3 * 4096 and h + at[h] > 4 * 4096
    assert not any(3 * 4096 <= r < 4 * 4096 for r in at)
    t = m["tile_last_row_cross"]
    assert t % 4096 == 4095 and at[t] > 1
    f = m["fast_at_end"]
    assert all(r in at for r in range(f, f + 8))
    assert (f + 8 == lay.n) if tail == 0 else (f + 8 in at and lay.n - (f + 8) == 3)


@pytest.mark.parametrize("with_minus1", [True, False])
def test_hash_input_reaches_every_path(with_minus1):
    lay = sl.hash_layout(with_minus1)
    assert lay.n == 155_365 and len(lay.run_lens) == 3691
    assert len(sl.active_bytes(lay.k)) == 8          # > 5: the hash strategy
    assert len(np.unique(sl.h32(lay.keys))) == len(lay.keys)
    _check_prediction(lay, sl.h32(lay.k))
    _all_conditions(sl.coverage(lay.glens), 5)
    assert int(sl.h32([-1])[0]) == sl.H32_MINUS1
    if with_minus1:
        # the last grouped run is key -1; it fills the guarded tail chunk
        # (5 rows) and reaches back into the chunk before it
        assert lay.keys[lay.order[-1]] == -1 and lay.glens[-1] == 9
        assert (np.sort(lay.gpos[lay.k == -1]) == np.arange(lay.n - 9, lay.n)).all()
        assert (sl.h32(lay.keys[lay.order[:-1]]) < sl.H32_MINUS1).all()
    else:
        assert (lay.keys != -1).all()


def _layouts():
    return [sl.soa_layout(0), sl.soa_layout(3), sl.hash_layout(True), sl.hash_layout(False)]


def test_minmax_values_place_the_extrema():
    for lay in _layouts():
        v = sl.values_minmax(lay, np.random.RandomState(1))
        cls = sl.minmax_classes(lay)
        assert set(cls.tolist()) == set(range(9))
        grouped = np.empty(lay.n, dtype=np.int64)
        grouped[lay.gpos] = v                      # values in grouped order
        e = np.cumsum(lay.glens)
        s = e - lay.glens
        gcls = cls[lay.order]
        first, last = grouped[s], grouped[e - 1]
        multi = lay.glens > 1
        assert (first[gcls == sl.CL_MIN_FIRST] == sl.I64_MIN).all()
        assert (first[gcls == sl.CL_MAX_FIRST] == sl.I64_MAX).all()
        assert (last[gcls == sl.CL_MIN_LAST] == sl.I64_MIN).all()
        assert (last[gcls == sl.CL_MAX_LAST] == sl.I64_MAX).all()
        for c in (sl.CL_MIN_FIRST, sl.CL_MAX_FIRST, sl.CL_MIN_LAST, sl.CL_MAX_LAST):
            assert (multi & (gcls == c)).sum() > 0     # on runs longer than a row
        # an extremum in another chunk, wave and tile than the run's first row
        for c, ext in ((sl.CL_MIN_LATER_CHUNK, sl.I64_MIN), (sl.CL_MAX_LATER_CHUNK, sl.I64_MAX)):
            far_chunk = far_tile = 0
            for i in np.flatnonzero(gcls == c):
                hit = np.flatnonzero(grouped[s[i]:e[i]] == ext) + s[i]
                if len(hit):
                    assert len(hit) == 1
                    far_chunk += hit[0] // 8 != s[i] // 8
                    far_tile += hit[0] // 4096 != s[i] // 4096
            assert far_chunk > 0 and far_tile > 0
        for c, ext in ((sl.CL_ALL_MAX, sl.I64_MAX), (sl.CL_ALL_MIN, sl.I64_MIN)):
            idx = np.flatnonzero(gcls == c)
            assert (lay.glens[idx] > 8).sum() > 0      # not only one-row runs
            for i in idx:
                assert (grouped[s[i]:e[i]] == ext).all()
        # both identities also come out as RESULTS of the other op
        _, mn = sl.reduce_ref(sl.OP_MIN_I64, lay.k, v)
        _, mx = sl.reduce_ref(sl.OP_MAX_I64, lay.k, v)
        assert (mn == sl.I64_MAX).any() and (mn == sl.I64_MIN).any()
        assert (mx == sl.I64_MAX).any() and (mx == sl.I64_MIN).any()


def test_sum_values_wrap_and_f64_values_meet_their_premises():
    for lay in _layouts():
        v = sl.values_sum_i64(lay, np.random.RandomState(2))
        _, exact = sl.exact_int_sums(lay.k, v)
        wraps = sum(not (-(1 << 63) <= x < (1 << 63)) for x in exact)
        assert wraps >= 10
        f = sl.values_f64_integral(lay, np.random.RandomState(3))
        assert (f == np.rint(f)).all()
        _, fs, sabs, _ = sl.sum_f64_ref(lay.k, f)
        assert sabs.max() < 2.0 ** 53
        g = sl.values_f64_mixed(lay, np.random.RandomState(4))
        assert (g > 0).any() and (g < 0).any()
        assert np.abs(g).max() / np.abs(g[g != 0]).min() > 1e8
