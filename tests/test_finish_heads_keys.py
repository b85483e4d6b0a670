"""tests/finish_heads_keys.py builds what it says: the final order it predicts
is the stable order by h32, and the planted runs sit on the edges named in the
GPU test (tests/test_gpu_finish_heads.py). No GPU needed."""
import numpy as np
import pytest

import bucket_keys as bk
import finish_heads_keys as fh

FT = fh.FT


@pytest.fixture(scope="module", params=fh.SIZES)
def lay(request):
    return fh.build(request.param, seed=request.param)


def test_sizes_cover_odd_and_even_tile_counts_off_the_chunk():
    tiles = [(n + FT - 1) // FT for n in fh.SIZES]
    assert sorted(t % 2 for t in tiles) == [0, 1]
    assert all(n % fh.CHUNK != 0 for n in fh.SIZES)


def test_final_order_is_the_stable_h32_order(lay):
    h32 = (bk.hash_u64(lay.k) & np.uint64(0xFFFFFFFF)).astype(np.int64)
    assert (lay.k[np.argsort(h32, kind="stable")] == lay.final_k).all()
    # distinct h32 per distinct key: the cleanup rule has nothing to regroup
    assert len(np.unique(h32)) == len(np.unique(lay.k)) == len(lay.run_lens)
    assert -1 in lay.k


def test_route_conditions(lay):
    # no repeated key on the sampled rows, buckets within the finish caps
    samp = lay.k[bk.sampled_positions(lay.n)]
    assert len(np.unique(samp)) == len(samp)
    b = bk.bucket_of(lay.final_k)
    starts = np.flatnonzero(np.concatenate([[True], b[1:] != b[:-1]]))
    assert (starts == lay.bucket_start).all()
    assert np.diff(np.concatenate([starts, [lay.n]])).max() <= bk.BUCKET_CAP
    assert lay.n / len(starts) >= 24      # FIN_MIN_BUCKET_ROWS


def test_planted_runs_sit_on_the_edges(lay):
    s, ln = lay.run_start, lay.run_lens
    e = s + ln                                     # one past the run's last row
    head = set(s.tolist())
    bstart = set(lay.bucket_start.tolist())

    def crossing(edge):
        return ((s < edge) & (e > edge)).any()
    # ~40-row runs over the finish-tile edge at 2048 and over 4096 (seg-tile edge too)
    assert ((s < FT) & (e > FT) & (ln == 40)).any()
    assert ((s < 2 * FT) & (e > 2 * FT) & (ln == 40)).any() and 2 * FT % fh.SEG_TILE == 0
    # a head on the last row of a finish tile
    assert any((x + 1) % FT == 0 for x in head)
    # a head on a tile's first row where a bucket starts too (p == lo), not row 0
    assert any(x % FT == 0 and x in bstart for x in head if x > 0)
    # a tile whose first row continues a run, in a bucket that began before the tile
    for edge in (FT, 2 * FT):
        assert crossing(edge) and edge not in head and edge not in bstart
    # 2-row and 9-row runs over an 8-row chunk edge
    for want in (2, 9):
        assert ((ln == want) & (s // fh.CHUNK != (e - 1) // fh.CHUNK)).any()


def test_distinct_variant_has_no_runs():
    lay = fh.build(fh.SIZES[0], seed=5, runs=False)
    assert len(np.unique(lay.k)) == lay.n and (lay.run_lens == 1).all()
