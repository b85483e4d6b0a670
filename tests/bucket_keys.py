"""Keys with chosen hashes, and inputs whose hash order has chosen buckets.

The hash route of the grouping sort orders rows by h32 = low 32 bits of
vega_hash_u64(key). After its three passes over hash bytes 1..3 the rows lie
in BUCKETS (equal bits 8..31 of h32), and the bucket finish kernel orders each
bucket by hash byte 0 inside a tile of FT rows plus slack. vega_hash_u64 is
the splitmix64 finalizer, a bijection of 64-bit words, so a test can ask for
any hash: keys_for_hashes() inverts it. Pure numpy; checked in
test_bucket_keys.py.

A layout is a list of bucket lengths in bucket order, so a bucket's position
in the hash-ordered array (and against the tile edges) is a running sum.
"""
import numpy as np

FT = 2048           # k_bucket_finish: rows per tile (FIN_FT)
BUCKET_CAP = 256    # rows per bucket, and slack rows staged either side
RUN_CAP = 64        # longest equal-h32 run the cleanup rule sorts
NSAMPLE = 2048      # rows k_sample_keys reads

GOLDEN = np.uint64(0x9E3779B97F4A7C15)
INV_M1 = np.uint64(0x96DE1B173F119089)   # inverse of 0xBF58476D1CE4E5B9 mod 2^64
INV_M2 = np.uint64(0x319642B2D24D8EC3)   # inverse of 0x94D049BB133111EB mod 2^64

CYCLE = (1, 2, 3, 5, 63, 64, 65, 127, 255, 256)
# equal-h32 runs by key, in input order; letters are distinct keys
SHAPES = ("AB", "AA", "ABA", "AAB", "ABC", "BABA")


def hash_u64(keys):
    """vega_hash_u64 (vega_common.h) of int64 keys, as uint64"""
    x = np.asarray(keys, dtype=np.int64).view(np.uint64).copy()
    with np.errstate(over="ignore"):
        x += GOLDEN
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        x ^= x >> np.uint64(31)
    return x


def draw_hi32(rng, count):
    """`count` distinct 32-bit values"""
    while True:
        hi = rng.randint(0, 1 << 32, size=count, dtype=np.uint64)
        if len(np.unique(hi)) == count:
            return hi


def keys_for_hashes(h64):
    """int64 keys k with vega_hash_u64(k) == h64"""
    x = np.array(h64, dtype=np.uint64, copy=True)
    with np.errstate(over="ignore"):
        x ^= (x >> np.uint64(31)) ^ (x >> np.uint64(62))
        x *= INV_M2
        x ^= (x >> np.uint64(27)) ^ (x >> np.uint64(54))
        x *= INV_M1
        x ^= (x >> np.uint64(30)) ^ (x >> np.uint64(60))
        x -= GOLDEN
    return x.view(np.int64)


def make_h64(bucket, byte0, hi32):
    return ((np.asarray(hi32, dtype=np.uint64) << np.uint64(32))
            | (np.asarray(bucket, dtype=np.uint64) << np.uint64(8))
            | np.asarray(byte0, dtype=np.uint64))


def bucket_of(keys):
    return ((hash_u64(keys) >> np.uint64(8)) & np.uint64(0xFFFFFF)).astype(np.int64)


def sampled_positions(n):
    ns = min(n, NSAMPLE)
    return np.arange(ns, dtype=np.int64) * (n // ns)


def fill_lengths(lens, upto, cyc):
    """append bucket lengths from the cycle until they sum to `upto` exactly"""
    pos = sum(lens)
    assert pos <= upto
    while pos < upto:
        length = min(CYCLE[cyc[0] % len(CYCLE)], upto - pos)
        cyc[0] += 1
        lens.append(length)
        pos += length
    return lens


def lengths_with(n, fixed):
    """bucket lengths summing to n, cycling through CYCLE, with a bucket of
    length L starting at row s for every (s, L) in `fixed` (ascending s)"""
    lens, cyc = [], [0]
    for s, length in fixed:
        fill_lengths(lens, s, cyc)
        lens.append(length)
    return fill_lengths(lens, n, cyc)


def bucket_starts(lens):
    return np.concatenate([[0], np.cumsum(lens)])[:-1].astype(np.int64)


class Layout:
    """an input (k, v = row index) and what its hash order looks like"""

    def __init__(self, k, lens, runs):
        self.k = k
        self.v = np.arange(len(k), dtype=np.int64)
        self.n = len(k)
        self.lens = list(lens)
        self.runs = runs      # [(bucket index, shape)] planted equal-h32 runs


def place(free, held, rng):
    """input order: the rows of each `held` group keep their order and stay off
    the sampled positions; `free` rows (distinct keys) go anywhere"""
    n = len(free) + sum(len(g) for g in held)
    out = np.empty(n, dtype=np.uint64)
    taken = np.zeros(n, dtype=bool)
    nheld = n - len(free)
    if nheld:
        off = np.setdiff1d(np.arange(n, dtype=np.int64), sampled_positions(n))
        assert nheld <= len(off), "not enough unsampled rows"
        slots = np.sort(rng.choice(off, size=nheld, replace=False))
        label = rng.permutation(np.repeat(np.arange(len(held)), [len(g) for g in held]))
        for gi, g in enumerate(held):
            out[slots[label == gi]] = g
        taken[slots] = True
    out[~taken] = rng.permutation(np.asarray(free, dtype=np.uint64))
    return out


def build(lens, rng, plant=True, minus1=False, dirty65=None):
    """Layout whose hash order has buckets of `lens` rows, in that order.

    plant: equal-h32 runs of SHAPES, cycling, in every bucket long enough.
    minus1: key -1 is one of the rows (its bucket takes the slot that keeps
    the bucket ids ascending).
    dirty65: index of a bucket that gets an equal-h32 run of 65 rows cycling
    through three keys (too long for the cleanup rule to sort)."""
    nb = len(lens)
    ids = set()
    h_m1 = int(hash_u64(np.array([-1]))[0])
    if minus1:
        ids.add((h_m1 >> 8) & 0xFFFFFF)
    while len(ids) < nb:
        ids.update(rng.randint(0, 1 << 24, size=nb - len(ids)).tolist())
    ids = np.sort(np.fromiter(ids, dtype=np.int64))
    free, held, runs = [], [], []
    shape_i = 0
    for bi, (b, length) in enumerate(zip(ids.tolist(), lens)):
        has_m1 = minus1 and b == ((h_m1 >> 8) & 0xFFFFFF)
        rows_left = length
        used = set()          # byte-0 values taken by planted runs / key -1
        if has_m1:
            free.append(np.array([h_m1], dtype=np.uint64))
            used.add(h_m1 & 0xFF)
            rows_left -= 1
        if dirty65 == bi:
            assert rows_left >= 65
            c = next(x for x in range(256) if x not in used)
            used.add(c)
            hi = draw_hi32(rng, 3)
            held.append(make_h64(b, c, hi[np.arange(65) % 3]))
            runs.append((bi, "ABC" * 21 + "AB"))
            rows_left -= 65
        elif plant and not has_m1:
            while rows_left >= 5 and len(used) < 3:
                shape = SHAPES[shape_i % len(SHAPES)]
                shape_i += 1
                c = next(x for x in range(int(rng.randint(0, 200)), 256) if x not in used)
                used.add(c)
                hi = draw_hi32(rng, 3)
                held.append(make_h64(b, c, hi[[ord(ch) - ord("A") for ch in shape]]))
                runs.append((bi, shape))
                rows_left -= len(shape)
        if rows_left:
            byte0 = rng.choice(np.setdiff1d(np.arange(256), sorted(used)), size=rows_left)
            hi = draw_hi32(rng, rows_left)
            free.append(make_h64(b, byte0, hi))
    free = np.concatenate(free) if free else np.empty(0, dtype=np.uint64)
    assert len(np.unique(free)) == len(free)
    return Layout(keys_for_hashes(place(free, held, rng)), lens, runs)


def crafted():
    """test 1: n = 3 FT + 37; every tile-edge case, planted runs, key -1"""
    n = 3 * FT + 37
    fixed = [(FT - 1, 1),            # 1-row bucket on a tile's last row, ends on the edge
             (FT, 127),              # starts on a tile edge
             (2 * FT - 1, 65),       # one row left of the edge
             (3 * FT + 1 - 255, 255)]  # one row right of the edge
    lens = lengths_with(n, fixed)
    return build(lens, np.random.RandomState(101), minus1=True)


def oversized():
    """test 2: a 257-row bucket inside a tile and one across a tile edge"""
    n = 2 * FT + 300
    lens = lengths_with(n, [(500, 257), (2 * FT - 100, 257)])
    return build(lens, np.random.RandomState(102))


def dirty_run():
    """test 3: one bucket holds a 65-row equal-h32 run over three keys"""
    n = 2 * FT + 100
    lens = lengths_with(n, [(700, 100)])
    at = int(np.flatnonzero(bucket_starts(lens) == 700)[0])
    return build(lens, np.random.RandomState(103), plant=False, dirty65=at)


def distinct(n, seed):
    """test 6: n distinct keys, buckets as the cycle gives them"""
    return build(lengths_with(n, []), np.random.RandomState(seed), plant=False)


def poisson(n=300_000, nbuckets=5000, seed=104):
    """test 4: n distinct keys, bucket drawn from nbuckets values (about
    Poisson(n / nbuckets) rows each), byte 0 and the high bits random"""
    rng = np.random.RandomState(seed)
    ids = np.unique(rng.randint(0, 1 << 24, size=2 * nbuckets))[:nbuckets]
    assert len(ids) == nbuckets
    h = make_h64(ids[rng.randint(0, nbuckets, size=n)], rng.randint(0, 256, size=n),
                 rng.randint(0, 1 << 32, size=n, dtype=np.uint64))
    assert len(np.unique(h)) == n
    k = keys_for_hashes(h)
    lens = np.unique(bucket_of(k), return_counts=True)[1]
    return Layout(k, lens.tolist(), [])


def with_sampled_repeat(lay):
    """test 5: the same input with one key copied to two sampled positions"""
    k = lay.k.copy()
    sp = sampled_positions(lay.n)
    k[sp[1000]] = k[sp[10]]
    return Layout(k, [], [])
