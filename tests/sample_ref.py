"""numpy restatement of the sampling definition (DESIGN.md "Sampling";
include/vega_common.h): sample / random_split / take_sample as pure functions
of (seed, global row index). Written from the definition, not from the
kernels; every keep/drop decision compares a 53-bit integer draw with an
integer threshold.

  d_i   = rand_u64(hash_u64(seed), i) >> 11
  T(p)  = min(uint64(p * 2^53), 2^53), 0 for p <= 0
  Bernoulli: keep i iff d_i < T(fraction)
  Poisson:   c_i = #{ c < L : d_i >= T(cdf_c) }
  split:     cell_i = #{ 1 <= j < W : d_i >= T(b_j) },  B_W = 2^53
  take_sample: candidates = sample(.., seed + attempt); shuffled by the
               priority rand_u64(hash_u64(~seed), j), stable ascending
"""
import math

import numpy as np

from vega_amd.shuffle import hash_u64_np

ONE = 1 << 53
MASK64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15
TABLE_MAX = 256
LAMBDA_MAX = 16.0


def hash_u64(x):
    """scalar splitmix64 finalizer (vega_hash_u64)"""
    x = (x + GOLDEN) & MASK64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & MASK64
    return x ^ (x >> 31)


def rand_u64_np(seed, idx):
    """vega_rand_u64(seed, j) for an array of counters j"""
    j = np.asarray(idx, dtype=np.uint64)
    with np.errstate(over="ignore"):
        x = np.uint64(seed & MASK64) ^ (np.uint64(GOLDEN) * (j + np.uint64(1)))
    return hash_u64_np(x.view(np.int64))


def draw53(seed, idx):
    """d_i for the global row indices idx (uint64 array of 53-bit draws)"""
    return rand_u64_np(hash_u64(seed & MASK64), idx) >> np.uint64(11)


def thresholds(p):
    """T(p) as a Python int"""
    if not p > 0.0:
        return 0
    x = p * 9007199254740992.0
    return ONE if x >= 9007199254740992.0 else int(x)


def poisson_table(lam):
    """[T(cdf_0), ..., T(cdf_{L-1})] as a uint64 array"""
    if not lam >= 0.0:
        raise ValueError("fraction must be >= 0")
    if lam > LAMBDA_MAX:
        raise NotImplementedError("fraction > 16")
    p = math.exp(-lam)
    cdf = p
    c = 0
    thr = []
    while True:
        if (c > lam and p < 2.0 ** -54) or c == TABLE_MAX - 1:
            break
        thr.append(thresholds(cdf))
        c += 1
        p = p * lam / c
        cdf = cdf + p
    return np.array(thr, dtype=np.uint64)


def poisson_counts(d, table):
    """c_i = #{ c < L : d_i >= T_c } for draws d"""
    table = np.asarray(table, dtype=np.uint64)
    # table ascending: the number of entries <= d
    return np.searchsorted(table, d, side="right").astype(np.int64)


def sample_counts(n, with_replacement, fraction, seed, start=0, table=None):
    """copies of each of the rows start .. start+n-1 (int64 array)"""
    d = draw53(seed, np.arange(start, start + n, dtype=np.uint64))
    if not with_replacement:
        if not (-1e-6 <= fraction <= 1.0 + 1e-6):
            raise ValueError("fraction out of [0, 1]")
        t = thresholds(min(fraction, 1.0))
        return (d < np.uint64(t)).astype(np.int64)
    if table is None:
        table = poisson_table(fraction)
    return poisson_counts(d, table)


def sample_ref(keys, vals, with_replacement, fraction, seed, start=0, table=None):
    """the sampled (keys, vals): row order kept, Poisson copies adjacent"""
    keys = np.asarray(keys)
    vals = np.asarray(vals)
    c = sample_counts(len(keys), with_replacement, fraction, seed, start, table)
    idx = np.repeat(np.arange(len(keys)), c)
    return keys[idx], vals[idx]


def split_bounds(weights):
    """[B_0 = 0, B_1, ..., B_W = 2^53] as Python ints"""
    w = [float(x) for x in weights]
    if len(w) == 0 or len(w) > 256:
        raise ValueError("1..256 weights")
    if any(not x >= 0.0 for x in w):
        raise ValueError("weights must be nonnegative")
    s = 0.0
    for x in w:
        s += x
    if not s > 0.0 or math.isinf(s):
        raise ValueError("sum of weights must be positive")
    b = [0]
    run = 0.0
    for j in range(1, len(w)):
        run = run + w[j - 1] / s
        b.append(thresholds(run))
    b.append(ONE)
    return b


def split_cells(n, weights, seed, start=0):
    b = split_bounds(weights)
    d = draw53(seed, np.arange(start, start + n, dtype=np.uint64))
    cell = np.zeros(n, dtype=np.int64)
    for j in range(1, len(weights)):
        cell += (d >= np.uint64(b[j])).astype(np.int64)
    return cell


def random_split_ref(keys, vals, weights, seed):
    """list of (keys, vals) per split, each in row order"""
    keys = np.asarray(keys)
    vals = np.asarray(vals)
    cell = split_cells(len(keys), weights, seed)
    return [(keys[cell == j], vals[cell == j]) for j in range(len(weights))]


def fraction_for_sample_size(num, total, with_replacement):
    """utils/random.rs:318-358 compute_fraction_for_sample_size"""
    if with_replacement:
        s = float(num)
        k = 12.0 if s < 6.0 else (9.0 if s < 16.0 else 6.0)
        return max(s + k * math.sqrt(s), 1e-10) / float(total)
    f = float(num) / float(total)
    gamma = -math.log(1e-4) / float(total)
    return min(1.0, max(1e-10, f + gamma + math.sqrt(gamma * gamma + 2.0 * gamma * f)))


def take_sample_ref(keys, vals, with_replacement, num, seed, fraction=None, info=None):
    """(keys, vals) of take_sample. `fraction` overrides the computed
    oversampling fraction (to exercise the re-sample loop); `info`, a dict,
    receives attempts / candidates."""
    keys = np.asarray(keys)
    vals = np.asarray(vals)
    n = len(keys)
    if num == 0 or n == 0:
        return keys[:0], vals[:0]
    if not with_replacement and num >= n:
        ck, cv = keys, vals
        attempts = 0
    else:
        if fraction is None:
            fraction = fraction_for_sample_size(num, n, with_replacement)
        for attempt in range(100):
            ck, cv = sample_ref(keys, vals, with_replacement, fraction,
                                (seed + attempt) & MASK64)
            if len(ck) >= num:
                break
        else:
            raise NotImplementedError("repeated sampling 100 times; aborting")
        attempts = attempt + 1
    if info is not None:
        info["attempts"] = attempts
        info["candidates"] = len(ck)
    prio = rand_u64_np(hash_u64(~seed & MASK64), np.arange(len(ck), dtype=np.uint64))
    order = np.argsort(prio, kind="stable")[:min(num, len(ck))]
    return ck[order], cv[order]
