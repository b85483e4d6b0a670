"""Pure-Python/numpy restatement of the device-side action semantics
(rdd.rs:274-322 reduce/fold, :534-620 first/take, :1073-1153 is_empty /
min / max / top / take_ordered) over (i64 key, i64|f64 value) rows.

Independent of the engine: the checker for tests/test_gpu_actions.py and
tests/test_gpu_select.py. Ops use the vega_op_t numbering."""
import math

import numpy as np

OP_SUM_I64 = 0
OP_SUM_F64 = 2
OP_MIN_I64 = 3
OP_MAX_I64 = 4

_M64 = (1 << 64) - 1


def wrap_i64(x):
    """two's-complement wrap of a Python int to i64 (Rust wrapping_add)"""
    x &= _M64
    return x - (1 << 64) if x >> 63 else x


def _wsum(a):
    return wrap_i64(sum(int(x) for x in np.asarray(a, dtype=np.int64).tolist()))


def reduce(keys, vals, op):
    """column-wise |(k1,v1),(k2,v2)| (k1 op k2, v1 op v2); None on empty.
    The key column is always i64 (SUM wraps, also under SUM_F64)."""
    keys = np.asarray(keys, dtype=np.int64)
    if len(keys) == 0:
        return None
    if op == OP_SUM_I64:
        return _wsum(keys), _wsum(vals)
    if op == OP_SUM_F64:
        return _wsum(keys), math.fsum(np.asarray(vals, dtype=np.float64).tolist())
    vals = np.asarray(vals, dtype=np.int64)
    if op == OP_MIN_I64:
        return int(keys.min()), int(vals.min())
    if op == OP_MAX_I64:
        return int(keys.max()), int(vals.max())
    raise ValueError(op)


def _comb(op, a, b, f64=False):
    if op in (OP_SUM_I64, OP_SUM_F64):
        return a + b if f64 else wrap_i64(a + b)
    return min(a, b) if op == OP_MIN_I64 else max(a, b)


def fold(keys, vals, op, init_k, init_v, nparts):
    """rdd.rs:311-322: init seeds each of the nparts partition folds and the
    fold across them, so it is combined nparts+1 times (empty partitions
    count); an empty rdd folds to init combined nparts+1 times."""
    red = reduce(keys, vals, op)
    acc_k, acc_v = (None, None) if red is None else red
    f64 = op == OP_SUM_F64
    for _ in range(nparts + 1):
        acc_k = init_k if acc_k is None else _comb(op, acc_k, init_k)
        acc_v = init_v if acc_v is None else _comb(op, acc_v, init_v, f64)
    return acc_k, acc_v


def _lex_order(keys, vals):
    keys = np.asarray(keys, dtype=np.int64)
    vals = np.asarray(vals, dtype=np.int64)
    return keys, vals, np.lexsort((vals, keys))  # primary key, then value


def lex_min(keys, vals):
    keys, vals, o = _lex_order(keys, vals)
    return None if len(o) == 0 else (int(keys[o[0]]), int(vals[o[0]]))


def lex_max(keys, vals):
    keys, vals, o = _lex_order(keys, vals)
    return None if len(o) == 0 else (int(keys[o[-1]]), int(vals[o[-1]]))


def take(keys, vals, num):
    """first min(num, n) rows in partition order = the row prefix"""
    keys = np.asarray(keys, dtype=np.int64)
    vals = np.asarray(vals)
    m = min(int(num), len(keys))
    return keys[:m], vals[:m]


def first(keys, vals):
    if len(keys) == 0:
        raise ValueError("empty collection")
    return int(keys[0]), np.asarray(vals)[0].item()


def is_empty(keys):
    return len(keys) == 0


def take_ordered(keys, vals, num):
    keys, vals, o = _lex_order(keys, vals)
    o = o[:min(int(num), len(o))]
    return keys[o], vals[o]


def top(keys, vals, num):
    keys, vals, o = _lex_order(keys, vals)
    o = o[::-1][:min(int(num), len(o))]
    return keys[o], vals[o]
