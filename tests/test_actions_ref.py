"""actions_ref (the pure-Python restatement of the action semantics) is
pinned to the reference's own test expectations (tests/golden/actions.json)
and to the fold / wrapping rules the engine documents. CPU only."""
import json
import os

import numpy as np
import pytest

import actions_ref as ar

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "actions.json")) as _f:
    ENTRIES = json.load(_f)["entries"]


def elements(g):
    if "range" in g:
        k = np.arange(g["range"][0], g["range"][1], dtype=np.int64)
    else:
        k = np.asarray(g["elements"], dtype=np.int64)
    return k, np.zeros(len(k), dtype=np.int64)  # element -> key column, value 0


def test_fixture_shape():
    ops = {g["op"] for g in ENTRIES}
    assert ops == {"fold", "max", "min", "top", "take_ordered", "take", "first", "is_empty"}
    for g in ENTRIES:
        assert g["source"].startswith("reference tests/test_rdd.rs:")
        assert g["mapping"] == "element -> key column, value 0"


@pytest.mark.parametrize("g", ENTRIES, ids=lambda g: g["op"])
def test_ref_reproduces_golden(g):
    k, v = elements(g)
    op = g["op"]
    if op == "fold":
        assert g["fold_op"] == "SUM_I64"
        fk, fv = ar.fold(k, v, ar.OP_SUM_I64, g["init"], 0, g["nparts"])
        assert (fk, fv) == (g["expected"], 0)
    elif op == "max":
        assert ar.lex_max(k, v) == (g["expected"], 0)
    elif op == "min":
        assert ar.lex_min(k, v) == (g["expected"], 0)
    elif op == "top":
        tk, tv = ar.top(k, v, g["num"])
        assert tk.tolist() == g["expected"] and not tv.any()
    elif op == "take_ordered":
        tk, tv = ar.take_ordered(k, v, g["num"])
        assert tk.tolist() == g["expected"] and not tv.any()
    elif op == "take":
        tk, tv = ar.take(k, v, g["num"])
        assert len(tk) == len(tv) == g["expected_len"]
        assert tk.tolist() == k[:g["expected_len"]].tolist()
    elif op == "first":
        if g["expected_ok"]:
            assert ar.first(k, v) == (int(k[0]), 0)
        else:
            with pytest.raises(ValueError, match="empty collection"):
                ar.first(k, v)
    elif op == "is_empty":
        assert ar.is_empty(k) is g["expected"]
    else:
        raise AssertionError(op)


def test_fold_nonzero_init_counts_every_partition():
    k = np.arange(-1000, 1000, dtype=np.int64)
    v = np.arange(2000, dtype=np.int64)
    rk, rv = ar.reduce(k, v, ar.OP_SUM_I64)
    # init = 5, P = 10: 11 inits -> reduce + 55, in both columns
    assert ar.fold(k, v, ar.OP_SUM_I64, 5, 5, 10) == (rk + 55, rv + 55)
    # empty rdd: (P+1) * init, empty partitions still count
    e = np.zeros(0, dtype=np.int64)
    assert ar.fold(e, e, ar.OP_SUM_I64, 5, -2, 10) == (55, -22)
    assert ar.fold(e, e, ar.OP_SUM_I64, 5, -2, 4) == (25, -10)
    # MIN / MAX: op(init, reduce), idempotent in the number of inits
    assert ar.fold(k, v, ar.OP_MIN_I64, 5, 5, 10) == (-1000, 0)
    assert ar.fold(k, v, ar.OP_MAX_I64, 5, 5000, 10) == (999, 5000)
    assert ar.fold(e, e, ar.OP_MAX_I64, 5, 7, 3) == (5, 7)
    # f64 value column, key column still wrapping i64
    fk, fv = ar.fold(k[:4], np.array([0.5, 0.25, 1.0, 2.0]), ar.OP_SUM_F64, 1, 0.5, 1)
    assert (fk, fv) == (int(k[:4].sum()) + 2, 3.75 + 1.0)


def test_wrapping_sums_near_the_i64_edges():
    big = (1 << 63) - 1
    k = np.array([big, 1], dtype=np.int64)            # MAX + 1 wraps to MIN
    v = np.array([-big - 1, -1], dtype=np.int64)      # MIN - 1 wraps to MAX
    assert ar.reduce(k, v, ar.OP_SUM_I64) == (-big - 1, big)
    assert ar.wrap_i64(1 << 63) == -(1 << 63)
    assert ar.wrap_i64(-(1 << 63) - 1) == big
    # agrees with numpy's two's-complement accumulation on a long column
    rng = np.random.default_rng(7)
    a = rng.integers(-(1 << 62), 1 << 62, size=10_001, dtype=np.int64) * 2
    with np.errstate(over="ignore"):
        assert ar.reduce(a, a[::-1], ar.OP_SUM_I64) == (int(a.sum()), int(a[::-1].sum()))
    # fold's init arithmetic wraps too
    e = np.zeros(0, dtype=np.int64)
    assert ar.fold(e, e, ar.OP_SUM_I64, big, 1 << 62, 1) == (-2, -(1 << 63))
    # key column wraps under SUM_F64 as well
    assert ar.reduce(k, np.array([0.5, 0.5]), ar.OP_SUM_F64) == (-big - 1, 1.0)


def test_lexicographic_order_is_key_then_value_signed():
    k = np.array([3, -1, 3, -1, 3], dtype=np.int64)
    v = np.array([0, 9, -5, -9, 7], dtype=np.int64)
    assert ar.lex_min(k, v) == (-1, -9)
    assert ar.lex_max(k, v) == (3, 7)
    tk, tv = ar.take_ordered(k, v, 3)
    assert list(zip(tk.tolist(), tv.tolist())) == [(-1, -9), (-1, 9), (3, -5)]
    tk, tv = ar.top(k, v, 9)
    assert list(zip(tk.tolist(), tv.tolist())) == [(3, 7), (3, 0), (3, -5), (-1, 9), (-1, -9)]
    assert ar.lex_min(k[:0], v[:0]) is None and ar.reduce(k[:0], v[:0], ar.OP_MIN_I64) is None
