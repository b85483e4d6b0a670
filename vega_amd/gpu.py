"""ctypes bindings for libvega_gpu.so (the C-ABI in include/vega_gpu.h).

Two layers, mirroring the ABI:
  - VegaContext: the RDD-handle API (single process, one GPU) — the drop-in
    surface a Rust host would bind.
  - dev_*: device-pointer entries for the rank-per-GPU path; they take torch
    CUDA tensors (device memory + stream plumbing only — all compute is in
    the hand-written HIP kernels).

This module FAILS LOUDLY if the HIP library is missing — no CPU fallback.
"""
import ctypes
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIBPATH = os.path.join(HERE, "csrc", "libvega_gpu.so")
LIBPATH_TORCH = os.path.join(HERE, "csrc", "libvega_gpu_torch.so")

OP_SUM_I64 = 0
OP_COUNT = 1
OP_SUM_F64 = 2
OP_MIN_I64 = 3
OP_MAX_I64 = 4
OP_MIN_F64 = 5  # f64 min / max: order of f64_order_key, NaN skipped
OP_MAX_F64 = 6
F64_OPS = (OP_SUM_F64, OP_MIN_F64, OP_MAX_F64)  # f64 values in, f64 values out

STAT_COUNT = 0
STAT_SUM = 1
STAT_MIN = 2
STAT_MAX = 3

MAP_VALUES_ADD = 0
MAP_VALUES_MUL = 1
MAP_KEYS_ADD = 2
MAP_SWAP = 3
PRED_KEY_MOD_EQ = 0
PRED_VAL_GT = 1
PRED_KEY_IN_RANGE = 2

JOIN_INNER = 0
JOIN_LEFT_OUTER = 1
JOIN_RIGHT_OUTER = 2
JOIN_FULL_OUTER = 3
JOIN_LEFT_SEMI = 4
JOIN_LEFT_ANTI = 5
JOIN_HAS_A = 1  # bit in a presence byte: the row carries an A value
JOIN_HAS_B = 2

_lib = None


class VegaGpuError(RuntimeError):
    pass


def lib():
    global _lib
    if _lib is None:
        # Prefer the torch-runtime-linked variant and load torch FIRST, so
        # exactly one HIP runtime (torch's bundled one) lives in the process;
        # torch tensors/streams and our kernels then share it.
        path = LIBPATH
        if os.path.exists(LIBPATH_TORCH):
            try:
                import torch  # noqa: F401  (loads its libamdhip64.so)
                path = LIBPATH_TORCH
            except ImportError:
                pass
        if not os.path.exists(path):
            raise VegaGpuError(
                f"{path} not built — run __graft_entry__.build() (hipcc "
                "--offload-arch=gfx950); the GPU path has no fallback")
        _lib = ctypes.CDLL(path)
        _lib.vega_dev_ws_bytes.restype = ctypes.c_size_t
        _lib.vega_dev_ws_bytes.argtypes = [ctypes.c_uint64]
        _lib.vega_gpu_last_error.restype = ctypes.c_char_p
        _lib.vega_f64_order_key.restype = ctypes.c_uint64
        _lib.vega_f64_order_key.argtypes = [ctypes.c_uint64]
    return _lib


def _np(a, dtype=np.int64):
    return np.ascontiguousarray(a, dtype=dtype)


def _pp(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _check(rc, what, ctx=None):
    if rc != 0:
        extra = b""
        if ctx is not None:
            extra = lib().vega_gpu_last_error(ctx)
        err = VegaGpuError(f"{what} failed rc={rc} {extra!r}")
        err.rc = rc  # the VEGA_ERR_* code
        raise err


class VegaContext:
    """Mirrors Context (context.rs:147-164) + PairRdd ops for one GPU."""

    def __init__(self, ngpus=1):
        self._c = ctypes.c_void_p()
        _check(lib().vega_gpu_init(ngpus, ctypes.byref(self._c)), "init")

    def close(self):
        if self._c:
            lib().vega_gpu_shutdown(self._c)
            self._c = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # --- construction (context.rs:406-442 make_rdd/parallelize) ---
    def make_rdd(self, keys, vals, nparts=4):
        h = ctypes.c_uint64()
        if np.asarray(vals).dtype == np.float64:
            k = _np(keys)
            v = _np(vals, np.float64)
            _check(lib().vega_gpu_make_rdd_f64(self._c, _pp(k), _pp(v),
                                               ctypes.c_uint64(len(k)),
                                               ctypes.c_uint32(nparts),
                                               ctypes.byref(h)), "make_rdd_f64", self._c)
        else:
            k = _np(keys)
            v = _np(vals)
            _check(lib().vega_gpu_make_rdd(self._c, _pp(k), _pp(v),
                                           ctypes.c_uint64(len(k)),
                                           ctypes.c_uint32(nparts),
                                           ctypes.byref(h)), "make_rdd", self._c)
        return Rdd(self, h.value, np.asarray(vals).dtype)

    def gen_rdd_uniform(self, n, seed, key_bits=63, start=0, nparts=256):
        h = ctypes.c_uint64()
        _check(lib().vega_gpu_gen_rdd_uniform(
            self._c, ctypes.c_uint64(n), ctypes.c_uint64(seed),
            ctypes.c_int(key_bits), ctypes.c_uint64(start),
            ctypes.c_uint32(nparts), ctypes.byref(h)), "gen_rdd", self._c)
        return Rdd(self, h.value, np.dtype(np.int64))

    def synchronize(self):
        _check(lib().vega_gpu_synchronize(self._c), "sync", self._c)

    def set_profiling(self, on):
        lib().vega_gpu_set_profiling(self._c, 1 if on else 0)

    def kernel_stats(self):
        import json
        buf = ctypes.create_string_buffer(1 << 16)
        _check(lib().vega_gpu_kernel_stats(self._c, buf, len(buf)), "stats")
        return json.loads(buf.value.decode())


class Rdd:
    def __init__(self, ctx, handle, vdtype):
        self.ctx = ctx
        self.h = handle
        self.vdtype = np.dtype(vdtype)

    # --- PairRdd ops (pair_rdd.rs names) ---
    def reduce_by_key(self, op=OP_SUM_I64, nparts=256):
        out = ctypes.c_uint64()
        _check(lib().vega_gpu_reduce_by_key(self.ctx._c, ctypes.c_uint64(self.h),
                                            ctypes.c_int(op), ctypes.c_uint32(nparts),
                                            ctypes.byref(out)),
               "reduce_by_key", self.ctx._c)
        return Rdd(self.ctx, out.value,
                   np.float64 if op in F64_OPS else np.int64)

    def stats_by_key_f64(self, nparts=256):
        """the f64 combiner: per key (count, sum, min, max) over f64 values
        from one grouping sort; sum bit-identical to reduce_by_key(OP_SUM_F64),
        min / max as OP_MIN_F64 / OP_MAX_F64"""
        out = ctypes.c_uint64()
        _check(lib().vega_gpu_stats_by_key_f64(self.ctx._c, ctypes.c_uint64(self.h),
                                               ctypes.c_uint32(nparts), ctypes.byref(out)),
               "stats_by_key_f64", self.ctx._c)
        return StatsF64Rdd(self.ctx, out.value)

    def stats_by_key(self, nparts=256):
        """combine_by_key (pair_rdd.rs:20-33) with C = (count, sum, min, max)
        over i64 values, all four columns from one grouping sort"""
        out = ctypes.c_uint64()
        _check(lib().vega_gpu_stats_by_key(self.ctx._c, ctypes.c_uint64(self.h),
                                           ctypes.c_uint32(nparts), ctypes.byref(out)),
               "stats_by_key", self.ctx._c)
        return StatsRdd(self.ctx, out.value)

    def map(self, op, p0=0):
        out = ctypes.c_uint64()
        _check(lib().vega_gpu_map(self.ctx._c, ctypes.c_uint64(self.h),
                                  ctypes.c_int(op), ctypes.c_int64(p0),
                                  ctypes.byref(out)), "map", self.ctx._c)
        return Rdd(self.ctx, out.value, np.int64)

    def filter(self, pred, p0=0, p1=0):
        out = ctypes.c_uint64()
        _check(lib().vega_gpu_filter(self.ctx._c, ctypes.c_uint64(self.h),
                                     ctypes.c_int(pred), ctypes.c_int64(p0),
                                     ctypes.c_int64(p1), ctypes.byref(out)),
               "filter", self.ctx._c)
        return Rdd(self.ctx, out.value, np.int64)

    def distinct(self, nparts=256):
        out = ctypes.c_uint64()
        _check(lib().vega_gpu_distinct(self.ctx._c, ctypes.c_uint64(self.h),
                                       ctypes.c_uint32(nparts), ctypes.byref(out)),
               "distinct", self.ctx._c)
        return Rdd(self.ctx, out.value, np.int64)

    def count_by_value(self, nparts=256):
        out = ctypes.c_uint64()
        _check(lib().vega_gpu_count_by_value(self.ctx._c, ctypes.c_uint64(self.h),
                                             ctypes.c_uint32(nparts), ctypes.byref(out)),
               "count_by_value", self.ctx._c)
        return Rdd(self.ctx, out.value, np.int64)

    def group_by_key(self):
        """Full groups (pair_rdd.rs:35-52, aggregator.rs:33-53) materialized
        IN THE ENGINE (vega_gpu_group_by_key): returns (keys, offsets,
        values) — values in grouped order, value order within a group = row
        order (stable grouping sort)."""
        out = ctypes.c_uint64()
        _check(lib().vega_gpu_group_by_key(self.ctx._c, ctypes.c_uint64(self.h),
                                           ctypes.c_uint32(256), ctypes.byref(out)),
               "group_by_key", self.ctx._c)
        g = Rdd(self.ctx, out.value, self.vdtype)
        nk = ctypes.c_uint64(0)
        nvals = ctypes.c_uint64(0)
        _check(lib().vega_gpu_collect_groups(self.ctx._c, ctypes.c_uint64(g.h),
                                             None, None, None,
                                             ctypes.byref(nk), ctypes.byref(nvals)),
               "collect_groups size", self.ctx._c)
        keys = np.empty(nk.value, dtype=np.int64)
        offsets = np.empty(nk.value + 1, dtype=np.uint64)
        values = np.empty(nvals.value, dtype=self.vdtype)
        _check(lib().vega_gpu_collect_groups(self.ctx._c, ctypes.c_uint64(g.h),
                                             _pp(keys), _pp(offsets), _pp(values),
                                             ctypes.byref(nk), ctypes.byref(nvals)),
               "collect_groups", self.ctx._c)
        g.free()
        return keys, offsets.astype(np.int64), values

    def cogroup(self, other):
        """cogroup (pair_rdd.rs:123-155): for every key in either side the
        (Vec<V>, Vec<W>) ranges. Returns (keys, offa, lena, offb, lenb,
        vala, valb)."""
        na, nb = self.count(), other.count()
        cap = na + nb
        keys = np.empty(max(cap, 1), dtype=np.int64)
        offa = np.empty(max(cap, 1), dtype=np.uint64)
        lena = np.empty(max(cap, 1), dtype=np.uint64)
        offb = np.empty(max(cap, 1), dtype=np.uint64)
        lenb = np.empty(max(cap, 1), dtype=np.uint64)
        vala = np.empty(max(na, 1), dtype=np.int64)
        valb = np.empty(max(nb, 1), dtype=np.int64)
        nk = ctypes.c_uint64(0)
        _check(lib().vega_gpu_cogroup_collect(
            self.ctx._c, ctypes.c_uint64(self.h), ctypes.c_uint64(other.h),
            _pp(keys), _pp(offa), _pp(lena), _pp(offb), _pp(lenb),
            _pp(vala), _pp(valb), ctypes.c_uint64(cap), ctypes.byref(nk)),
            "cogroup", self.ctx._c)
        n = nk.value
        return (keys[:n], offa[:n].astype(np.int64), lena[:n].astype(np.int64),
                offb[:n].astype(np.int64), lenb[:n].astype(np.int64),
                vala[:na], valb[:nb])

    def intersection(self, other, nparts=256):
        """distinct keys present in both sides (rdd.rs set semantics)"""
        out = ctypes.c_uint64()
        _check(lib().vega_gpu_intersection(self.ctx._c, ctypes.c_uint64(self.h),
                                           ctypes.c_uint64(other.h),
                                           ctypes.c_uint32(nparts), ctypes.byref(out)),
               "intersection", self.ctx._c)
        return Rdd(self.ctx, out.value, np.int64)

    def subtract(self, other, nparts=256):
        """distinct keys of self absent from other"""
        out = ctypes.c_uint64()
        _check(lib().vega_gpu_subtract(self.ctx._c, ctypes.c_uint64(self.h),
                                       ctypes.c_uint64(other.h),
                                       ctypes.c_uint32(nparts), ctypes.byref(out)),
               "subtract", self.ctx._c)
        return Rdd(self.ctx, out.value, np.int64)

    def group_count(self, nparts=256):
        out = ctypes.c_uint64()
        _check(lib().vega_gpu_group_count(self.ctx._c, ctypes.c_uint64(self.h),
                                          ctypes.c_uint32(nparts), ctypes.byref(out)),
               "group_count", self.ctx._c)
        return Rdd(self.ctx, out.value, np.int64)

    def sort_by_key(self):
        out = ctypes.c_uint64()
        _check(lib().vega_gpu_sort_by_key(self.ctx._c, ctypes.c_uint64(self.h),
                                          ctypes.byref(out)), "sort_by_key", self.ctx._c)
        return Rdd(self.ctx, out.value, self.vdtype)

    def join(self, other, nparts=256):
        out = ctypes.c_uint64()
        _check(lib().vega_gpu_join(self.ctx._c, ctypes.c_uint64(self.h),
                                   ctypes.c_uint64(other.h), ctypes.c_uint32(nparts),
                                   ctypes.byref(out)), "join", self.ctx._c)
        r = Rdd(self.ctx, out.value, np.int64)
        r.is_join = True
        return r

    def collect_join(self):
        n = ctypes.c_uint64(self.count())
        k = np.empty(n.value, dtype=np.int64)
        va = np.empty(n.value, dtype=np.int64)
        vb = np.empty(n.value, dtype=np.int64)
        _check(lib().vega_gpu_collect_join(self.ctx._c, ctypes.c_uint64(self.h),
                                           _pp(k), _pp(va), _pp(vb), ctypes.byref(n)),
               "collect_join", self.ctx._c)
        return k[:n.value], va[:n.value], vb[:n.value]

    def join_kind(self, other, kind, nparts=256):
        """the join family (vega_gpu_join_kind). JOIN_INNER .. JOIN_FULL_OUTER
        give a join result (collect_join_outer / collect_join); JOIN_LEFT_SEMI
        and JOIN_LEFT_ANTI give a plain Rdd: the rows of self whose key does /
        does not occur in other, in self's row order, value type kept."""
        out = ctypes.c_uint64()
        _check(lib().vega_gpu_join_kind(self.ctx._c, ctypes.c_uint64(self.h),
                                        ctypes.c_uint64(other.h), ctypes.c_int(kind),
                                        ctypes.c_uint32(nparts), ctypes.byref(out)),
               "join_kind", self.ctx._c)
        if kind in (JOIN_LEFT_SEMI, JOIN_LEFT_ANTI):
            return Rdd(self.ctx, out.value, self.vdtype)
        r = Rdd(self.ctx, out.value, np.int64)
        r.is_join = True
        return r

    def left_outer_join(self, other, nparts=256):
        return self.join_kind(other, JOIN_LEFT_OUTER, nparts)

    def right_outer_join(self, other, nparts=256):
        return self.join_kind(other, JOIN_RIGHT_OUTER, nparts)

    def full_outer_join(self, other, nparts=256):
        return self.join_kind(other, JOIN_FULL_OUTER, nparts)

    def semi_join(self, other, nparts=256):
        """rows of self whose key occurs in other (row order, duplicates kept)"""
        return self.join_kind(other, JOIN_LEFT_SEMI, nparts)

    def subtract_by_key(self, other, nparts=256):
        """Spark's subtractByKey, the anti join: rows of self whose key does
        not occur in other (row order, duplicates kept)"""
        return self.join_kind(other, JOIN_LEFT_ANTI, nparts)

    def collect_join_outer(self):
        """(k, va, vb, present) of any join result; present[i] has JOIN_HAS_A /
        JOIN_HAS_B set, an absent side's value is 0 (an inner result: all 3)"""
        n = ctypes.c_uint64(0)
        _check(lib().vega_gpu_collect_join_outer(self.ctx._c, ctypes.c_uint64(self.h),
                                                 None, None, None, None, ctypes.byref(n)),
               "collect_join_outer size", self.ctx._c)
        k = np.empty(n.value, dtype=np.int64)
        va = np.empty(n.value, dtype=np.int64)
        vb = np.empty(n.value, dtype=np.int64)
        pr = np.empty(n.value, dtype=np.uint8)
        _check(lib().vega_gpu_collect_join_outer(self.ctx._c, ctypes.c_uint64(self.h),
                                                 _pp(k), _pp(va), _pp(vb), _pp(pr),
                                                 ctypes.byref(n)),
               "collect_join_outer", self.ctx._c)
        return k[:n.value], va[:n.value], vb[:n.value], pr[:n.value]

    # --- actions (rdd.rs collect/count) ---
    def count(self):
        n = ctypes.c_uint64()
        _check(lib().vega_gpu_count(self.ctx._c, ctypes.c_uint64(self.h),
                                    ctypes.byref(n)), "count", self.ctx._c)
        return n.value

    def collect(self):
        n = ctypes.c_uint64(self.count())
        k = np.empty(n.value, dtype=np.int64)
        v = np.empty(n.value, dtype=self.vdtype)
        _check(lib().vega_gpu_collect(self.ctx._c, ctypes.c_uint64(self.h),
                                      _pp(k), _pp(v), ctypes.byref(n)),
               "collect", self.ctx._c)
        return k[:n.value], v[:n.value]

    # --- device-side actions (rdd.rs:274-322, :534-620, :1073-1153) ---
    def _vbox(self, op=None):
        f64 = (op in F64_OPS) if op is not None else self.vdtype == np.float64
        return ctypes.c_double() if f64 else ctypes.c_int64()

    def reduce(self, op=OP_SUM_I64):
        """column-wise reduce -> (k, v), or None on an empty rdd"""
        k = ctypes.c_int64()
        v = self._vbox(op)
        ne = ctypes.c_int(0)
        _check(lib().vega_gpu_reduce(self.ctx._c, ctypes.c_uint64(self.h),
                                     ctypes.c_int(op), ctypes.byref(k),
                                     ctypes.byref(v), ctypes.byref(ne)),
               "reduce", self.ctx._c)
        return (k.value, v.value) if ne.value else None

    def fold(self, op, init_k, init_v):
        """fold (rdd.rs:311-322): init combined nparts+1 times with reduce"""
        k = ctypes.c_int64()
        v = self._vbox(op)
        iv = ctypes.c_double(init_v) if op in F64_OPS else ctypes.c_int64(init_v)
        _check(lib().vega_gpu_fold(self.ctx._c, ctypes.c_uint64(self.h),
                                   ctypes.c_int(op), ctypes.c_int64(init_k),
                                   ctypes.byref(iv), ctypes.byref(k), ctypes.byref(v)),
               "fold", self.ctx._c)
        return k.value, v.value

    def _extreme(self, fn, what):
        k = ctypes.c_int64()
        v = ctypes.c_int64()
        ne = ctypes.c_int(0)
        _check(fn(self.ctx._c, ctypes.c_uint64(self.h), ctypes.byref(k),
                  ctypes.byref(v), ctypes.byref(ne)), what, self.ctx._c)
        return (k.value, v.value) if ne.value else None

    def min(self):
        """lexicographic smallest row, or None on an empty rdd"""
        return self._extreme(lib().vega_gpu_min, "min")

    def max(self):
        return self._extreme(lib().vega_gpu_max, "max")

    def _out_rows(self, num):
        # the entries write min(num, n) rows: a small num sizes the buffers
        # itself, only a large one is worth a count() call to trim it
        num = int(num)
        return num if num <= (1 << 16) else min(num, self.count())

    def take(self, num):
        """first min(num, n) rows in partition order -> (keys, vals)"""
        m = self._out_rows(num)
        k = np.empty(m, dtype=np.int64)
        v = np.empty(m, dtype=self.vdtype)
        n = ctypes.c_uint64(0)
        _check(lib().vega_gpu_take(self.ctx._c, ctypes.c_uint64(self.h),
                                   ctypes.c_uint64(num), _pp(k), _pp(v),
                                   ctypes.byref(n)), "take", self.ctx._c)
        return k[:n.value], v[:n.value]

    def first(self):
        """first row; raises VegaGpuError (empty collection) on an empty rdd"""
        k = ctypes.c_int64()
        v = self._vbox()
        _check(lib().vega_gpu_first(self.ctx._c, ctypes.c_uint64(self.h),
                                    ctypes.byref(k), ctypes.byref(v)),
               "first", self.ctx._c)
        return k.value, v.value

    def is_empty(self):
        e = ctypes.c_int(0)
        _check(lib().vega_gpu_is_empty(self.ctx._c, ctypes.c_uint64(self.h),
                                       ctypes.byref(e)), "is_empty", self.ctx._c)
        return bool(e.value)

    def _ordered(self, fn, what, num):
        m = self._out_rows(num)
        k = np.empty(m, dtype=np.int64)
        v = np.empty(m, dtype=np.int64)
        n = ctypes.c_uint64(0)
        _check(fn(self.ctx._c, ctypes.c_uint64(self.h), ctypes.c_uint64(num),
                  _pp(k), _pp(v), ctypes.byref(n)), what, self.ctx._c)
        return k[:n.value], v[:n.value]

    def take_ordered(self, num):
        """min(num, n) lexicographically smallest rows, ascending"""
        return self._ordered(lib().vega_gpu_take_ordered, "take_ordered", num)

    def top(self, num):
        """min(num, n) lexicographically largest rows, descending"""
        return self._ordered(lib().vega_gpu_top, "top", num)

    # --- samplers (rdd.rs:623-783); seed=None draws a 64-bit seed on the host ---
    def sample(self, with_replacement, fraction, seed=None):
        """Bernoulli (with_replacement false: each row kept with probability
        fraction) or Poisson (true: each row emitted Poisson(fraction) times
        in place) sample; row order kept, value type kept. The choice for row
        i depends on (seed, i) only."""
        out = ctypes.c_uint64()
        _check(lib().vega_gpu_sample(self.ctx._c, ctypes.c_uint64(self.h),
                                     ctypes.c_int(1 if with_replacement else 0),
                                     ctypes.c_double(fraction),
                                     ctypes.c_uint64(_seed(seed)), ctypes.byref(out)),
               "sample", self.ctx._c)
        return Rdd(self.ctx, out.value, self.vdtype)

    def random_split(self, weights, seed=None):
        """list of len(weights) disjoint Rdds whose union is this one, sized
        in proportion to the weights; each keeps row order"""
        w = _np(weights, np.float64)
        outs = (ctypes.c_uint64 * max(len(w), 1))()
        _check(lib().vega_gpu_random_split(self.ctx._c, ctypes.c_uint64(self.h),
                                           _pp(w), ctypes.c_uint32(len(w)),
                                           ctypes.c_uint64(_seed(seed)), outs),
               "random_split", self.ctx._c)
        return [Rdd(self.ctx, outs[j], self.vdtype) for j in range(len(w))]

    def take_sample(self, with_replacement, num, seed=None):
        """min(num, candidates) uniformly chosen rows in random order ->
        (keys, vals) on the host"""
        m = int(num)
        if not with_replacement:  # at most n rows come back
            m = min(m, self.count())
        k = np.empty(m, dtype=np.int64)
        v = np.empty(m, dtype=self.vdtype)
        n = ctypes.c_uint64(0)
        _check(lib().vega_gpu_take_sample(self.ctx._c, ctypes.c_uint64(self.h),
                                          ctypes.c_int(1 if with_replacement else 0),
                                          ctypes.c_uint64(num),
                                          ctypes.c_uint64(_seed(seed)), _pp(k), _pp(v),
                                          ctypes.byref(n)), "take_sample", self.ctx._c)
        return k[:n.value], v[:n.value]

    def free(self):
        lib().vega_gpu_free_rdd(self.ctx._c, ctypes.c_uint64(self.h))


def _seed(seed):
    """the reference's Option<u64> seed: None draws 64 bits on the host"""
    if seed is None:
        return int.from_bytes(os.urandom(8), "little")
    return int(seed) & 0xFFFFFFFFFFFFFFFF


def sample_poisson_table(fraction):
    """the integer threshold table the Poisson sampler uses (host only)"""
    thr = np.zeros(256, dtype=np.uint64)
    n = ctypes.c_int(0)
    _check(lib().vega_sample_poisson_table(ctypes.c_double(fraction), _pp(thr),
                                           ctypes.byref(n)), "sample_poisson_table")
    return thr[:n.value].copy()


class StatsRdd:
    """result of Rdd.stats_by_key: per key (count, sum, min, max)"""

    def __init__(self, ctx, handle):
        self.ctx = ctx
        self.h = handle

    def count(self):
        """number of keys"""
        n = ctypes.c_uint64()
        _check(lib().vega_gpu_count(self.ctx._c, ctypes.c_uint64(self.h),
                                    ctypes.byref(n)), "count", self.ctx._c)
        return n.value

    def collect(self):
        """(keys, count, sum, min, max) as int64 arrays, rows aligned"""
        n = ctypes.c_uint64(0)
        _check(lib().vega_gpu_collect_stats(self.ctx._c, ctypes.c_uint64(self.h),
                                            None, None, None, None, None,
                                            ctypes.byref(n)),
               "collect_stats size", self.ctx._c)
        cols = [np.empty(n.value, dtype=np.int64) for _ in range(5)]
        _check(lib().vega_gpu_collect_stats(self.ctx._c, ctypes.c_uint64(self.h),
                                            *[_pp(a) for a in cols], ctypes.byref(n)),
               "collect_stats", self.ctx._c)
        return tuple(a[:n.value] for a in cols)

    def column(self, which):
        """map_values(|c| c.<which>): a plain (key, column) Rdd (device copy)"""
        out = ctypes.c_uint64()
        _check(lib().vega_gpu_stats_column(self.ctx._c, ctypes.c_uint64(self.h),
                                           ctypes.c_int(which), ctypes.byref(out)),
               "stats_column", self.ctx._c)
        return Rdd(self.ctx, out.value, np.int64)

    def free(self):
        lib().vega_gpu_free_rdd(self.ctx._c, ctypes.c_uint64(self.h))


class StatsF64Rdd:
    """result of Rdd.stats_by_key_f64: per key (count i64, sum, min, max f64)"""

    def __init__(self, ctx, handle):
        self.ctx = ctx
        self.h = handle

    def count(self):
        """number of keys"""
        n = ctypes.c_uint64()
        _check(lib().vega_gpu_count(self.ctx._c, ctypes.c_uint64(self.h),
                                    ctypes.byref(n)), "count", self.ctx._c)
        return n.value

    def collect(self):
        """(keys i64, count i64, sum f64, min f64, max f64), rows aligned"""
        n = ctypes.c_uint64(0)
        _check(lib().vega_gpu_collect_stats_f64(self.ctx._c, ctypes.c_uint64(self.h),
                                                None, None, None, None, None,
                                                ctypes.byref(n)),
               "collect_stats_f64 size", self.ctx._c)
        cols = [np.empty(n.value, dtype=np.int64) for _ in range(2)] + [
            np.empty(n.value, dtype=np.float64) for _ in range(3)]
        _check(lib().vega_gpu_collect_stats_f64(self.ctx._c, ctypes.c_uint64(self.h),
                                                *[_pp(a) for a in cols], ctypes.byref(n)),
               "collect_stats_f64", self.ctx._c)
        return tuple(a[:n.value] for a in cols)

    def column(self, which):
        """map_values(|c| c.<which>): a plain (key, column) Rdd (device copy);
        the count is i64-valued, sum / min / max f64-valued"""
        out = ctypes.c_uint64()
        _check(lib().vega_gpu_stats_column(self.ctx._c, ctypes.c_uint64(self.h),
                                           ctypes.c_int(which), ctypes.byref(out)),
               "stats_column", self.ctx._c)
        return Rdd(self.ctx, out.value, np.int64 if which == STAT_COUNT else np.float64)

    def free(self):
        lib().vega_gpu_free_rdd(self.ctx._c, ctypes.c_uint64(self.h))


def f64_order_key(a):
    """the order key of each element of a, as int64: the signed order MIN_F64 /
    MAX_F64 compare by. a is a float64 array, or a uint64 / int64 array of bit
    patterns (any other dtype: TypeError). Host only; it calls the exported
    vega_f64_order_key once per element — meant for checks and small arrays,
    not for columns."""
    a = np.ascontiguousarray(a)
    if a.dtype not in (np.float64, np.uint64, np.int64):
        raise TypeError(f"f64_order_key: float64, uint64 or int64 expected, not {a.dtype}")
    bits = a.view(np.uint64)
    fn = lib().vega_f64_order_key
    out = np.fromiter((fn(int(b)) for b in bits.ravel()), dtype=np.uint64, count=bits.size)
    return out.view(np.int64).reshape(bits.shape)


# ---------------- device-pointer API over torch tensors ----------------

def _t(t):
    return ctypes.c_void_p(t.data_ptr())


def _stream():
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def ws_bytes(n):
    return int(lib().vega_dev_ws_bytes(ctypes.c_uint64(n)))


def alloc_ws(n, device="cuda"):
    import torch
    return torch.empty(ws_bytes(n), dtype=torch.uint8, device=device)


def dev_gen_uniform(keys_t, vals_t, seed, key_bits=63, start=0):
    n = keys_t.numel()
    _check(lib().vega_dev_gen_uniform_i64(_stream(), _t(keys_t), _t(vals_t),
                                          ctypes.c_uint64(n), ctypes.c_uint64(seed),
                                          ctypes.c_int(key_bits), ctypes.c_uint64(start)),
           "dev_gen")


def dev_gen_uniform_f64(keys_t, vals_t, seed, key_bits=63, start=0):
    n = keys_t.numel()
    _check(lib().vega_dev_gen_uniform_f64(_stream(), _t(keys_t), _t(vals_t),
                                          ctypes.c_uint64(n), ctypes.c_uint64(seed),
                                          ctypes.c_int(key_bits), ctypes.c_uint64(start)),
           "dev_gen_f64")


def dev_partition(keys_t, vals_t, nparts, out_k, out_v, ws_t):
    n = keys_t.numel()
    counts = np.zeros(nparts, dtype=np.uint64)
    _check(lib().vega_dev_partition_i64(_stream(), _t(keys_t), _t(vals_t),
                                        ctypes.c_uint64(n), ctypes.c_uint32(nparts),
                                        _t(out_k), _t(out_v), _pp(counts),
                                        _t(ws_t), ctypes.c_size_t(ws_t.numel())),
           "dev_partition")
    return counts


def dev_partition_range(keys_t, vals_t, splitters_t, out_k, out_v, ws_t):
    """range partition: bucket = #splitters <= key; splitters_t is a device
    tensor of nparts-1 ascending i64 splitters"""
    n = keys_t.numel()
    nparts = splitters_t.numel() + 1
    counts = np.zeros(nparts, dtype=np.uint64)
    _check(lib().vega_dev_partition_range_i64(
        _stream(), _t(keys_t), _t(vals_t), ctypes.c_uint64(n),
        ctypes.c_uint32(nparts), _t(splitters_t), _t(out_k), _t(out_v),
        _pp(counts), _t(ws_t), ctypes.c_size_t(ws_t.numel())),
        "dev_partition_range")
    return counts


def dev_sort_reduce(keys_t, vals_t, op, out_k, out_v, ws_t):
    n = keys_t.numel()
    nout = ctypes.c_uint64()
    _check(lib().vega_dev_sort_reduce(_stream(), _t(keys_t), _t(vals_t),
                                      ctypes.c_uint64(n), ctypes.c_int(op),
                                      _t(out_k), _t(out_v), ctypes.byref(nout),
                                      _t(ws_t), ctypes.c_size_t(ws_t.numel())),
           "dev_sort_reduce")
    return nout.value


def dev_sort_stats(keys_t, vals_t, out_k, out_count, out_sum, out_min, out_max, ws_t):
    """grouping sort + fused (count, sum, min, max) per key; the five out
    tensors hold n rows each; returns the number of keys"""
    n = keys_t.numel()
    nout = ctypes.c_uint64()
    _check(lib().vega_dev_sort_stats_i64(_stream(), _t(keys_t), _t(vals_t),
                                         ctypes.c_uint64(n), _t(out_k), _t(out_count),
                                         _t(out_sum), _t(out_min), _t(out_max),
                                         ctypes.byref(nout),
                                         _t(ws_t), ctypes.c_size_t(ws_t.numel())),
           "dev_sort_stats")
    return nout.value


def dev_sort_stats_f64(keys_t, vals_t, out_k, out_count, out_sum, out_min, out_max, ws_t):
    """dev_sort_stats for f64 values: out_k / out_count int64, out_sum / out_min /
    out_max float64, n rows each; returns the number of keys"""
    n = keys_t.numel()
    nout = ctypes.c_uint64()
    _check(lib().vega_dev_sort_stats_f64(_stream(), _t(keys_t), _t(vals_t),
                                         ctypes.c_uint64(n), _t(out_k), _t(out_count),
                                         _t(out_sum), _t(out_min), _t(out_max),
                                         ctypes.byref(nout),
                                         _t(ws_t), ctypes.c_size_t(ws_t.numel())),
           "dev_sort_stats_f64")
    return nout.value


def dev_group_rows(keys_t, vals_t, route, out_k, out_v, ws_t):
    """diagnostic: the grouped rows dev_sort_reduce aggregates, as SoA columns.
    route 0 automatic, 1 four hash passes + cleanup, 2 three passes + bucket
    finish; returns the route that produced the result"""
    taken = ctypes.c_int(0)
    _check(lib().vega_dev_group_rows_i64(
        _stream(), _t(keys_t), _t(vals_t), ctypes.c_uint64(keys_t.numel()),
        ctypes.c_int(route), _t(out_k), _t(out_v), _t(ws_t),
        ctypes.c_size_t(ws_t.numel()), ctypes.byref(taken)), "dev_group_rows")
    return taken.value


def diag_bucket_rows(sample_keys, n):
    """rows per occupied hash bucket the automatic route would estimate for n
    rows from these (<= 2048, host) sampled keys; no device call"""
    k = _np(sample_keys)
    out = ctypes.c_double(0)
    _check(lib().vega_diag_bucket_rows(_pp(k), ctypes.c_uint32(len(k)),
                                       ctypes.c_uint64(n), ctypes.byref(out)),
           "diag_bucket_rows")
    return out.value


def dev_sort_pairs(keys_t, vals_t, ws_t):
    n = keys_t.numel()
    _check(lib().vega_dev_sort_pairs_i64(_stream(), _t(keys_t), _t(vals_t),
                                         ctypes.c_uint64(n), _t(ws_t),
                                         ctypes.c_size_t(ws_t.numel())),
           "dev_sort_pairs")


def dev_group_pairs(keys_t, vals_t, ws_t):
    """in-place grouping-order sort; returns the order tag (4 = (h32,key)
    lex usable with dev_join_grouped mode 2; 0 = full unsigned-key order)"""
    tag = ctypes.c_int(0)
    _check(lib().vega_dev_group_pairs_i64(
        _stream(), _t(keys_t), _t(vals_t), ctypes.c_uint64(keys_t.numel()),
        ctypes.byref(tag), _t(ws_t), ctypes.c_size_t(ws_t.numel())), "dev_group_pairs")
    return tag.value


def dev_join_grouped(ak, av, bk, bv, order_mode, out_k, out_va, out_vb, ws_t):
    nout = ctypes.c_uint64()
    _check(lib().vega_dev_join_grouped(
        _stream(), _t(ak), _t(av), ctypes.c_uint64(ak.numel()),
        _t(bk), _t(bv), ctypes.c_uint64(bk.numel()), ctypes.c_int(order_mode),
        _t(out_k), _t(out_va), _t(out_vb), ctypes.c_uint64(out_k.numel()),
        ctypes.byref(nout), _t(ws_t), ctypes.c_size_t(ws_t.numel())),
        "dev_join_grouped")
    return nout.value


def dev_join_grouped_kind(ak, av, bk, bv, order_mode, kind, out=None, ws_t=None):
    """kinds JOIN_INNER .. JOIN_FULL_OUTER on device sides that are both in
    the order named by order_mode. Returns (out_k, out_va, out_vb, present,
    needed), the tensors trimmed to the result. out = (out_k, out_va, out_vb,
    present) caller-given tensors: when too small the call raises VegaGpuError
    with rc == -5 (VEGA_ERR_CAP) and .needed = the rows the join holds, and
    nothing is written. Without them a count-only call sizes them."""
    import torch
    na, nb = ak.numel(), bk.numel()
    if ws_t is None:
        ws_t = alloc_ws(max(na, nb), ak.device)
    nout = ctypes.c_uint64(0)

    def call(o, cap):
        return lib().vega_dev_join_grouped_kind(
            _stream(), _t(ak), _t(av), ctypes.c_uint64(na),
            _t(bk), _t(bv), ctypes.c_uint64(nb), ctypes.c_int(order_mode),
            ctypes.c_int(kind), *[_t(x) if x is not None else None for x in o],
            ctypes.c_uint64(cap), ctypes.byref(nout),
            _t(ws_t), ctypes.c_size_t(ws_t.numel()))

    if out is None:
        _check(call((None, None, None, None), 0), "dev_join_grouped_kind count")
        m = max(nout.value, 1)
        out = tuple(torch.empty(m, dtype=torch.int64, device=ak.device) for _ in range(3)) + (
            torch.empty(m, dtype=torch.uint8, device=ak.device),)
    rc = call(out, min(x.numel() for x in out))
    if rc != 0:
        err = VegaGpuError(f"dev_join_grouped_kind failed rc={rc} (needed {nout.value} rows)")
        err.rc = rc
        err.needed = nout.value
        raise err
    return tuple(x[:nout.value] for x in out) + (nout.value,)


def dev_join_sorted(ak, av, bk, bv, out_k, out_va, out_vb, ws_t):
    """sort-merge inner join of two KEY-SORTED sides; returns rows emitted"""
    nout = ctypes.c_uint64()
    _check(lib().vega_dev_join_sorted(
        _stream(), _t(ak), _t(av), ctypes.c_uint64(ak.numel()),
        _t(bk), _t(bv), ctypes.c_uint64(bk.numel()),
        _t(out_k), _t(out_va), _t(out_vb), ctypes.c_uint64(out_k.numel()),
        ctypes.byref(nout), _t(ws_t), ctypes.c_size_t(ws_t.numel())),
        "dev_join_sorted")
    return nout.value


def dev_checksum(keys_t, vals_t, ws_t):
    n = keys_t.numel()
    s = ctypes.c_uint64()
    _check(lib().vega_dev_checksum_pairs(_stream(), _t(keys_t), _t(vals_t),
                                         ctypes.c_uint64(n), ctypes.byref(s),
                                         _t(ws_t), ctypes.c_size_t(ws_t.numel())),
           "dev_checksum")
    return s.value


def select_ws_bytes(num, cand_cap=0):
    fn = lib().vega_dev_select_ws_bytes
    fn.restype = ctypes.c_size_t
    fn.argtypes = [ctypes.c_uint64, ctypes.c_uint64]
    return int(fn(num, cand_cap))


def dev_select_k(keys_t, vals_t, num, descending=False, cand_cap=0, ws_t=None):
    """MSB radix select on device tensors: the min(num, n) smallest
    (descending: largest) rows in order. Returns (out_k, out_v, passes);
    ws_t defaults to a fresh workspace of select_ws_bytes(min(num, n))."""
    import torch
    n = keys_t.numel()
    m = min(int(num), n)
    if ws_t is None:
        ws_t = torch.empty(select_ws_bytes(m, cand_cap), dtype=torch.uint8,
                           device=keys_t.device)
    out_k = torch.empty(m, dtype=torch.int64, device=keys_t.device)
    out_v = torch.empty(m, dtype=torch.int64, device=keys_t.device)
    nout = ctypes.c_uint64(0)
    passes = ctypes.c_int(0)
    _check(lib().vega_dev_select_k_i64(
        _stream(), _t(keys_t), _t(vals_t), ctypes.c_uint64(n), ctypes.c_uint64(num),
        ctypes.c_int(1 if descending else 0), ctypes.c_uint64(cand_cap),
        _t(out_k), _t(out_v), ctypes.byref(nout), ctypes.byref(passes),
        _t(ws_t), ctypes.c_size_t(ws_t.numel())), "dev_select_k")
    return out_k[:nout.value], out_v[:nout.value], passes.value


def dev_reduce_pairs(keys_t, vals_t, op, ws_t=None):
    """column-wise reduce of device rows -> (k, v) on the host"""
    import torch
    if ws_t is None:
        ws_t = torch.empty(1 << 16, dtype=torch.uint8, device=keys_t.device)
    k = ctypes.c_int64()
    v = ctypes.c_double() if op in F64_OPS else ctypes.c_int64()
    _check(lib().vega_dev_reduce_pairs(
        _stream(), _t(keys_t), _t(vals_t), ctypes.c_uint64(keys_t.numel()),
        ctypes.c_int(op), ctypes.byref(k), ctypes.byref(v),
        _t(ws_t), ctypes.c_size_t(ws_t.numel())), "dev_reduce_pairs")
    return k.value, v.value


def dev_sample(keys_t, vals_t, with_replacement, fraction, seed, start=0,
               out_k=None, out_v=None, ws_t=None):
    """sample of device rows whose first row has the global index `start`
    (shards sampled with their own start are the slices of the whole sample).
    Returns (out_k, out_v, needed): the tensors trimmed to the sample. With
    caller-given out tensors that are too small the call raises VegaGpuError
    with rc == -5 (VEGA_ERR_CAP) and .needed = the rows the sample holds;
    nothing is written then. Without them a count-only call sizes them."""
    import torch
    n = keys_t.numel()
    if ws_t is None:
        ws_t = alloc_ws(n, keys_t.device)
    nout = ctypes.c_uint64(0)

    def call(ok, ov, cap):
        return lib().vega_dev_sample(
            _stream(), _t(keys_t), _t(vals_t), ctypes.c_uint64(n),
            ctypes.c_int(1 if with_replacement else 0), ctypes.c_double(fraction),
            ctypes.c_uint64(_seed(seed)), ctypes.c_uint64(start),
            _t(ok) if ok is not None else None, _t(ov) if ov is not None else None,
            ctypes.c_uint64(cap), ctypes.byref(nout),
            _t(ws_t), ctypes.c_size_t(ws_t.numel()))

    if out_k is None:
        seed = _seed(seed)  # one seed for the sizing call and the real one
        rc = call(None, None, 0)
        if rc not in (0, -5):
            _check(rc, "dev_sample")
        out_k = torch.empty(max(nout.value, 1), dtype=torch.int64, device=keys_t.device)
        out_v = torch.empty(max(nout.value, 1), dtype=vals_t.dtype, device=keys_t.device)
    rc = call(out_k, out_v, min(out_k.numel(), out_v.numel()))
    if rc != 0:
        err = VegaGpuError(f"dev_sample failed rc={rc} (needed {nout.value} rows)")
        err.rc = rc
        err.needed = nout.value
        raise err
    return out_k[:nout.value], out_v[:nout.value], nout.value


def prof_enable(on=True):
    lib().vega_prof_enable(1 if on else 0)


def prof_stats():
    import json
    buf = ctypes.create_string_buffer(1 << 16)
    _check(lib().vega_prof_stats(buf, len(buf)), "prof_stats")
    return json.loads(buf.value.decode())
