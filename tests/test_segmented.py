"""Segmented reduce and the sort-based group-by (ops/segmented.py,
src/gpu/seg_reduce.hip, ops/aggregate.py groupby_sorted): the native kernels
and their CPU twin against two oracles that use neither the op nor a torch
scan - the pattern of tests/test_window.py.

* The LOOP ORACLE walks the segments in plain Python, one function at a time:
  math.fsum for float sums, an explicit NaN-greatest comparison for min and
  max.
* The NUMPY ORACLE is vectorised (np.add.reduceat / np.minimum.reduceat on
  head indices) for the one large size, and is itself checked against the
  loop oracle at small sizes.
* `groupby_tensors` is checked against a Python dict keyed by normalised key
  tuples (null -> a sentinel, NaN -> one token, -0.0 -> 0.0).

Exact: count, integer sum (wrapping), min, max, all validity, the data word
under a null (zero), first_rows, the segment count, and float sums over
quarter-integers (every partial sum is exactly representable, so any order of
summation is exact). With a bound, the one tests/test_window.py derives in its
header: float sum over general values, |got - want| <= k * 2**-52 * sum|x_j|
with k the number of valid values of the segment (gamma_(k-1) * sum|x| for
any summation order plus the oracle's one rounding); avg takes that bound
divided by the count plus one ulp of the quotient.
"""
import functools
import math

import numpy as np
import pytest
import torch

from spark_rapids_jni_amd import _native
from spark_rapids_jni_amd.columnar import Column, DType, Table
from spark_rapids_jni_amd.ops import segmented as SG

T = SG.TILE_ROWS
S = SG.SMALL_ROWS
SIZES = sorted({0, 1, 2, 63, 64, 65, S - 1, S, S + 1, T + 1, 3 * T + 7})
# the carry scan takes CARRY_CHUNK tile carries per round: two rounds
TWO_CHUNKS = SG.CARRY_CHUNK * T + 1
assert TWO_CHUNKS <= 1 << 22  # else the case would have to be left out
PATTERNS = ["one", "each", "random5", "span", "aligned"]
NULLS = ["none", "all", "interior", "segment"]
DTYPES = ["bool", "int8", "int16", "int32", "int64", "float32", "float64"]
NP_DTYPE = {"bool": np.bool_, "int8": np.int8, "int16": np.int16,
            "int32": np.int32, "int64": np.int64, "float32": np.float32,
            "float64": np.float64}
FNS = ["count", "sum", "min", "max", "avg"]
I64 = np.iinfo(np.int64)


# ---------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------

def make_structure(m, pattern, seed):
    """perm (a genuine shuffle) and normalised head flags per sorted
    position."""
    rng = np.random.default_rng(seed)
    perm = rng.permutation(m).astype(np.int64)
    head = np.zeros(m, dtype=bool)
    if m:
        head[0] = True
    if pattern == "each":
        head[:] = True
    elif pattern == "random5":
        head |= rng.random(m) < 0.2
    elif pattern == "span":
        if m >= 3 * T + 3:
            # one segment across two whole tiles, length-1 neighbours
            heads = [T - 3, T - 2, T - 1, 3 * T, 3 * T + 1, 3 * T + 2]
        else:
            heads = [1, 2, m - 3, m - 2, m - 1]
        for h in heads:
            if 0 < h < m:
                head[h] = True
    elif pattern == "aligned":
        # heads exactly on every tile border, and one on a tile's last row
        head[::T] = True
        k = max(1, (m // T) // 2)
        if 0 < T * k - 1 < m:
            head[T * k - 1] = True
    return perm, head


def raw_flags(head):
    """What a careless caller passes: position 0 unflagged. The op has to
    repair it."""
    h = head.copy()
    if h.size:
        h[0] = False
    return h


def make_values(m, dtype, seed, perm):
    """Values in ORIGINAL row order (make_values of test_window.py). Float
    specials sit in the second half of the sorted order, so the first half
    keeps finite sums."""
    rng = np.random.default_rng(seed + 1000)
    if dtype == "bool":
        vs = rng.random(m) < 0.5
    elif dtype == "int64":
        ext = np.array([I64.max, I64.max - 1, I64.min, I64.min + 1, 0, 7,
                        -9], dtype=np.int64)
        vs = ext[rng.integers(0, len(ext), m)]
    elif dtype.startswith("int"):
        ii = np.iinfo(NP_DTYPE[dtype])
        vs = rng.integers(ii.min, int(ii.max) + 1, m).astype(NP_DTYPE[dtype])
    else:
        vs = (rng.integers(-200, 200, m) / 4.0).astype(NP_DTYPE[dtype])
        if m:
            for x in (0.0, -0.0):
                vs[rng.integers(0, m, max(1, m // 16))] = x
            half = m // 2
            if m - half > 3:
                for x in (np.nan, np.inf, -np.inf):
                    vs[rng.integers(half, m, max(1, m // 200))] = x
    out = np.empty_like(vs)
    out[perm] = vs
    return out


def make_valid(m, pattern, head, perm, seed):
    if pattern == "none":
        return None
    rng = np.random.default_rng(seed + 3000)
    vs = np.ones(m, dtype=bool)
    heads = np.flatnonzero(head)
    ends = np.append(heads[1:], m)
    if pattern == "all":
        vs[:] = False
    elif pattern == "interior":
        vs &= rng.random(m) >= 0.3
    elif pattern == "segment" and len(heads):
        k = len(heads) // 2
        vs[heads[k]:ends[k]] = False
    out = np.empty(m, dtype=bool)
    out[perm] = vs
    return out


def general_floats(m, seed, perm):
    rng = np.random.default_rng(seed + 2000)
    vs = rng.standard_normal(m) * 1e6
    if m:
        vs[rng.integers(0, m, 5)] = 1e12
    out = np.empty_like(vs)
    out[perm] = vs
    return out


# ---------------------------------------------------------------------------
# loop oracle
# ---------------------------------------------------------------------------

def _greater(a, b):
    """a > b in Spark's order: NaN is greater than everything, equal to
    itself."""
    if a != a:
        return b == b
    if b != b:
        return False
    return a > b


def _wrap64(x):
    return (x + (1 << 63)) % (1 << 64) - (1 << 63)


def _float_sum(xs):
    nan = any(x != x for x in xs)
    pinf = any(x == math.inf for x in xs)
    ninf = any(x == -math.inf for x in xs)
    if nan or (pinf and ninf):
        return math.nan
    if pinf:
        return math.inf
    if ninf:
        return -math.inf
    return math.fsum(xs)


def oracle_loop(perm, head, funcs):
    """funcs: (fn, values or None, valid or None) with numpy values in
    original row order. Returns (first_rows, per function (data, valid,
    bound), count): lists with one entry per segment; bound is the allowed
    |error|."""
    m = len(perm)
    heads = [i for i in range(m) if head[i]]
    ends = heads[1:] + [m]
    permL = perm.tolist()
    first = [permL[h] for h in heads]
    results = []
    for fn, values, valid in funcs:
        vs = values.tolist() if values is not None else None
        vl = valid.tolist() if valid is not None else None
        is_float = values is not None and values.dtype.kind == "f"
        data, ok, bound = [], [], []
        for h, e in zip(heads, ends):
            rows = [r for r in permL[h:e] if vl is None or vl[r]]
            cnt = len(rows)
            b = 0.0
            if fn == "count":
                val = cnt
            elif cnt == 0:
                val = 0
            elif fn in ("min", "max"):
                val = vs[rows[0]]
                for r in rows[1:]:
                    x = vs[r]
                    if fn == "max" and _greater(x, val):
                        val = x
                    elif fn == "min" and _greater(val, x):
                        val = x
            elif is_float or fn == "avg":
                xs = [float(vs[r]) for r in rows]
                val = _float_sum(xs)
                sabs = math.fsum(abs(x) for x in xs if math.isfinite(x))
                b = cnt * 2.0 ** -52 * sabs
                if fn == "avg":
                    val = val / cnt
                    ulp = math.ulp(val) if math.isfinite(val) else 0.0
                    b = b / cnt + ulp
            else:
                val = _wrap64(sum(int(vs[r]) for r in rows))
            data.append(val)
            ok.append(cnt > 0)
            bound.append(b)
        nullable = fn != "count" and valid is not None
        results.append((data, ok if nullable else None, bound))
    return first, results, len(heads)


# ---------------------------------------------------------------------------
# numpy oracle (finite values whose sums are exact; integer min / max)
# ---------------------------------------------------------------------------

def oracle_numpy(perm, head, funcs):
    m = len(perm)
    heads = np.flatnonzero(head)
    first = perm[heads]
    results = []
    for fn, values, valid in funcs:
        vl = valid[perm] if valid is not None else np.ones(m, dtype=bool)
        cnt = np.add.reduceat(vl.astype(np.int64), heads)
        if fn == "count":
            results.append((cnt, None))
            continue
        vs = values[perm]
        if fn in ("sum", "avg"):
            wide = np.float64 if (fn == "avg" or vs.dtype.kind == "f") \
                else np.int64
            x = np.where(vl, vs.astype(wide), wide(0))
            with np.errstate(over="ignore"):
                res = np.add.reduceat(x, heads)
            if fn == "avg":
                res = res / np.maximum(cnt, 1)
        else:
            ii = np.iinfo(np.int64)
            x = np.where(vl, vs.astype(np.int64),
                         ii.max if fn == "min" else ii.min)
            red = np.minimum if fn == "min" else np.maximum
            res = red.reduceat(x, heads)
        res = np.where(cnt > 0, res, np.zeros_like(res))
        if fn in ("min", "max"):
            res = res.astype(values.dtype)
        results.append((res, cnt > 0 if valid is not None else None))
    return first, results, len(heads)


# ---------------------------------------------------------------------------
# running the op and comparing
# ---------------------------------------------------------------------------

def to_torch(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)) \
        .to(dev)


def run_op(dev, perm, head, funcs, raw=True, num_segments="exact",
           use_perm=True):
    tensors = {}

    def tt(a):
        if a is None:
            return None
        if id(a) not in tensors:
            tensors[id(a)] = to_torch(a, dev)
        return tensors[id(a)]

    specs = [(fn, tt(v), tt(vl)) for fn, v, vl in funcs]
    k = int(head.sum()) if num_segments == "exact" else num_segments
    first, res, count = SG.segmented_reduce_tensors(
        to_torch(raw_flags(head) if raw else head, dev), specs,
        to_torch(perm, dev) if use_perm else None, num_segments=k)
    assert count.dtype == torch.int64 and tuple(count.shape) == (1,)
    assert first.dtype == torch.int64
    return (first.cpu(), [(d.cpu(), None if v is None else v.cpu())
                          for d, v in res], int(count.cpu()[0]))


def _same_float(got, want):
    if want != want:
        return got != got
    return got == want


def compare(got, want, funcs, exact_float_sum=True, rows=None):
    """rows: compare the first `rows` segments only (outputs may be longer
    or the oracle's lists longer)."""
    gfirst, gres, gcount = got
    wfirst, wres, wcount = want
    assert gcount == wcount
    n = wcount if rows is None else rows
    assert gfirst[:n].tolist() == [int(x) for x in wfirst[:n]]
    if rows is None:
        assert len(gfirst) == n
    assert len(gres) == len(wres) == len(funcs)
    for k, ((gd, gv), w, (fn, values, valid)) in enumerate(
            zip(gres, wres, funcs)):
        wd, wv = w[0], w[1]
        bound = w[2] if len(w) > 2 else None
        what = f"funcs[{k}] = {fn}"
        if fn == "count":
            assert gd.dtype == torch.int64, what
        elif fn == "avg":
            assert gd.dtype == torch.float64, what
        elif fn == "sum":
            assert gd.dtype == (torch.float64 if values.dtype.kind == "f"
                                else torch.int64), what
        else:
            assert gd.dtype == to_torch(values[:0], "cpu").dtype, what
        if rows is None:
            assert len(gd) == n, what
        if wv is None:
            assert gv is None, what
        else:
            assert gv is not None and gv.dtype == torch.bool, what
            assert gv[:n].tolist() == [bool(x) for x in wv[:n]], what
        g = gd[:n].tolist()
        wl = (wd.tolist() if isinstance(wd, np.ndarray) else wd)[:n]
        if gd.dtype.is_floating_point:
            loose = fn == "avg" or (fn == "sum" and not exact_float_sum)
            for r, (a, b) in enumerate(zip(g, wl)):
                if loose and bound is not None and math.isfinite(b):
                    assert abs(a - b) <= bound[r], (what, r, a, b, bound[r])
                else:
                    assert _same_float(a, float(b)), (what, r, a, b)
        else:
            assert g == [int(x) for x in wl], what


def all_funcs(values, valid):
    funcs = [("count", None, None)]
    funcs += [(fn, values, valid) for fn in FNS]
    return funcs


@functools.lru_cache(maxsize=None)
def grid_case(m, pattern, null_pat, dtype):
    """Inputs and the loop oracle's answer, computed once and shared by the
    CPU and GPU tests."""
    seed = 19 * m + 7 * PATTERNS.index(pattern)
    perm, head = make_structure(m, pattern, seed)
    values = make_values(m, dtype, seed, perm)
    valid = make_valid(m, null_pat, head, perm, seed)
    funcs = all_funcs(values, valid)
    return perm, head, funcs, oracle_loop(perm, head, funcs)


def _rotation(m, pattern):
    """Null pattern and dtype of a (size, pattern) cell: the grid as a whole
    covers each of them many times."""
    k = SIZES.index(m) * len(PATTERNS) + PATTERNS.index(pattern)
    return NULLS[k % 4], DTYPES[k % 7]


def _run_grid(dev, m, pattern):
    perm, head, funcs, want = grid_case(m, pattern, *_rotation(m, pattern))
    compare(run_op(dev, perm, head, funcs), want, funcs)


def _run_dtype(dev, dtype, null_pat):
    perm, head, funcs, want = grid_case(T + 1, "random5", null_pat, dtype)
    compare(run_op(dev, perm, head, funcs), want, funcs)


@functools.lru_cache(maxsize=None)
def general_case(pattern):
    m = 3 * T + 7
    perm, head = make_structure(m, pattern, 31)
    values = general_floats(m, 31, perm)
    valid = make_valid(m, "interior", head, perm, 31)
    funcs = [("sum", values, valid), ("avg", values, valid),
             ("sum", values, None)]
    return perm, head, funcs, oracle_loop(perm, head, funcs)


def _run_general(dev, pattern):
    perm, head, funcs, want = general_case(pattern)
    got = run_op(dev, perm, head, funcs)
    compare(got, want, funcs, exact_float_sum=False)
    return got


def _run_identity_perm(dev):
    """perm=None is the identity order."""
    m = T + 1
    _perm, head = make_structure(m, "random5", 43)
    ident = np.arange(m, dtype=np.int64)
    values = make_values(m, "float64", 43, ident)
    valid = make_valid(m, "interior", head, ident, 43)
    funcs = all_funcs(values, valid)
    want = oracle_loop(ident, head, funcs)
    a = run_op(dev, ident, head, funcs, use_perm=False)
    b = run_op(dev, ident, head, funcs, use_perm=True)
    compare(a, want, funcs)
    compare(b, want, funcs)
    assert torch.equal(a[0], b[0])
    for (da, va), (db, vb) in zip(a[1], b[1]):
        # bitwise: NaNs compare unequal under torch.equal
        assert torch.equal(da.view(torch.uint8), db.view(torch.uint8))
        assert (va is None and vb is None) or torch.equal(va, vb)


def _run_strided(dev):
    """A value column that is every other element of a buffer, a validity
    that starts one byte into its buffer, and flags sliced the same way."""
    m = T + 1
    perm, head = make_structure(m, "random5", 41)
    values = make_values(m, "int32", 41, perm)
    valid = make_valid(m, "interior", head, perm, 41)
    funcs = [("sum", values, valid), ("max", values, valid),
             ("count", values, valid)]
    want = oracle_loop(perm, head, funcs)
    buf = torch.zeros(2 * m + 1, dtype=torch.int32, device=dev)
    v = buf[1::2]
    v.copy_(to_torch(values, dev))
    assert not v.is_contiguous()
    vbuf = torch.zeros(m + 1, dtype=torch.bool, device=dev)
    vl = vbuf[1:]
    vl.copy_(to_torch(valid, dev))
    hbuf = torch.zeros(m + 3, dtype=torch.uint8, device=dev)
    hbuf[3:] = to_torch(raw_flags(head), dev).to(torch.uint8) * 7
    first, res, count = SG.segmented_reduce_tensors(
        hbuf[3:], [("sum", v, vl), ("max", v, vl), ("count", v, vl)],
        to_torch(perm, dev), num_segments=want[2])
    compare((first.cpu(), [(d.cpu(), None if o is None else o.cpu())
                           for d, o in res], int(count.cpu()[0])),
            want, funcs)


def _run_nine_funcs(dev):
    """More than SEG_MAX_FUNCS functions: two kernel calls."""
    m = T + 1
    perm, head = make_structure(m, "random5", 47)
    vi = make_values(m, "int16", 47, perm)
    vf = make_values(m, "float32", 48, perm)
    valid = make_valid(m, "interior", head, perm, 47)
    funcs = [(fn, vi, valid) for fn in FNS] + \
        [(fn, vf, None) for fn in FNS[1:]]
    assert len(funcs) == SG.SEG_MAX_FUNCS + 1
    compare(run_op(dev, perm, head, funcs), oracle_loop(perm, head, funcs),
            funcs)


def _run_num_segments(dev):
    m = 3 * T + 7
    perm, head, funcs, want = grid_case(m, "random5", "interior", "int32")
    total = want[2]
    # the upper bound: one row per input row, rows beyond count unspecified
    got = run_op(dev, perm, head, funcs, num_segments=None)
    assert len(got[0]) == m and all(len(d) == m for d, _v in got[1])
    compare(got, want, funcs, rows=total)
    # one short: the first total - 1 segments, and the true total
    got = run_op(dev, perm, head, funcs, num_segments=total - 1)
    assert len(got[0]) == total - 1
    assert all(len(d) == total - 1 for d, _v in got[1])
    compare(got, want, funcs, rows=total - 1)
    # none at all: only the count
    got = run_op(dev, perm, head, funcs, num_segments=0)
    assert got[2] == total and len(got[0]) == 0


# -- groupby_tensors ----------------------------------------------------------

_NULL = ("null",)
_NAN = ("nan",)


def _norm(x, ok):
    if not ok:
        return _NULL
    if isinstance(x, float):
        if x != x:
            return _NAN
        if x == 0.0:
            return 0.0
    return x


def _key_order(t):
    """Ascending, nulls first, NaN last."""
    return tuple((0, 0) if x is _NULL else (2, 0) if x is _NAN else (1, x)
                 for x in t)


def oracle_groupby(keys, valids, values, valid):
    """Groups in ascending key order: (first row, count(*), count, wrapped
    integer sum or exact float sum, min, max) of `values` per group."""
    n = len(values)
    groups = {}
    for r in range(n):
        t = tuple(_norm(k[r].item(), vl is None or bool(vl[r]))
                  for k, vl in zip(keys, valids))
        groups.setdefault(t, []).append(r)
    out = []
    for t in sorted(groups, key=_key_order):
        rows = groups[t]
        live = [r for r in rows if valid is None or valid[r]]
        xs = [values[r].item() for r in live]
        if values.dtype.kind == "f":
            total = math.fsum(xs) if xs else 0
        else:
            total = _wrap64(sum(int(x) for x in xs))
        out.append((rows[0], len(rows), len(live), total,
                    min(xs) if xs else 0, max(xs) if xs else 0))
    return out


def _groupby_case(m, which, seed):
    rng = np.random.default_rng(seed)
    values = rng.integers(-1000, 1000, m).astype(np.int64)
    valid = rng.random(m) < 0.8
    key_bits = None
    if which == "one":
        keys = [rng.integers(-5, 6, m).astype(np.int32)]
        valids = [None]
    elif which == "three":
        keys = [rng.integers(0, 3, m).astype(np.int64),
                rng.integers(0, 1000, m).astype(np.int32) % 4,
                rng.integers(0, 2, m).astype(np.int8)]
        valids = [None, rng.random(m) < 0.7, None]
        key_bits = [2, 10, 1]
    else:  # a nullable float64 key with NaN and both zeros
        pool = np.array([np.nan, 0.0, -0.0, 1.5, -2.25, np.inf, -np.inf])
        keys = [pool[rng.integers(0, len(pool), m)]]
        valids = [rng.random(m) < 0.8]
        values = (rng.integers(-200, 200, m) / 4.0)
    return keys, valids, key_bits, values, valid


def _run_groupby(dev, m, which):
    keys, valids, key_bits, values, valid = _groupby_case(m, which, 50 + m)
    want = oracle_groupby(keys, valids, values, valid)
    tv, tvl = to_torch(values, dev), to_torch(valid, dev)
    first, res, ng = SG.groupby_tensors(
        [to_torch(k, dev) for k in keys],
        [("count", None, None), ("count", tv, tvl), ("sum", tv, tvl),
         ("min", tv, tvl), ("max", tv, tvl)],
        [to_torch(v, dev) for v in valids], key_bits)
    assert isinstance(ng, int) and ng == len(want)
    assert first.tolist() == [w[0] for w in want]  # key order, first rows
    for k in range(5):
        assert res[k][0].tolist() == [w[k + 1] for w in want], k
        assert len(res[k][0]) == ng
    assert res[0][1] is None and res[1][1] is None
    for k in (2, 3, 4):
        assert res[k][1].tolist() == [w[2] > 0 for w in want]


def _run_groupby_edges(dev):
    v = torch.arange(10, dtype=torch.int32, device=dev)
    ok = (v % 3 != 0)
    # no key: one global group, no sort
    first, res, ng = SG.groupby_tensors([], [("sum", v, ok),
                                             ("count", None, None),
                                             ("min", v, None)])
    assert ng == 1 and first.tolist() == [0]
    assert res[0][0].tolist() == [1 + 2 + 4 + 5 + 7 + 8]
    assert res[0][1].tolist() == [True]
    assert res[1][0].tolist() == [10] and res[2][0].tolist() == [0]
    assert res[2][0].dtype == torch.int32
    # no rows: no groups, with and without keys
    e = v[:0]
    for keys in ([], [e]):
        first, res, ng = SG.groupby_tensors(keys, [("sum", e, ok[:0]),
                                                   ("max", e, None)])
        assert ng == 0 and first.numel() == 0
        assert [d.numel() for d, _ in res] == [0, 0]
        assert res[0][0].dtype == torch.int64
        assert res[0][1].dtype == torch.bool and res[1][1] is None
    with pytest.raises(ValueError, match="key or a value"):
        SG.groupby_tensors([], [("count", None, None)])


# ---------------------------------------------------------------------------
# CPU tier: the oracles against each other, the twin, argument checking
# ---------------------------------------------------------------------------

def test_constants_mirror_the_native_header():
    g = _native.gpu()  # the extension loads without a GPU
    assert (g.SEG_MAX_FUNCS, g.SEG_SMALL_ROWS, g.SEG_TILE_ROWS,
            g.SEG_CARRY_CHUNK) == (SG.SEG_MAX_FUNCS, S, T, SG.CARRY_CHUNK)
    assert g.seg_reduce_work_bytes(S, 3) == 0
    assert g.seg_reduce_work_bytes(S + 1, 3) > 0
    assert SG.seg_reduce_work_bytes(S + 1, 3) == \
        g.seg_reduce_work_bytes(S + 1, 3)


def _numpy_case(m, pattern, seed):
    perm, head = make_structure(m, pattern, seed)
    rng = np.random.default_rng(seed)
    vi = rng.integers(-2 ** 31, 2 ** 31, m).astype(np.int32)
    v64 = rng.integers(-2 ** 62, 2 ** 62, m).astype(np.int64)
    vf = (rng.integers(-200, 200, m) / 4.0).astype(np.float64)
    valid = make_valid(m, "interior", head, perm, seed)
    funcs = [("count", None, None), ("count", vi, valid), ("sum", v64, valid),
             ("sum", vf, valid), ("sum", vf, None), ("min", vi, valid),
             ("max", vi, valid), ("avg", vf, valid), ("max", v64, None)]
    return perm, head, funcs


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("m", [1, 65, T + 1])
def test_numpy_oracle_matches_loop_oracle(m, pattern):
    perm, head, funcs = _numpy_case(m, pattern, 61 + m)
    lfirst, loop, lcount = oracle_loop(perm, head, funcs)
    vfirst, vec, vcount = oracle_numpy(perm, head, funcs)
    assert lcount == vcount and vfirst.tolist() == lfirst
    for (ld, lv, _b), (vd, vv) in zip(loop, vec):
        assert vd.tolist() == ld
        assert (None if vv is None else vv.tolist()) == lv


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("m", SIZES)
def test_cpu_twin_grid(m, pattern):
    _run_grid("cpu", m, pattern)


@pytest.mark.parametrize("null_pat", NULLS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_cpu_twin_dtypes_and_nulls(dtype, null_pat):
    _run_dtype("cpu", dtype, null_pat)


@pytest.mark.parametrize("pattern", ["one", "random5"])
def test_cpu_twin_general_float_sums(pattern):
    _run_general("cpu", pattern)


def test_cpu_twin_identity_perm():
    _run_identity_perm("cpu")


def test_cpu_twin_strided_inputs():
    _run_strided("cpu")


def test_cpu_twin_nine_functions():
    _run_nine_funcs("cpu")


def test_cpu_twin_num_segments():
    _run_num_segments("cpu")


@pytest.mark.parametrize("which", ["one", "three", "float"])
@pytest.mark.parametrize("m", [1, 65, S + 1, 3 * T + 7])
def test_cpu_groupby_tensors(m, which):
    _run_groupby("cpu", m, which)


def test_cpu_groupby_tensors_edges():
    _run_groupby_edges("cpu")


def test_empty_input():
    eb = torch.empty(0, dtype=torch.bool)
    v = torch.empty(0, dtype=torch.float32)
    first, out, count = SG.segmented_reduce_tensors(
        eb, [("count", None, None), ("sum", v, eb), ("min", v, None)])
    assert first.numel() == 0 and count.tolist() == [0]
    assert [d.dtype for d, _ in out] == [torch.int64, torch.float64,
                                         torch.float32]
    assert [d.numel() for d, _ in out] == [0, 0, 0]
    assert out[0][1] is None and out[2][1] is None
    assert out[1][1].dtype == torch.bool and out[1][1].numel() == 0


def test_argument_validation():
    m = 8
    perm = torch.arange(m)
    head = torch.zeros(m, dtype=torch.bool)
    v = torch.arange(m, dtype=torch.int32)
    ok = torch.ones(m, dtype=torch.bool)
    good = ("sum", v, ok)
    R = SG.segmented_reduce_tensors
    with pytest.raises(TypeError, match="head_flags"):
        R(head.to(torch.int32), [good])
    with pytest.raises(ValueError, match="head_flags"):
        R(head.view(2, 4), [good])
    with pytest.raises(TypeError, match="perm"):
        R(head, [good], perm.to(torch.int32))
    with pytest.raises(ValueError, match="perm"):
        R(head, [good], perm[:-1])
    with pytest.raises(TypeError, match="num_segments"):
        R(head, [good], perm, num_segments=2.0)
    with pytest.raises(ValueError, match="num_segments"):
        R(head, [good], perm, num_segments=m + 1)
    with pytest.raises(ValueError, match="num_segments"):
        R(head, [good], perm, num_segments=-1)
    with pytest.raises(ValueError, match=r"funcs\[1\].*unknown function"):
        R(head, [good, ("median", v, None)])
    with pytest.raises(ValueError, match=r"funcs\[0\].*needs values"):
        R(head, [("min", None, None)])
    with pytest.raises(TypeError, match=r"funcs\[1\].*dtype"):
        R(head, [good, ("sum", v.to(torch.float16), None)])
    with pytest.raises(ValueError, match=r"funcs\[1\].*1-D"):
        R(head, [good, ("sum", v.view(2, 4), None)])
    with pytest.raises(ValueError, match=r"funcs\[1\].*rows"):
        R(head, [good, ("sum", v[:-1], None)])
    with pytest.raises(TypeError, match=r"funcs\[1\].*valid"):
        R(head, [good, ("sum", v, ok.to(torch.int32))])
    with pytest.raises(ValueError, match=r"funcs\[1\].*valid"):
        R(head, [good, ("sum", v, ok[:-1])])
    with pytest.raises(ValueError, match=r"funcs\[0\]"):
        R(head, [("sum", v)])
    if torch.cuda.is_available():
        with pytest.raises(ValueError, match=r"funcs\[0\].*devices"):
            R(head, [("sum", v.cuda(), None)])
        with pytest.raises(ValueError, match="perm.*devices"):
            R(head, [good], perm.cuda())


@pytest.mark.parametrize("fn", ["rank", "dense_rank"])
def test_ranking_functions_are_unknown(fn):
    """The window's ranking functions share the kernels' code table but are
    no segmented reduce."""
    head = torch.zeros(8, dtype=torch.bool)
    with pytest.raises(ValueError, match="unknown function"):
        SG.segmented_reduce_tensors(head, [(fn, None, None)])


@pytest.mark.parametrize("code", [0, 1, 2])  # row_number, rank, dense_rank
def test_binding_rejects_ranking_function_codes(code):
    """The binding refuses a ranking code before anything is launched. Every
    pointer is a real buffer of the 8-row call it describes."""
    dev = "cuda" if torch.cuda.is_available() else "cpu"
    m = 8
    head = torch.zeros(m, dtype=torch.bool, device=dev)
    v = torch.arange(m, dtype=torch.int64, device=dev)
    ok = torch.ones(m, dtype=torch.bool, device=dev)
    out = torch.full((m,), -7, dtype=torch.int64, device=dev)
    ov = torch.zeros(m, dtype=torch.bool, device=dev)
    first = torch.full((m,), -7, dtype=torch.int64, device=dev)
    count = torch.full((1,), -7, dtype=torch.int64, device=dev)
    g = _native.gpu()
    assert g.seg_reduce_work_bytes(m, 1) == 0
    desc = (code, 0, 2, 8, 1, v.data_ptr(), ok.data_ptr(), out.data_ptr(),
            ov.data_ptr())
    with pytest.raises(ValueError, match=r"seg_reduce: funcs\[0\]: unknown "
                                         "function"):
        g.seg_reduce([desc], 0, head.data_ptr(), m, m, m, first.data_ptr(),
                     count.data_ptr(), 0, _native.current_stream()
                     if dev == "cuda" else 0)
    # nothing ran
    assert out.tolist() == [-7] * m and first.tolist() == [-7] * m
    assert count.tolist() == [-7]


# ---------------------------------------------------------------------------
# GPU tier
# ---------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("m", SIZES)
def test_gpu_grid(m, pattern):
    _run_grid("cuda", m, pattern)


@pytest.mark.gpu
@pytest.mark.parametrize("null_pat", NULLS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_gpu_dtypes_and_nulls(dtype, null_pat):
    _run_dtype("cuda", dtype, null_pat)


@pytest.mark.gpu
@pytest.mark.parametrize("pattern", ["one", "random5"])
def test_gpu_general_float_sums(pattern):
    _run_general("cuda", pattern)


@pytest.mark.gpu
def test_gpu_float_sums_are_deterministic():
    a = _run_general("cuda", "random5")
    b = _run_general("cuda", "random5")
    for (da, va), (db, vb) in zip(a[1], b[1]):
        assert torch.equal(da, db)
        assert (va is None and vb is None) or torch.equal(va, vb)


@pytest.mark.gpu
def test_gpu_identity_perm():
    _run_identity_perm("cuda")


@pytest.mark.gpu
def test_gpu_strided_inputs():
    _run_strided("cuda")


@pytest.mark.gpu
def test_gpu_nine_functions():
    _run_nine_funcs("cuda")


@pytest.mark.gpu
def test_gpu_num_segments():
    _run_num_segments("cuda")


@pytest.mark.gpu
@pytest.mark.parametrize("pattern", ["one", "random5", "span"])
def test_gpu_carry_scan_takes_two_chunks(pattern):
    """Vectorised oracle only. `span` keeps one segment open across the
    chunk border of the carry scan."""
    m = TWO_CHUNKS
    perm, head, funcs = _numpy_case(m, pattern, 81)
    if pattern == "span":
        head[:] = False
        head[[0, T - 1, m - 2]] = True
    wfirst, want, wcount = oracle_numpy(perm, head, funcs)
    gfirst, got, gcount = run_op("cuda", perm, head, funcs)
    assert gcount == wcount
    assert torch.equal(gfirst, torch.from_numpy(wfirst))
    for k, ((gd, gv), (wd, wv)) in enumerate(zip(got, want)):
        assert torch.equal(gd, torch.from_numpy(wd)), (k, funcs[k][0])
        assert (gv is None) == (wv is None)
        if wv is not None:
            assert torch.equal(gv, torch.from_numpy(wv)), k


@pytest.mark.gpu
def test_runs_under_stream_capture():
    m = T + 1
    dev = "cuda"

    def case(seed):
        perm, head = make_structure(m, "random5", seed)
        values = make_values(m, "float64", seed, perm)
        valid = make_valid(m, "interior", head, perm, seed)
        return perm, head, values, valid

    def specs(v, vl):
        return [("count", None, None), ("sum", v, vl), ("max", v, vl),
                ("avg", v, vl)]

    perm, head, values, valid = case(91)
    perm2, head2, values2, valid2 = case(92)
    funcs2 = specs(values2, valid2)
    want2 = oracle_loop(perm2, head2, funcs2)
    tp, th = to_torch(perm, dev), to_torch(raw_flags(head), dev)
    tv, tvl = to_torch(values, dev), to_torch(valid, dev)
    SG.segmented_reduce_tensors(th, specs(tv, tvl), tp)  # warm up
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            first, out, count = SG.segmented_reduce_tensors(
                th, specs(tv, tvl), tp)
    torch.cuda.current_stream().wait_stream(side)
    for dst, src in ((tp, perm2), (th, raw_flags(head2)), (tv, values2),
                     (tvl, valid2)):
        dst.copy_(to_torch(src, dev))
    graph.replay()
    torch.cuda.synchronize()
    got = (first.cpu(), [(d.cpu(), None if v is None else v.cpu())
                         for d, v in out], int(count.cpu()[0]))
    compare(got, want2, funcs2, rows=want2[2])
    direct = SG.segmented_reduce_tensors(th, specs(tv, tvl), tp)
    n = want2[2]
    assert torch.equal(direct[2], count)
    assert torch.equal(direct[0][:n], first[:n])
    for (da, va), (db, vb) in zip(direct[1], out):
        assert torch.equal(da[:n].view(torch.uint8), db[:n].view(torch.uint8))


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["one", "three", "float"])
@pytest.mark.parametrize("m", [1, 65, S + 1, 3 * T + 7])
def test_gpu_groupby_tensors(m, which):
    _run_groupby("cuda", m, which)


@pytest.mark.gpu
def test_gpu_groupby_tensors_edges():
    _run_groupby_edges("cuda")


def _sorted_rows(keys, results):
    cols = [c.to_pylist() for c in keys.columns] + \
        [c.to_pylist() for c in results]
    rows = list(zip(*cols))
    return sorted(rows, key=lambda r: tuple(
        (0, 0) if x is None else (1, x) for x in r[:keys.num_columns]))


@pytest.mark.gpu
@pytest.mark.parametrize("n", [65, 3 * T + 7])
def test_gpu_groupby_sorted_matches_hash_groupby(n):
    """The new kernels against the round-1 hash table on the same input:
    integer aggregates and quarter-integer float sums, so both are exact."""
    from spark_rapids_jni_amd.ops.aggregate import (Agg, groupby,
                                                    groupby_sorted)
    rng = np.random.default_rng(101 + n)
    dev = "cuda"

    def col(vals, dt, nulls=None):
        vals = vals.tolist()
        if nulls is not None:
            vals = [None if z else x for x, z in zip(vals, nulls)]
        return Column.from_pylist(vals, dt, dev)

    k1 = col(rng.integers(-3, 4, n), DType.INT32, rng.random(n) < 0.2)
    k2 = col(rng.integers(0, 3, n), DType.INT64)
    vi = col(rng.integers(-1000, 1000, n), DType.INT32, rng.random(n) < 0.3)
    vf = col(rng.integers(-200, 200, n) / 4.0, DType.FLOAT64,
             rng.random(n) < 0.3)
    vn = col(rng.integers(-5, 5, n), DType.INT64)
    aggs = [(Agg.COUNT_ALL, None), (Agg.COUNT_VALID, vi), (Agg.SUM, vi),
            (Agg.SUM, vf), (Agg.MIN, vi), (Agg.MAX, vi), (Agg.SUM, vn),
            (Agg.MIN, vf)]
    for keys in ([k2], [k1, k2]):
        hk, hr = groupby(Table(keys), aggs)
        sk, sr = groupby_sorted(Table(keys), aggs)
        assert [c.dtype for c in sr] == [c.dtype for c in hr]
        assert [c.dtype for c in sk.columns] == [c.dtype for c in hk.columns]
        assert _sorted_rows(sk, sr) == _sorted_rows(hk, hr)
        # the sorted path's own order is the key order already
        got = list(zip(*[c.to_pylist() for c in sk.columns]))
        assert got == [r[:len(keys)] for r in _sorted_rows(sk, sr)]
    # an all-null group gives null results
    k = Column.from_pylist([1, 1, 2], DType.INT32, dev)
    v = Column.from_pylist([None, None, 5], DType.INT64, dev)
    sk, sr = groupby_sorted([k], [(Agg.SUM, v), (Agg.COUNT_VALID, v)])
    assert sk.columns[0].to_pylist() == [1, 2]
    assert sr[0].to_pylist() == [None, 5] and sr[1].to_pylist() == [0, 1]


@pytest.mark.gpu
def test_gpu_groupby_sorted_decimal128_keys():
    from spark_rapids_jni_amd.ops.aggregate import Agg, groupby_sorted
    big = 1 << 64
    d128 = [(-3 * big + 5, -big, -1, 0, big + 1)[i % 5] for i in range(40)]
    d128 = [None if i % 11 == 0 else x for i, x in enumerate(d128)]
    vals = list(range(40))
    kc = Column.from_pylist(d128, DType.DECIMAL128, "cuda", scale=2)
    vc = Column.from_pylist(vals, DType.INT64, "cuda")
    sk, sr = groupby_sorted([kc], [(Agg.SUM, vc), (Agg.COUNT_ALL, None)])
    want = {}
    for k, v in zip(d128, vals):
        s, c = want.get(k, (0, 0))
        want[k] = (s + v, c + 1)
    order = sorted(want, key=lambda k: (0, 0) if k is None else (1, k))
    assert sk.columns[0].to_pylist() == order
    assert sr[0].to_pylist() == [want[k][0] for k in order]
    assert sr[1].to_pylist() == [want[k][1] for k in order]
