"""Rolling window functions (ops/window.py, src/gpu/window_rolling.hip): lag,
lead and count/sum/min/max/avg over bounded ROWS frames; the native kernel
and its CPU twin against a loop oracle that uses neither the op nor a torch
scan.

The ORACLE walks the sorted positions in plain Python. A float sum is the
left-to-right float64 sum of the frame's valid values from +0.0, avg is one
float64 division of that sum by the count, min and max use an explicit
NaN-greatest comparison in which, of equal values (-0.0 and 0.0), the later
one of the frame wins - the one choice the comparison leaves open, taken as
seg_scan.hpp's seg_max_f / seg_min_f take it.

Everything is compared EXACTLY, general float sums and avg included: NaN as
NaN-ness (IEEE 754 does not fix the sign and payload of the NaN that
inf + -inf makes, and hosts and the GPU differ in it), everything else as
bits, validity and the zero data word under a null included. No tolerance
appears anywhere.
"""
import functools

import numpy as np
import pytest
import torch

from spark_rapids_jni_amd import _native
from spark_rapids_jni_amd.columnar import Column, DType, Table
from spark_rapids_jni_amd.nds.expr import Val, col
from spark_rapids_jni_amd.nds.plan import (Engine, Frame, Join, Project, Scan,
                                           Window)
from spark_rapids_jni_amd.ops import window as W

R = W.ROLL_TILE_ROWS
H = W.ROLL_MAX_REACH
SIZES = sorted({0, 1, 2, 63, 64, 65, R - 1, R, R + 1, 3 * R + 7})
PARTS = ["one", "each", "random5", "span"]
NULLS = ["none", "all", "interior", "leading"]
DTYPES = ["bool", "int8", "int16", "int32", "int64", "float32", "float64"]
NP_DTYPE = {"bool": np.bool_, "int8": np.int8, "int16": np.int16,
            "int32": np.int32, "int64": np.int64, "float32": np.float32,
            "float64": np.float64}
AGGS = ("count", "sum", "min", "max", "avg")
SHIFTS = ("lag", "lead")
SMALL_FRAMES = [(0, 0), (-1, 0), (0, 1), (-1, 1), (-3, -1), (1, 3), (-2, 5)]
I64 = np.iinfo(np.int64)
DIRECT_ENV = "SRJ_WINDOW_ROLLING_DIRECT"


def shift_ks(m):
    return [0, 1, 2, 63, 64, 65, H, H + 1, m, 2 ** 31 - 1, -1, -65]


# ---------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------

def make_structure(m, part_pat, seed):
    """perm (a genuine shuffle) and normalised partition head flags per
    sorted position. `span`: heads on a tile's last three rows and the first
    three rows three tiles on, one long partition between, so frames clip at
    tile edges, halos cross partition heads and a partition outruns a halo."""
    rng = np.random.default_rng(seed)
    perm = rng.permutation(m).astype(np.int64)
    part = np.zeros(m, dtype=bool)
    if m:
        part[0] = True
    if part_pat == "each":
        part[:] = True
    elif part_pat == "random5":
        part |= rng.random(m) < 0.2
    elif part_pat == "span":
        if m >= 3 * R + 3:
            heads = [R - 3, R - 2, R - 1, 3 * R, 3 * R + 1, 3 * R + 2]
        else:
            heads = [1, 2, m - 3, m - 2, m - 1]
        for h in heads:
            if 0 < h < m:
                part[h] = True
    return perm, part


def make_values(m, dtype, seed, perm):
    """Values in ORIGINAL row order: int64 extremes (sums wrap), general
    floats (sums round at every step) with +-0.0 anywhere and NaN, +-inf in
    the second half of the sorted order."""
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
        vs = (rng.standard_normal(m) * 1e6).astype(NP_DTYPE[dtype])
        if m:
            vs[rng.integers(0, m, 3)] = 1e12
            for x in (0.0, -0.0):
                vs[rng.integers(0, m, max(1, m // 8))] = x
            half = m // 2
            if m - half > 3:
                for x in (np.nan, np.inf, -np.inf):
                    vs[rng.integers(half, m, max(1, m // 200))] = x
    out = np.empty_like(vs)
    out[perm] = vs
    return out


def make_valid(m, pattern, part, perm):
    if pattern == "none":
        return None
    vs = np.ones(m, dtype=bool)
    heads = np.flatnonzero(part)
    ends = np.append(heads[1:], m)
    if pattern == "all":
        vs[:] = False
    elif pattern == "interior" and len(heads):
        k = len(heads) // 2
        vs[heads[k]:ends[k]] = False
        vs[m // 3::7] = False
    elif pattern == "leading":
        for h, e in zip(heads, ends):
            vs[h:h + (e - h + 1) // 3] = False
    out = np.empty(m, dtype=bool)
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


def _bounds(part):
    m = len(part)
    ps, pe = [0] * m, [0] * m
    s = 0
    for i in range(m):
        if i == 0 or part[i]:
            s = i
        ps[i] = s
    e = m - 1
    for i in range(m - 1, -1, -1):
        pe[i] = e
        if i == 0 or part[i]:
            e = i - 1
    return ps, pe


def _fold(fn, xs, as_float):
    """(count, value or None) of the frame's valid values xs, in order."""
    cnt = len(xs)
    if fn == "count":
        return cnt, cnt
    if cnt == 0:
        return 0, None
    if fn in ("sum", "avg"):
        if as_float or fn == "avg":
            s = 0.0
            for x in xs:
                s += float(x)
            return cnt, (s / cnt if fn == "avg" else s)
        t = 0
        for x in xs:
            t += int(x)
        return cnt, _wrap64(t)
    acc = xs[0]
    if fn == "max":
        for x in xs[1:]:
            if not _greater(acc, x):
                acc = x
    else:
        for x in xs[1:]:
            if not _greater(x, acc):
                acc = x
    return cnt, acc


def out_np_dtype(fn, values):
    if fn == "count":
        return np.int64
    if fn == "avg":
        return np.float64
    if fn == "sum":
        return np.float64 if values.dtype.kind == "f" else np.int64
    return values.dtype


def nullable(fn, valid, arg):
    if fn in SHIFTS:
        return True
    if fn == "count":
        return False
    return valid is not None or arg[1] > 0 or arg[2] < 0


def oracle(perm, part, funcs):
    """funcs: (fn, values or None, valid or None, ("rows", lo, hi) or k) with
    numpy values in original row order. Returns per function (data, valid or
    None) as numpy arrays in original row order."""
    m = len(perm)
    ps, pe = _bounds(part)
    permL = perm.tolist()
    items = {}  # sorted values with None under a null

    def items_of(values, valid):
        key = (id(values), id(valid))
        if key not in items:
            vs = values[perm].tolist() if values is not None else [1] * m
            if valid is not None:
                vs = [x if ok else None
                      for x, ok in zip(vs, valid[perm].tolist())]
            items[key] = vs
        return items[key]

    data = [[0] * m for _ in funcs]
    oks = [[True] * m for _ in funcs]
    groups = {}
    for n, (fn, values, valid, arg) in enumerate(funcs):
        if fn in SHIFTS:
            its = items_of(values, valid)
            d = -arg if fn == "lag" else arg
            for i in range(m):
                j = i + d
                x = its[j] if ps[i] <= j <= pe[i] else None
                if x is None:
                    oks[n][permL[i]] = False
                else:
                    data[n][permL[i]] = x
        else:
            groups.setdefault((id(values), id(valid), arg), []).append(n)
    for (_v, _vl, arg), members in groups.items():
        _fn, values, valid, _arg = funcs[members[0]]
        its = items_of(values, valid)
        as_float = values is not None and values.dtype.kind == "f"
        lo, hi = arg[1], arg[2]
        for i in range(m):
            a, b = max(i + lo, ps[i]), min(i + hi, pe[i])
            xs = [x for x in its[a:b + 1] if x is not None] if a <= b else []
            r = permL[i]
            for n in members:
                _cnt, val = _fold(funcs[n][0], xs, as_float)
                if val is None:
                    oks[n][r] = False
                else:
                    data[n][r] = val
    out = []
    for n, (fn, values, valid, arg) in enumerate(funcs):
        d = np.array(data[n], dtype=out_np_dtype(fn, values)) if m else \
            np.empty(0, dtype=out_np_dtype(fn, values))
        ok = np.array(oks[n], dtype=bool) if nullable(fn, valid, arg) \
            else None
        out.append((d, ok))
    return out


# ---------------------------------------------------------------------------
# running the op and comparing
# ---------------------------------------------------------------------------

def to_torch(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)) \
        .to(dev)


def run_op(dev, perm, part, funcs, peer=None):
    """The op on raw flags: position 0 unflagged."""
    p = part.copy()
    if p.size:
        p[0] = False
    tensors = {}

    def tt(a):
        if a is None:
            return None
        if id(a) not in tensors:
            tensors[id(a)] = to_torch(a, dev)
        return tensors[id(a)]

    specs = [(fn, tt(v), tt(vl), arg) for fn, v, vl, arg in funcs]
    got = W.window_tensors(to_torch(perm, dev), to_torch(p, dev), specs,
                           to_torch(peer, dev))
    return [(d.cpu().numpy(), None if v is None else v.cpu().numpy())
            for d, v in got]


def _bits(a):
    """NaN as NaN-ness, everything else as bits."""
    a = np.ascontiguousarray(a)
    if a.dtype.kind == "f":
        a = a.copy()
        a[np.isnan(a)] = np.nan
        return a.view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)
    return a


def compare(got, want, funcs, tag=""):
    assert len(got) == len(want) == len(funcs)
    for n, ((gd, gv), (wd, wv), (fn, _v, _vl, arg)) in enumerate(
            zip(got, want, funcs)):
        what = f"{tag}funcs[{n}] = {fn}/{arg}"
        assert gd.dtype == wd.dtype, what
        assert gd.shape == wd.shape, what
        if wv is None:
            assert gv is None, what
        else:
            assert gv is not None and gv.dtype == np.bool_, what
            bad = np.flatnonzero(gv != wv)
            assert bad.size == 0, (what, "valid", int(bad[0]))
        bad = np.flatnonzero(_bits(gd) != _bits(wd))
        assert bad.size == 0, (what, int(bad[0]), gd[bad[0]], wd[bad[0]])


def grid_funcs(m, values, valid):
    """Every frame and every k of the issue. The first 44 stay within
    ROLL_MAX_REACH (staged launches of WINDOW_MAX_FUNCS), the next ten do
    not."""
    fs = []
    for fr in SMALL_FRAMES:
        fs.append(("count", None, None, ("rows",) + fr))
        fs += [(fn, values, valid, ("rows",) + fr) for fn in AGGS]
    fs += [(fn, values, valid, ("rows", -H, H)) for fn in ("sum", "max")]
    fs += [(fn, values, valid, ("rows", -H - 1, 0)) for fn in ("avg", "min")]
    fs += [(fn, values, valid, ("rows", 0, H + 1)) for fn in ("count", "sum")]
    fs += [(fn, values, valid, ("rows", -m - 5, m + 5))
           for fn in ("sum", "max")]
    for k in shift_ks(m):
        fs.append(("lag", values, valid, k))
        fs.append(("lead", values, valid, k))
    return fs


def _rotation(m, part_pat):
    k = SIZES.index(m) * len(PARTS) + PARTS.index(part_pat)
    return DTYPES[k % 7], NULLS[(k // 3) % 4]


@functools.lru_cache(maxsize=None)
def case(m, part_pat, dtype, null_pat):
    """Inputs and the oracle's answer, computed once and shared by the CPU
    and GPU tests."""
    seed = 19 * m + 7 * PARTS.index(part_pat)
    perm, part = make_structure(m, part_pat, seed)
    values = make_values(m, dtype, seed, perm)
    valid = make_valid(m, null_pat, part, perm)
    funcs = grid_funcs(m, values, valid)
    return perm, part, funcs, oracle(perm, part, funcs)


@functools.lru_cache(maxsize=None)
def twin(m, part_pat, dtype, null_pat):
    perm, part, funcs, _want = case(m, part_pat, dtype, null_pat)
    return run_op("cpu", perm, part, funcs)


def _run_case(dev, *key):
    perm, part, funcs, want = case(*key)
    if dev == "cpu":
        compare(twin(*key), want, funcs)
        return
    got = run_op(dev, perm, part, funcs)
    compare(got, want, funcs)
    compare(got, twin(*key), funcs, "GPU == twin: ")


def _raw_equal(a, b):
    """Bit for bit, NaN payloads included."""
    assert len(a) == len(b)
    for n, ((ad, av), (bd, bv)) in enumerate(zip(a, b)):
        assert ad.tobytes() == bd.tobytes(), n
        assert (av is None) == (bv is None), n
        if av is not None:
            assert av.tobytes() == bv.tobytes(), n


# ---------------------------------------------------------------------------
# shared bodies
# ---------------------------------------------------------------------------

F64 = np.float64


def _bits_to_f64(words):
    return np.array(words, dtype=np.uint64).view(F64)


def _run_float_specials(dev):
    """-0.0 and a NaN payload through lag as bits; a frame whose only value
    is -0.0; +-inf. Expected values written out by hand."""
    nz, pz = 0x8000000000000000, 0
    nan = 0x7ff8000000000123
    pinf, ninf = 0x7ff0000000000000, 0xfff0000000000000
    one = 0x3ff0000000000000
    vs = _bits_to_f64([nz, nan, pinf, ninf, pz, nz, one, nz])
    m = len(vs)
    valid = np.array([1, 1, 1, 1, 0, 1, 1, 1], dtype=bool)
    perm = np.arange(m, dtype=np.int64)
    part = np.zeros(m, dtype=bool)
    part[5] = True  # partitions [0, 4] and [5, 7]
    funcs = [("lag", vs, None, 1), ("lead", vs, valid, 1),
             ("sum", vs, valid, ("rows", 0, 0)),
             ("max", vs, valid, ("rows", 0, 0)),
             ("min", vs, valid, ("rows", -1, 0)),
             ("max", vs, valid, ("rows", -1, 0)),
             ("sum", vs, valid, ("rows", -1, 0)),
             ("avg", vs, valid, ("rows", 0, 0))]
    got = run_op(dev, perm, part, funcs)
    compare(got, oracle(perm, part, funcs), funcs)
    lag = got[0][0].view(np.uint64).tolist()
    assert lag == [0, nz, nan, pinf, ninf, 0, nz, one]  # payload, -0.0 kept
    assert got[0][1].tolist() == [False, True, True, True, True, False, True,
                                  True]
    lead = got[1][0].view(np.uint64).tolist()
    assert lead == [nan, pinf, ninf, 0, 0, one, nz, 0]
    assert got[1][1].tolist() == [True, True, True, False, False, True, True,
                                  False]
    # the only value of the frame is -0.0: the sum starts from +0.0, max and
    # min return the value itself
    assert got[2][0].view(np.uint64)[0] == pz and got[2][1][0]
    assert got[3][0].view(np.uint64)[0] == nz and got[3][1][0]
    assert got[7][0].view(np.uint64)[0] == pz and got[7][1][0]
    # the null row's own frame: null, data zero
    assert not got[2][1][4] and got[2][0].view(np.uint64)[4] == 0
    # NaN is greatest; +inf + -inf is NaN; min over (NaN, +inf) is +inf
    assert np.isnan(got[5][0][2]) and got[4][0].view(np.uint64)[2] == pinf
    assert np.isnan(got[6][0][3]) and got[6][1][3]
    # of -0.0 then 1.0 the min is -0.0; of 1.0 then -0.0 the max is 1.0
    assert got[4][0].view(np.uint64)[6] == nz
    assert got[5][0].view(np.uint64)[7] == one


def _run_mixed(dev):
    """Old string-frame functions and new forms interleaved, more than
    WINDOW_MAX_FUNCS of each; results in caller order, the old ones equal to
    a call without the new ones."""
    m = R + 1
    perm, part = make_structure(m, "random5", 23)
    rng = np.random.default_rng(23)
    peer = part | (rng.random(m) < 0.5)
    values = make_values(m, "int32", 23, perm)
    valid = make_valid(m, "leading", part, perm)
    old = [("rank", None, None, "rows"), ("sum", values, valid, "rows"),
           ("max", values, valid, "partition"),
           ("avg", values, valid, "range"), ("count", None, None, "range"),
           ("dense_rank", None, None, "rows"),
           ("min", values, None, "rows"), ("sum", values, None, "partition"),
           ("row_number", None, None, "rows"),
           ("count", values, valid, "partition")]
    new = [("lag", values, valid, 1), ("sum", values, valid, ("rows", -2, 0)),
           ("lead", values, None, 2), ("max", values, valid, ("rows", -3, -1)),
           ("avg", values, None, ("rows", -1, 1)),
           ("count", None, None, ("rows", 0, 3)),
           ("min", values, valid, ("rows", -H - 1, 0)),
           ("lag", values, None, -1), ("sum", values, None, ("rows", 1, 3)),
           ("count", values, valid, ("rows", -H, H))]
    assert min(len(old), len(new)) > W.WINDOW_MAX_FUNCS
    mixed = [f for pair in zip(old, new) for f in pair]
    got = run_op(dev, perm, part, mixed, peer)
    alone = run_op(dev, perm, part, old, peer)
    _raw_equal(got[0::2], alone)
    compare(got[1::2], oracle(perm, part, new), new)


def _run_strided(dev):
    """A value column that is every other element of a buffer and a validity
    that starts one byte into its buffer."""
    m = R + 1
    perm, part = make_structure(m, "random5", 41)
    values = make_values(m, "int32", 41, perm)
    valid = make_valid(m, "leading", part, perm)
    funcs = [("sum", values, valid, ("rows", -2, 1)),
             ("lag", values, valid, 1),
             ("max", values, valid, ("rows", -H - 1, 0))]
    want = oracle(perm, part, funcs)
    buf = torch.zeros(2 * m + 1, dtype=torch.int32, device=dev)
    v = buf[1::2]
    v.copy_(to_torch(values, dev))
    assert not v.is_contiguous()
    vbuf = torch.zeros(m + 1, dtype=torch.bool, device=dev)
    vl = vbuf[1:]
    vl.copy_(to_torch(valid, dev))
    pbuf = torch.zeros(m + 3, dtype=torch.uint8, device=dev)
    pbuf[3:] = to_torch(part, dev).to(torch.uint8) * 7  # nonzero = head
    pbuf[3] = 0
    got = W.window_tensors(to_torch(perm, dev), pbuf[3:],
                           [(fn, v, vl, arg) for fn, _v, _vl, arg in funcs])
    compare([(d.cpu().numpy(), None if o is None else o.cpu().numpy())
             for d, o in got], want, funcs)


def _run_table(dev):
    n = 40
    rng = np.random.default_rng(51)
    pkey = rng.integers(0, 3, n).tolist()
    okey = rng.permutation(n).tolist()  # distinct: the order is total
    vals = rng.integers(-50, 50, n).tolist()
    vals = [None if i % 5 == 1 else x for i, x in enumerate(vals)]
    pcol = Column.from_pylist(pkey, DType.INT32, dev)
    ocol = Column.from_pylist(okey, DType.INT64, dev)
    vcol = Column.from_pylist(vals, DType.INT16, dev)
    out = W.window_columns(
        Table([pcol]), Table([ocol]),
        [("lag", vcol, 1), ("lead", vcol, 2),
         ("sum", vcol, ("rows", -2, 0)), ("max", vcol, ("rows", -3, -1)),
         ("count", vcol, ("rows", -1, 1)), ("avg", vcol, ("rows", 0, 1)),
         ("sum", vcol, "partition")])
    assert [c.dtype for c in out] == [DType.INT16, DType.INT16, DType.INT64,
                                      DType.INT16, DType.INT64, DType.FLOAT64,
                                      DType.INT64]
    want = [[None] * n for _ in range(7)]
    for p in set(pkey):
        rows = sorted((i for i in range(n) if pkey[i] == p),
                      key=lambda i: okey[i])
        for q, i in enumerate(rows):
            def frame(lo, hi):
                sel = rows[max(q + lo, 0):max(q + hi + 1, 0)]
                return [vals[j] for j in sel if vals[j] is not None]
            want[0][i] = vals[rows[q - 1]] if q >= 1 else None
            want[1][i] = vals[rows[q + 2]] if q + 2 < len(rows) else None
            f = frame(-2, 0)
            want[2][i] = sum(f) if f else None
            f = frame(-3, -1)
            want[3][i] = max(f) if f else None
            want[4][i] = len(frame(-1, 1))
            f = frame(0, 1)
            want[5][i] = sum(f) / len(f) if f else None
            f = frame(-n, n)
            want[6][i] = sum(f) if f else None
    for k in range(7):
        assert out[k].to_pylist() == want[k], k


def _nds_frame(dev):
    """192 rows: 8 (cat, brand) groups of 24 distinct (year, moy) months, in
    shuffled order, with null sum_sales."""
    g = torch.Generator().manual_seed(120)
    rows = [(c, b, y, mo) for c in range(4) for b in range(2)
            for y in (1999, 2000) for mo in range(1, 13)]
    order = torch.randperm(len(rows), generator=g).tolist()
    rows = [rows[i] for i in order]
    n = len(rows)
    t = torch.tensor(rows, dtype=torch.int64)
    sales = torch.randint(-4000, 4000, (n,), generator=g).to(torch.float64) / 8
    vsales = torch.rand(n, generator=g) < 0.85
    return Frame({
        "cat": Val(t[:, 0].contiguous().to(dev), None,
                   ["c%d" % i for i in range(4)]),
        "brand": Val(t[:, 1].contiguous().to(dev)),
        "d_year": Val(t[:, 2].contiguous().to(dev)),
        "d_moy": Val(t[:, 3].contiguous().to(dev)),
        "sum_sales": Val(sales.to(dev), vsales.to(dev)),
    }, n)


def _run_nds(dev):
    """lag / lead of the Window node against the row_number self-join
    construction of queries._monthly_rank_lag."""
    order = [("d_year", True), ("d_moy", True)]
    keys = ["cat", "brand"]
    eng = Engine({}, device=dev)
    eng.register("t", _nds_frame(dev))
    direct = eng.run(Window(Scan("t"), keys,
                            [("psum", "lag", "sum_sales", order, 1),
                             ("nsum", "lead", "sum_sales", order),
                             ("p2", "lag", "d_moy", order, 2),
                             ("rn", "row_number", None, order)]))
    assert direct.cols["psum"].data.dtype == torch.float64
    assert direct.cols["p2"].data.dtype == torch.int64  # not cast to float64
    assert direct.cols["psum"].valid is not None
    eng.register("v1", eng.run(Window(Scan("t"), keys,
                                      [("rn", "row_number", None, order)])))
    v1 = Scan("v1")
    prev = Project(v1, [("rnp", col("rn") + 1), ("psum", col("sum_sales"))] +
                   [(f"p_{k}", col(k)) for k in keys])
    nxt = Project(v1, [("rnn", col("rn") - 1), ("nsum", col("sum_sales"))] +
                  [(f"n_{k}", col(k)) for k in keys])
    p = Join(v1, prev, [(k, f"p_{k}") for k in keys] + [("rn", "rnp")],
             "inner")
    p = Join(p, nxt, [(k, f"n_{k}") for k in keys] + [("rn", "rnn")], "inner")
    joined = eng.run(p)
    names = joined.names()
    pick = [names.index(k) for k in
            ("cat", "brand", "d_year", "d_moy", "psum", "nsum")]
    want = sorted((tuple(r[i] for i in pick) for r in joined.to_rows()),
                  key=repr)
    dn = direct.names()
    dpick = [dn.index(k) for k in
             ("cat", "brand", "d_year", "d_moy", "psum", "nsum")]
    rn_i = dn.index("rn")
    drows = direct.to_rows()
    # the self-joins keep the rows that have both a previous and a next month
    got = sorted((tuple(r[i] for i in dpick) for r in drows
                  if 1 < r[rn_i] < 24), key=repr)
    assert len(want) == 8 * 22
    assert [repr(r) for r in got] == [repr(r) for r in want]
    assert any(r[4] is None for r in got) and any(r[5] is None for r in got)
    # the first month has no previous one, the last no next one
    for r in drows:
        if r[rn_i] == 1:
            assert r[dn.index("psum")] is None
        if r[rn_i] == 24:
            assert r[dn.index("nsum")] is None
        want_p2 = None if r[rn_i] <= 2 else (r[dn.index("d_moy")] - 3) % 12 + 1
        assert r[dn.index("p2")] == want_p2
    return drows


# ---------------------------------------------------------------------------
# CPU tier
# ---------------------------------------------------------------------------

def _descs(specs):
    """Descriptor tuples of the binding for (fn code, lo, hi, shift), with
    dummy aligned pointers: the path predicate reads the offsets only."""
    return [((fn, 1, 2, 8, 1, 64, 0, 64, 64), lo, hi, sh)
            for fn, lo, hi, sh in specs]


def test_constants_mirror_the_native_header(monkeypatch):
    monkeypatch.delenv(DIRECT_ENV, raising=False)
    g = _native.gpu()  # the extension loads without a GPU
    assert (g.ROLL_TILE_ROWS, g.ROLL_MAX_REACH) == (R, H)
    assert R % 256 == 0 and H % 128 == 0
    SUM, SHIFT = 4, g.ROLL_FN_SHIFT
    assert g.window_rolling_staged(_descs([(SUM, -H, H, 0)]))
    assert not g.window_rolling_staged(_descs([(SUM, -H - 1, 0, 0)]))
    assert not g.window_rolling_staged(_descs([(SUM, 0, H + 1, 0)]))
    assert not g.window_rolling_staged(
        _descs([(SUM, -1, 1, 0), (SUM, 0, H + 1, 0)]))
    # lag and lead are never staged and do not decide the path
    assert g.window_rolling_staged(
        _descs([(SUM, -1, 1, 0), (SHIFT, 0, 0, 2 ** 31 - 1)]))
    assert not g.window_rolling_staged(_descs([(SHIFT, 0, 0, 1)]))
    monkeypatch.setenv(DIRECT_ENV, "1")
    assert not g.window_rolling_staged(_descs([(SUM, -H, H, 0)]))
    monkeypatch.setenv(DIRECT_ENV, "0")
    assert g.window_rolling_staged(_descs([(SUM, -H, H, 0)]))
    with pytest.raises(ValueError, match="lo > hi"):
        g.window_rolling_staged(_descs([(SUM, 1, 0, 0)]))
    with pytest.raises(ValueError, match="offset"):
        g.window_rolling_staged(_descs([(SUM, 0, 2 ** 31, 0)]))
    with pytest.raises(ValueError, match="unknown function"):
        g.window_rolling_staged(_descs([(0, 0, 0, 0)]))  # row_number


@pytest.mark.parametrize("part_pat", PARTS)
@pytest.mark.parametrize("m", SIZES)
def test_cpu_twin_grid(m, part_pat):
    _run_case("cpu", m, part_pat, *_rotation(m, part_pat))


@pytest.mark.parametrize("null_pat", NULLS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_cpu_twin_dtypes_and_nulls(dtype, null_pat):
    _run_case("cpu", R + 1, "random5", dtype, null_pat)


def test_cpu_float_specials():
    _run_float_specials("cpu")


def test_cpu_mixed_old_and_new_forms():
    _run_mixed("cpu")


def test_cpu_strided_inputs():
    _run_strided("cpu")


def test_cpu_table_level():
    _run_table("cpu")


def test_cpu_nds_lag_lead_equal_the_self_joins():
    _run_nds("cpu")


def test_empty_input():
    e64 = torch.empty(0, dtype=torch.int64)
    eb = torch.empty(0, dtype=torch.bool)
    v = torch.empty(0, dtype=torch.float32)
    out = W.window_tensors(e64, eb, [("lag", v, None, 1),
                                     ("sum", v, None, ("rows", -1, 0)),
                                     ("sum", v, None, ("rows", -2, -1)),
                                     ("count", v, eb, ("rows", 1, 2)),
                                     ("max", v, eb, ("rows", 0, 0))])
    assert [d.dtype for d, _ in out] == [torch.float32, torch.float64,
                                         torch.float64, torch.int64,
                                         torch.float32]
    assert [d.numel() for d, _ in out] == [0] * 5
    assert [o is None for _, o in out] == [False, True, False, True, False]


def test_result_conventions():
    m = 8
    perm = torch.arange(m)
    part = torch.zeros(m, dtype=torch.bool)
    v = torch.arange(m, dtype=torch.int16)
    ok = torch.ones(m, dtype=torch.bool)
    out = W.window_tensors(perm, part, [
        ("lag", v, None, 1), ("lead", v, ok, 1),
        ("count", v, ok, ("rows", 1, 2)), ("sum", v, None, ("rows", -1, 1)),
        ("sum", v, ok, ("rows", -1, 1)), ("min", v, None, ("rows", 1, 2)),
        ("avg", v, None, ("rows", -2, -1)), ("max", v, None, ("rows", 0, 0))])
    assert [d.dtype for d, _ in out] == [
        torch.int16, torch.int16, torch.int64, torch.int64, torch.int64,
        torch.int16, torch.float64, torch.int16]
    assert [o is None for _, o in out] == [False, False, True, True, False,
                                           False, False, True]
    assert out[0][0].tolist() == [0, 0, 1, 2, 3, 4, 5, 6]
    assert out[0][1].tolist() == [False] + [True] * 7
    assert out[5][1].tolist() == [True] * 7 + [False]


def test_argument_validation():
    m = 8
    perm = torch.arange(m)
    part = torch.zeros(m, dtype=torch.bool)
    v = torch.arange(m, dtype=torch.int32)
    big = 2 ** 31

    def call(*spec):
        return W.window_tensors(perm, part, [("sum", v, None, "rows"), spec])

    with pytest.raises(ValueError, match=r"funcs\[1\].*lo > hi"):
        call("sum", v, None, ("rows", 1, 0))
    for bad in (1.0, True, "1"):
        with pytest.raises(TypeError, match=r"funcs\[1\].*int"):
            call("sum", v, None, ("rows", bad, 2))
        with pytest.raises(TypeError, match=r"funcs\[1\].*int"):
            call("sum", v, None, ("rows", -1, bad))
    for bad in (1.0, True, None):
        with pytest.raises(TypeError, match=r"funcs\[1\].*int"):
            call("lag", v, None, bad)
    with pytest.raises(ValueError, match=r"funcs\[1\].*2\*\*31"):
        call("sum", v, None, ("rows", -big, 0))
    with pytest.raises(ValueError, match=r"funcs\[1\].*2\*\*31"):
        call("sum", v, None, ("rows", 0, big))
    with pytest.raises(ValueError, match=r"funcs\[1\].*2\*\*31"):
        call("lead", v, None, -big)
    call("sum", v, None, ("rows", -(big - 1), big - 1))
    call("lag", v, None, big - 1)
    with pytest.raises(ValueError, match=r"funcs\[1\].*needs values"):
        call("lag", None, None, 1)
    with pytest.raises(ValueError, match=r"funcs\[1\].*row offset"):
        call("lag", v, None, ("rows", -1, 0))
    with pytest.raises(ValueError, match=r"funcs\[1\].*row offset"):
        call("lead", v, None, "rows")
    with pytest.raises(ValueError, match=r"funcs\[1\].*unknown frame"):
        call("sum", v, None, ("range", -1, 0))
    with pytest.raises(ValueError, match=r"funcs\[1\].*unknown frame"):
        call("sum", v, None, ("rows", -1))
    with pytest.raises(NotImplementedError, match="unbounded on one side"):
        call("sum", v, None, ("rows", None, 0))
    with pytest.raises(NotImplementedError, match="unbounded on one side"):
        call("max", v, None, ("rows", -1, None))
    with pytest.raises(ValueError, match=r"funcs\[1\].*unknown function"):
        call("first_value", v, None, ("rows", -1, 0))
    # ranking functions go on ignoring the frame
    peer = torch.ones(m, dtype=torch.bool)
    out = W.window_tensors(perm, part,
                           [("row_number", None, None, ("rows", -1, 0))], peer)
    assert out[0][0].tolist() == list(range(1, m + 1))


# ---------------------------------------------------------------------------
# GPU tier
# ---------------------------------------------------------------------------

@pytest.fixture
def no_path_override(monkeypatch):
    monkeypatch.delenv(DIRECT_ENV, raising=False)


@pytest.mark.gpu
@pytest.mark.parametrize("part_pat", PARTS)
@pytest.mark.parametrize("m", SIZES)
def test_gpu_grid(m, part_pat, no_path_override):
    _run_case("cuda", m, part_pat, *_rotation(m, part_pat))


@pytest.mark.gpu
@pytest.mark.parametrize("null_pat", NULLS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_gpu_dtypes_and_nulls(dtype, null_pat, no_path_override):
    _run_case("cuda", R + 1, "random5", dtype, null_pat)


@pytest.mark.gpu
@pytest.mark.parametrize("m,part_pat", [(R + 1, "random5"),
                                        (3 * R + 7, "span"),
                                        (3 * R + 7, "one")])
def test_gpu_staged_equals_direct_and_runs_repeat(m, part_pat, monkeypatch):
    key = (m, part_pat) + _rotation(m, part_pat)
    perm, part, funcs, want = case(*key)
    monkeypatch.delenv(DIRECT_ENV, raising=False)
    staged = run_op("cuda", perm, part, funcs)
    again = run_op("cuda", perm, part, funcs)
    monkeypatch.setenv(DIRECT_ENV, "1")
    direct = run_op("cuda", perm, part, funcs)
    _raw_equal(staged, again)
    _raw_equal(staged, direct)
    compare(direct, want, funcs)


@pytest.mark.gpu
def test_gpu_float_specials(no_path_override):
    _run_float_specials("cuda")


@pytest.mark.gpu
def test_gpu_mixed_old_and_new_forms(no_path_override):
    _run_mixed("cuda")


@pytest.mark.gpu
def test_gpu_strided_inputs(no_path_override):
    _run_strided("cuda")


@pytest.mark.gpu
def test_gpu_table_level(no_path_override):
    _run_table("cuda")


@pytest.mark.gpu
def test_gpu_perm_entries_off_the_column_hold_no_row(no_path_override):
    """Positions whose perm entry is outside [0, m) get no result and count
    as null sources; nothing is read or written through them."""
    m = R + 1
    perm, part = make_structure(m, "random5", 61)
    values = make_values(m, "int32", 61, perm)
    funcs = [("sum", values, None, ("rows", -2, 1)), ("lag", values, None, 1),
             ("count", None, None, ("rows", -H - 1, 0))]
    bad = [5, R - 1, R]
    holes = perm[bad].copy()
    vl = np.ones(m, dtype=bool)
    vl[holes] = False  # the oracle sees the same rows as nulls
    want = oracle(perm, part, [(fn, v, vl, arg) for fn, v, _vl, arg in funcs])
    broken = perm.copy()
    broken[bad] = [-1, m, 1 << 40]
    p = part.copy()
    p[0] = False
    tv = to_torch(values, "cuda")
    outs = W.window_tensors(to_torch(broken, "cuda"), to_torch(p, "cuda"),
                            [(fn, tv, None, arg) for fn, _v, _vl, arg in
                             funcs])
    keep = np.ones(m, dtype=bool)
    keep[holes] = False
    for (d, _o), (wd, _wo) in zip(outs, want):
        assert np.array_equal(d.cpu().numpy()[keep], wd[keep])
    # count(*) has no values to be null: the holes still count as no row
    assert outs[1][1].cpu().numpy()[keep].tolist() == want[1][1][keep].tolist()


class Guarded:
    """n elements of device memory in the middle of a tensor of 0xA5, with
    64 guard bytes on each side."""
    GUARD = 64

    def __init__(self, n, dtype):
        self.nbytes = n * torch.empty(0, dtype=dtype).element_size()
        pad = (self.nbytes + 7) // 8 * 8
        self.big = torch.full((2 * self.GUARD + pad,), 0xA5,
                              dtype=torch.uint8, device="cuda")
        self.mid = self.big[self.GUARD:self.GUARD + self.nbytes].view(dtype)
        assert self.mid.data_ptr() % 8 == 0

    def check(self, what):
        h = self.big.cpu().numpy()
        assert (h[:self.GUARD] == 0xA5).all(), f"{what}: wrote in front"
        assert (h[self.GUARD + self.nbytes:] == 0xA5).all(), \
            f"{what}: wrote past the end"
        assert (h[self.GUARD:self.GUARD + self.nbytes] != 0xA5).any(), what


@pytest.mark.gpu
@pytest.mark.parametrize("direct", [False, True])
def test_gpu_guard_bands_round_the_outputs(direct, no_path_override):
    g = _native.gpu()
    m = R + 1
    perm, part = make_structure(m, "random5", 71)
    rng = np.random.default_rng(71)
    v8 = to_torch(rng.integers(-100, 100, m).astype(np.int8), "cuda")
    v16 = to_torch(rng.integers(-100, 100, m).astype(np.int16), "cuda")
    v32 = to_torch(rng.standard_normal(m).astype(np.float32), "cuda")
    tperm, tpart = to_torch(perm, "cuda"), to_torch(part, "cuda")
    stream = _native.current_stream()
    rn = torch.empty(m, dtype=torch.int64, device="cuda")
    pc = torch.empty(m, dtype=torch.int64, device="cuda")
    ident = torch.arange(m, device="cuda")
    work = torch.empty(g.window_work_bytes(m, 2) // 8 + 1, dtype=torch.int64,
                       device="cuda")
    g.window([(0, 1, 0, 1, 1, 0, 0, rn.data_ptr(), 0),
              (3, 0, 0, 1, 1, 0, 0, pc.data_ptr(), 0)], ident.data_ptr(),
             tpart.data_ptr(), 0, m, work.data_ptr(), stream)
    lo, hi = (-H - 1, 1) if direct else (-2, 1)
    SHIFT = g.ROLL_FN_SHIFT
    plan = [(SHIFT, v8, torch.int8, 0, 0, 1), (SHIFT, v16, torch.int16, 0, 0,
                                               -1),
            (SHIFT, v32, torch.float32, 0, 0, 3),
            (6, v8, torch.int8, lo, hi, 0), (5, v16, torch.int16, lo, hi, 0),
            (4, v32, torch.float64, lo, hi, 0),
            (7, v16, torch.float64, lo, hi, 0), (3, v8, torch.int64, lo, hi, 0)]
    outs, descs = [], []
    for fn, v, odt, a, b, sh in plan:
        data, ok = Guarded(m, odt), Guarded(m, torch.bool)
        outs.append((data, ok))
        kind = 3 if v.dtype == torch.float32 else 2
        descs.append(((fn, 1, kind, v.element_size(), 1, v.data_ptr(), 0,
                       data.mid.data_ptr(),
                       0 if fn == 3 else ok.mid.data_ptr()), a, b, sh))
    assert g.window_rolling_staged(descs) == (not direct)
    g.window_rolling(descs, tperm.data_ptr(), rn.data_ptr(), pc.data_ptr(), m,
                     stream)
    torch.cuda.synchronize()
    for n, (data, ok) in enumerate(outs):
        data.check(f"funcs[{n}] data")
        if plan[n][0] != 3:
            ok.check(f"funcs[{n}] valid")


@pytest.mark.gpu
def test_runs_under_stream_capture(no_path_override):
    m = R + 1
    dev = "cuda"

    def inputs(seed):
        perm, part = make_structure(m, "random5", seed)
        values = make_values(m, "float64", seed, perm)
        valid = make_valid(m, "leading", part, perm)
        return perm, part, values, valid

    def specs(v, vl):
        return [("lag", v, vl, 1), ("sum", v, vl, ("rows", -2, 0)),
                ("rank", None, None, "rows"),
                ("max", v, vl, ("rows", -H - 1, 0)),
                ("avg", v, vl, ("rows", -1, 1)), ("lead", v, None, 65)]

    perm, part, values, valid = inputs(91)
    perm2, part2, values2, valid2 = inputs(92)
    funcs2 = [s for s in specs(values2, valid2) if s[0] != "rank"]
    want2 = oracle(perm2, part2, funcs2)
    tp, tpart = to_torch(perm, dev), to_torch(part, dev)
    tv, tvl = to_torch(values, dev), to_torch(valid, dev)
    W.window_tensors(tp, tpart, specs(tv, tvl), tpart)  # warm up
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            out = W.window_tensors(tp, tpart, specs(tv, tvl), tpart)
    torch.cuda.current_stream().wait_stream(side)
    for dst, src in ((tp, perm2), (tpart, part2), (tv, values2),
                     (tvl, valid2)):
        dst.copy_(to_torch(src, dev))
    graph.replay()
    torch.cuda.synchronize()
    got = [(d.cpu().numpy(), None if v is None else v.cpu().numpy())
           for n, (d, v) in enumerate(out) if n != 2]
    compare(got, want2, funcs2)


@pytest.mark.gpu
def test_gpu_nds_lag_lead(monkeypatch, no_path_override):
    want = _run_nds("cpu")
    from spark_rapids_jni_amd.ops import window as opw
    calls = []
    real = opw.window_tensors

    def counting(perm, part, funcs, peer=None):
        calls.append([f[0] for f in funcs])
        return real(perm, part, funcs, peer)

    monkeypatch.setattr(opw, "window_tensors", counting)
    got = _run_nds("cuda")
    monkeypatch.undo()
    # lag, lead and row_number share one order: one sort, one call
    assert ["lag", "lead", "lag", "row_number"] in calls
    assert [repr(r) for r in got] == [repr(r) for r in want]
