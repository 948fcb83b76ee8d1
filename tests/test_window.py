"""Window functions (ops/window.py, src/gpu/window.hip): the native kernels
and their CPU twin against two oracles that use neither the op nor a torch
scan.

* The LOOP ORACLE walks the sorted positions in plain Python, one function at
  a time: math.fsum for float sums, an explicit NaN-greatest comparison for
  min and max.
* The NUMPY ORACLE is vectorised (np.add.reduceat / np.maximum.accumulate on
  head indices) for the one large size, and is itself checked against the
  loop oracle at small sizes.

Exact: ranking functions, count, integer sum, min, max, all validity, the
data word under a null (zero), and float sums over quarter-integers (every
partial sum is exactly representable, so any order of summation is exact).
With a bound: float sum over general values, |got - want| <= k * 2**-52 *
sum|x_j| with k the number of valid values of the frame (gamma_(k-1) * sum|x|
for any summation order plus the oracle's one rounding); avg takes that bound
divided by the count plus one ulp of the quotient.
"""
import functools
import math

import numpy as np
import pytest
import torch

from spark_rapids_jni_amd import _native
from spark_rapids_jni_amd.columnar import Column, DType, Table
from spark_rapids_jni_amd.nds.expr import Val
from spark_rapids_jni_amd.nds.plan import Engine, Frame, Scan, Window
from spark_rapids_jni_amd.ops import window as W

T = W.TILE_ROWS
S = W.SMALL_ROWS
SIZES = sorted({0, 1, 2, 63, 64, 65, S - 1, S, S + 1, T + 1, 3 * T + 7})
# the carry scan takes CARRY_CHUNK tile carries per round: two rounds
TWO_CHUNKS = W.CARRY_CHUNK * T + 1
assert TWO_CHUNKS <= 1 << 22  # else the case would have to be left out
PARTS = ["one", "each", "random5", "span"]
PEERS = ["all", "distinct", "ties"]
NULLS = ["none", "all", "interior", "leading"]
DTYPES = ["bool", "int8", "int16", "int32", "int64", "float32", "float64"]
NP_DTYPE = {"bool": np.bool_, "int8": np.int8, "int16": np.int16,
            "int32": np.int32, "int64": np.int64, "float32": np.float32,
            "float64": np.float64}
FRAMES = ["partition", "rows", "range"]
RANKING = ("row_number", "rank", "dense_rank")
I64 = np.iinfo(np.int64)


# ---------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------

def make_structure(m, part_pat, peer_pat, seed):
    """perm (a genuine shuffle) and normalised head flags per sorted
    position."""
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
        if m >= 3 * T + 3:
            # one partition from a tile's last row to just before the head
            # on a tile's first row, three tiles on; length-1 neighbours
            heads = [T - 3, T - 2, T - 1, 3 * T, 3 * T + 1, 3 * T + 2]
        else:
            heads = [1, 2, m - 3, m - 2, m - 1]
        for h in heads:
            if 0 < h < m:
                part[h] = True
    peer = part.copy()
    if peer_pat == "distinct":
        peer[:] = True
    elif peer_pat == "ties":
        peer |= rng.random(m) < 0.5
    return perm, part, peer


def raw_flags(part, peer):
    """What a careless caller passes: position 0 unflagged and the peer
    flags without the partition heads. The op has to repair both."""
    p = part.copy()
    if p.size:
        p[0] = False
    return p, peer & ~part


def make_values(m, dtype, seed, perm):
    """Values in ORIGINAL row order. Float specials sit in the second half
    of the sorted order, so the first half keeps finite sums."""
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


def make_valid(m, pattern, part, perm, seed):
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
    elif pattern == "leading":
        for h, e in zip(heads, ends):
            vs[h:h + (e - h + 1) // 3] = False
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


def _frame_ends(part, peer):
    m = len(part)
    ep, eq = [0] * m, [0] * m
    lastp = lastq = m - 1
    for i in range(m - 1, -1, -1):
        ep[i], eq[i] = lastp, lastq
        if part[i]:
            lastp = i - 1
        if peer[i]:
            lastq = i - 1
    return ep, eq


def _float_sum(finite, nan, pinf, ninf):
    if nan or (pinf and ninf):
        return math.nan
    if pinf:
        return math.inf
    if ninf:
        return -math.inf
    return math.fsum(finite)


def _running(fn, vs, valid, part, peer, is_float):
    """Per sorted position: (count, value, sum|x|) over the rows of the
    partition up to it."""
    m = len(part)
    out = [None] * m
    for i in range(m):
        if part[i]:
            cnt, acc, ps, qs, dense = 0, None, i, i, 0
            finite, absx, nan, pinf, ninf, isum = [], [], 0, 0, 0, 0
        if peer[i]:
            qs = i
            dense += 1
        if fn == "row_number":
            out[i] = (1, i - ps + 1, 0.0)
            continue
        if fn == "rank":
            out[i] = (1, qs - ps + 1, 0.0)
            continue
        if fn == "dense_rank":
            out[i] = (1, dense, 0.0)
            continue
        if valid is None or valid[i]:
            cnt += 1
            if fn == "count":
                pass
            elif fn in ("min", "max"):
                x = vs[i]
                if acc is None:
                    acc = x
                elif fn == "max" and _greater(x, acc):
                    acc = x
                elif fn == "min" and _greater(acc, x):
                    acc = x
            elif is_float or fn == "avg":
                x = float(vs[i])
                if x != x:
                    nan += 1
                elif x == math.inf:
                    pinf += 1
                elif x == -math.inf:
                    ninf += 1
                else:
                    finite.append(x)
                    absx.append(abs(x))
            else:
                isum += int(vs[i])
        if fn == "count":
            out[i] = (cnt, cnt, 0.0)
        elif fn in ("min", "max"):
            out[i] = (cnt, acc, 0.0)
        elif is_float or fn == "avg":
            out[i] = (cnt, _float_sum(finite, nan, pinf, ninf),
                      math.fsum(absx))
        else:
            out[i] = (cnt, _wrap64(isum), 0.0)
    return out


def oracle_loop(perm, part, peer, funcs):
    """funcs: (fn, values or None, valid or None, frame) with numpy values in
    original row order. Returns per function (data, valid, bound): lists in
    original row order; bound is the allowed |error| (None = exact)."""
    m = len(perm)
    ep, eq = _frame_ends(part, peer)
    idx = list(range(m))
    ends = {"rows": idx, "partition": ep, "range": eq}
    permL = perm.tolist()
    cache = {}
    results = []
    for fn, values, valid, frame in funcs:
        key = (fn, id(values), id(valid))
        if key not in cache:
            vs = values[perm].tolist() if values is not None else None
            vl = valid[perm].tolist() if valid is not None else None
            is_float = values is not None and values.dtype.kind == "f"
            cache[key] = (_running(fn, vs, vl, part, peer, is_float),
                          is_float)
        states, is_float = cache[key]
        e = idx if fn in RANKING else ends[frame]
        data, ok, bound = [0] * m, [True] * m, [0.0] * m
        for i in range(m):
            cnt, val, sabs = states[e[i]]
            r = permL[i]
            if fn in RANKING or fn == "count":
                data[r] = val
            elif cnt == 0:
                data[r], ok[r] = 0, False
            elif fn == "avg":
                q = val / cnt
                data[r] = q
                ulp = math.ulp(q) if math.isfinite(q) else 0.0
                bound[r] = cnt * 2.0 ** -52 * sabs / cnt + ulp
            else:
                data[r] = val
                bound[r] = cnt * 2.0 ** -52 * sabs
        nullable = fn not in RANKING and fn != "count" and valid is not None
        results.append((data, ok if nullable else None, bound))
    return results


# ---------------------------------------------------------------------------
# numpy oracle (finite values whose sums are exact; integer min / max)
# ---------------------------------------------------------------------------

def oracle_numpy(perm, part, peer, funcs):
    m = len(perm)
    idx = np.arange(m, dtype=np.int64)
    heads = np.flatnonzero(part)
    lens = np.diff(np.append(heads, m))
    seg = np.repeat(np.arange(len(heads), dtype=np.int64), lens)
    ps = np.maximum.accumulate(np.where(part, idx, 0))
    qs = np.maximum.accumulate(np.where(peer, idx, 0))

    def last_of(head):
        nxt = np.where(head, idx, m)
        nxt = np.minimum.accumulate(nxt[::-1])[::-1]
        return np.append(nxt[1:], m) - 1

    ends = {"rows": idx, "partition": last_of(part), "range": last_of(peer)}

    def seg_running_sum(x):
        with np.errstate(over="ignore"):
            cs = np.cumsum(x)
            base = cs[heads] - x[heads]
            return cs - base[seg]

    results = []
    for fn, values, valid, frame in funcs:
        if fn == "row_number":
            res, cnt = idx - ps + 1, None
        elif fn == "rank":
            res, cnt = qs - ps + 1, None
        elif fn == "dense_rank":
            res, cnt = seg_running_sum(peer.astype(np.int64)), None
        else:
            vl = valid[perm] if valid is not None else np.ones(m, dtype=bool)
            if frame == "partition":
                cnt = np.add.reduceat(vl.astype(np.int64), heads)[seg]
            else:
                cnt = seg_running_sum(vl.astype(np.int64))[ends[frame]]
            if fn == "count":
                res = cnt
            elif fn in ("sum", "avg"):
                vs = values[perm]
                wide = np.float64 if (fn == "avg" or vs.dtype.kind == "f") \
                    else np.int64
                x = np.where(vl, vs.astype(wide), wide(0))
                if frame == "partition":
                    with np.errstate(over="ignore"):
                        res = np.add.reduceat(x, heads)[seg]
                else:
                    res = seg_running_sum(x)[ends[frame]]
                if fn == "avg":
                    res = res / np.maximum(cnt, 1)
            else:
                # values within 32 bits: one running extreme over keys that
                # put every partition above the one before it
                big = np.int64(1) << 34
                vs = values[perm].astype(np.int64)
                sign = 1 if fn == "max" else -1
                x = np.where(vl, sign * vs, -(big >> 1)) + seg * big
                res = sign * (np.maximum.accumulate(x) - seg * big)
                res = res[ends[frame]].astype(values.dtype)
            res = np.where(cnt > 0, res, np.zeros_like(res))
        data = np.empty_like(res)
        data[perm] = res
        ok = None
        if cnt is not None and fn != "count" and valid is not None:
            ok = np.empty(m, dtype=bool)
            ok[perm] = cnt > 0
        results.append((data, ok))
    return results


# ---------------------------------------------------------------------------
# running the op and comparing
# ---------------------------------------------------------------------------

def to_torch(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)) \
        .to(dev)


def run_op(dev, perm, part, peer, funcs, raw=True, with_peer=True):
    p, q = raw_flags(part, peer) if raw else (part, peer)
    tensors = {}

    def tt(a):
        if a is None:
            return None
        if id(a) not in tensors:
            tensors[id(a)] = to_torch(a, dev)
        return tensors[id(a)]

    specs = [(fn, tt(v), tt(vl), fr) for fn, v, vl, fr in funcs]
    got = W.window_tensors(to_torch(perm, dev), to_torch(p, dev), specs,
                           to_torch(q, dev) if with_peer else None)
    return [(d.cpu(), None if v is None else v.cpu()) for d, v in got]


def _same_float(got, want):
    if want != want:
        return got != got
    return got == want


def compare(got, want, funcs, exact_float_sum=True):
    assert len(got) == len(want) == len(funcs)
    for k, ((gd, gv), w, (fn, values, valid, frame)) in enumerate(
            zip(got, want, funcs)):
        wd, wv = w[0], w[1]
        bound = w[2] if len(w) > 2 else None
        what = f"funcs[{k}] = {fn}/{frame}"
        if fn in RANKING or fn in ("count",):
            assert gd.dtype == torch.int64, what
        elif fn == "avg":
            assert gd.dtype == torch.float64, what
        elif fn == "sum":
            assert gd.dtype == (torch.float64 if values.dtype.kind == "f"
                                else torch.int64), what
        else:
            assert gd.dtype == to_torch(values[:0], "cpu").dtype, what
        if wv is None:
            assert gv is None, what
        else:
            assert gv is not None and gv.dtype == torch.bool, what
            assert gv.tolist() == list(wv), what
        g = gd.tolist()
        wl = wd.tolist() if isinstance(wd, np.ndarray) else wd
        assert len(g) == len(wl), what
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
    """The three ranking functions, count(*) and the five aggregates of
    `values` over every frame: more than WINDOW_MAX_FUNCS in one call."""
    funcs = [(fn, None, None, "rows") for fn in RANKING]
    for fr in FRAMES:
        funcs.append(("count", None, None, fr))
        for fn in ("count", "sum", "min", "max", "avg"):
            funcs.append((fn, values, valid, fr))
    assert len(funcs) > 2 * W.WINDOW_MAX_FUNCS
    return funcs


@functools.lru_cache(maxsize=None)
def grid_case(m, part_pat, peer_pat, null_pat, dtype):
    """Inputs and the loop oracle's answer, computed once and shared by the
    CPU and GPU tests."""
    seed = 17 * m + 5 * PARTS.index(part_pat) + PEERS.index(peer_pat)
    perm, part, peer = make_structure(m, part_pat, peer_pat, seed)
    values = make_values(m, dtype, seed, perm)
    valid = make_valid(m, null_pat, part, perm, seed)
    funcs = all_funcs(values, valid)
    return perm, part, peer, funcs, oracle_loop(perm, part, peer, funcs)


def _rotation(m, part_pat):
    """Peer pattern, null pattern and dtype of a (size, partition pattern)
    cell: the grid as a whole covers each of them many times."""
    k = SIZES.index(m) * len(PARTS) + PARTS.index(part_pat)
    return PEERS[k % 3], NULLS[(k // 3) % 4], DTYPES[k % 7]


def _run_grid(dev, m, part_pat):
    perm, part, peer, funcs, want = grid_case(m, part_pat,
                                              *_rotation(m, part_pat))
    compare(run_op(dev, perm, part, peer, funcs), want, funcs)


def _run_dtype(dev, dtype, null_pat):
    perm, part, peer, funcs, want = grid_case(T + 1, "random5", "ties",
                                              null_pat, dtype)
    compare(run_op(dev, perm, part, peer, funcs), want, funcs)


def _run_peers(dev, peer_pat):
    m = 3 * T + 7
    perm, part, peer, funcs, want = grid_case(m, "span", peer_pat, "leading",
                                              "int32")
    got = run_op(dev, perm, part, peer, funcs)
    compare(got, want, funcs)
    by = {(fn, fr, v is None): d for (fn, v, _vl, fr), (d, _ok)
          in zip(funcs, got)}
    if peer_pat == "all":
        assert torch.equal(by[("rank", "rows", True)],
                           torch.ones(m, dtype=torch.int64))
        for fn in ("sum", "min", "max", "avg", "count"):
            assert torch.equal(by[(fn, "range", False)],
                               by[(fn, "partition", False)])
    if peer_pat == "distinct":
        assert torch.equal(by[("rank", "rows", True)],
                           by[("row_number", "rows", True)])
        for fn in ("sum", "min", "max", "avg", "count"):
            assert torch.equal(by[(fn, "range", False)],
                               by[(fn, "rows", False)])


@functools.lru_cache(maxsize=None)
def general_case(part_pat):
    m = 3 * T + 7
    perm, part, peer = make_structure(m, part_pat, "ties", 31)
    values = general_floats(m, 31, perm)
    valid = make_valid(m, "leading", part, perm, 31)
    funcs = [(fn, values, valid, fr) for fr in FRAMES
             for fn in ("sum", "avg")]
    return perm, part, peer, funcs, oracle_loop(perm, part, peer, funcs)


def _run_general(dev, part_pat):
    perm, part, peer, funcs, want = general_case(part_pat)
    got = run_op(dev, perm, part, peer, funcs)
    compare(got, want, funcs, exact_float_sum=False)
    return got


def _run_strided(dev):
    """A value column that is every other element of a buffer, a validity
    that starts one byte into its buffer, and flags sliced the same way."""
    m = T + 1
    perm, part, peer = make_structure(m, "random5", "ties", 41)
    values = make_values(m, "int32", 41, perm)
    valid = make_valid(m, "leading", part, perm, 41)
    funcs = [("sum", values, valid, "rows"), ("max", values, valid, "range"),
             ("rank", None, None, "rows")]
    want = oracle_loop(perm, part, peer, funcs)
    buf = torch.zeros(2 * m + 1, dtype=torch.int32, device=dev)
    v = buf[1::2]
    v.copy_(to_torch(values, dev))
    assert not v.is_contiguous() or m == 1
    vbuf = torch.zeros(m + 1, dtype=torch.bool, device=dev)
    vl = vbuf[1:]
    vl.copy_(to_torch(valid, dev))
    p, q = raw_flags(part, peer)
    pbuf = torch.zeros(m + 3, dtype=torch.bool, device=dev)
    pbuf[3:] = to_torch(p, dev)
    qbuf = torch.zeros(m + 5, dtype=torch.uint8, device=dev)
    qbuf[5:] = to_torch(q, dev).to(torch.uint8) * 7  # any nonzero is a head
    got = W.window_tensors(
        to_torch(perm, dev), pbuf[3:],
        [("sum", v, vl, "rows"), ("max", v, vl, "range"),
         ("rank", None, None, "rows")], qbuf[5:])
    compare([(d.cpu(), None if o is None else o.cpu()) for d, o in got],
            want, funcs)


def _run_table(dev):
    big = 1 << 64
    d128 = [(-3 * big + 5, -big, -1, 0, big + 1)[i % 5] for i in range(40)]
    d128 = [None if i % 11 == 0 else x for i, x in enumerate(d128)]
    rng = np.random.default_rng(51)
    okey = rng.integers(0, 4, 40).tolist()
    okey = [None if i % 7 == 3 else x for i, x in enumerate(okey)]
    vals = rng.integers(-50, 50, 40).tolist()
    vals = [None if i % 5 == 1 else x for i, x in enumerate(vals)]
    pcol = Column.from_pylist(d128, DType.DECIMAL128, dev, scale=2)
    ocol = Column.from_pylist(okey, DType.INT32, dev)
    vcol = Column.from_pylist(vals, DType.INT64, dev)
    out = W.window_columns(
        Table([pcol]), Table([ocol]),
        [("rank", None, "rows"), ("sum", vcol, "range"),
         ("min", vcol, "partition"), ("count", vcol, "rows"),
         ("avg", vcol, "partition")], ascending=[False])
    assert [c.dtype for c in out] == [DType.INT64, DType.INT64, DType.INT64,
                                      DType.INT64, DType.FLOAT64]
    # oracle by sorting in Python: nulls first for the ascending partition
    # key, last for the descending order key (the Spark defaults)
    def key(i):
        p, o = d128[i], okey[i]
        return ((0, 0) if p is None else (1, p),
                (1, 0) if o is None else (0, -o))
    order = sorted(range(40), key=key)
    want = {k: [None] * 40 for k in range(5)}
    for i in order:
        grp = [j for j in order if key(j)[0] == key(i)[0]]
        upto = [j for j in grp if key(j)[1] <= key(i)[1]]
        before = [j for j in grp if key(j)[1] < key(i)[1]]
        rows = grp[:grp.index(i) + 1]
        want[0][i] = len(before) + 1
        rv = [vals[j] for j in upto if vals[j] is not None]
        want[1][i] = sum(rv) if rv else None
        pv = [vals[j] for j in grp if vals[j] is not None]
        want[2][i] = min(pv) if pv else None
        want[3][i] = len([j for j in rows if vals[j] is not None])
        want[4][i] = sum(pv) / len(pv) if pv else None
    for k in range(5):
        assert out[k].to_pylist() == want[k], k
    # no partition columns: one partition
    one = W.window_columns(None, Table([ocol]),
                           [("row_number", None, "rows"),
                            ("count", None, "partition")])
    assert sorted(one[0].to_pylist()) == list(range(1, 41))
    assert one[1].to_pylist() == [40] * 40


# ---------------------------------------------------------------------------
# CPU tier: the oracles against each other, the twin, argument checking
# ---------------------------------------------------------------------------

def test_constants_mirror_the_native_header():
    g = _native.gpu()  # the extension loads without a GPU
    assert (g.WINDOW_MAX_FUNCS, g.WINDOW_SMALL_ROWS, g.WINDOW_TILE_ROWS,
            g.WINDOW_CARRY_CHUNK) == (W.WINDOW_MAX_FUNCS, S, T, W.CARRY_CHUNK)
    assert g.window_work_bytes(S, 3) == 0
    assert g.window_work_bytes(S + 1, 3) > 0
    assert W.window_work_bytes(S + 1, 3) == g.window_work_bytes(S + 1, 3)


def _numpy_case(m, part_pat, seed):
    perm, part, peer = make_structure(m, part_pat, "ties", seed)
    rng = np.random.default_rng(seed)
    vi = rng.integers(-2 ** 31, 2 ** 31, m).astype(np.int32)
    v64 = rng.integers(-2 ** 62, 2 ** 62, m).astype(np.int64)
    vf = (rng.integers(-200, 200, m) / 4.0).astype(np.float64)
    valid = make_valid(m, "leading", part, perm, seed)
    funcs = [(fn, None, None, "rows") for fn in RANKING]
    for fr in FRAMES:
        funcs += [("count", None, None, fr), ("count", vi, valid, fr),
                  ("sum", v64, valid, fr), ("sum", vf, valid, fr),
                  ("sum", vf, None, fr), ("min", vi, valid, fr),
                  ("max", vi, valid, fr), ("avg", vf, valid, fr)]
    return perm, part, peer, funcs


@pytest.mark.parametrize("part_pat", PARTS)
@pytest.mark.parametrize("m", [1, 65, T + 1])
def test_numpy_oracle_matches_loop_oracle(m, part_pat):
    perm, part, peer, funcs = _numpy_case(m, part_pat, 61 + m)
    loop = oracle_loop(perm, part, peer, funcs)
    vec = oracle_numpy(perm, part, peer, funcs)
    for (ld, lv, _b), (vd, vv) in zip(loop, vec):
        assert vd.tolist() == ld
        assert (None if vv is None else vv.tolist()) == lv


@pytest.mark.parametrize("part_pat", PARTS)
@pytest.mark.parametrize("m", SIZES)
def test_cpu_twin_grid(m, part_pat):
    _run_grid("cpu", m, part_pat)


@pytest.mark.parametrize("null_pat", NULLS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_cpu_twin_dtypes_and_nulls(dtype, null_pat):
    _run_dtype("cpu", dtype, null_pat)


@pytest.mark.parametrize("peer_pat", PEERS)
def test_cpu_twin_peer_patterns(peer_pat):
    _run_peers("cpu", peer_pat)


@pytest.mark.parametrize("part_pat", ["one", "random5"])
def test_cpu_twin_general_float_sums(part_pat):
    _run_general("cpu", part_pat)


def test_cpu_twin_strided_inputs():
    _run_strided("cpu")


def test_cpu_table_level():
    _run_table("cpu")


def test_without_peer_flags_every_row_is_its_own_peer_group():
    m = 65
    perm, part, _peer = make_structure(m, "random5", "all", 71)
    values = make_values(m, "int16", 71, perm)
    funcs = [("sum", values, None, "range"), ("count", None, None, "range")]
    want = oracle_loop(perm, part, np.ones(m, dtype=bool), funcs)
    compare(run_op("cpu", perm, part, part, funcs, with_peer=False), want,
            funcs)


def test_empty_input():
    e64 = torch.empty(0, dtype=torch.int64)
    eb = torch.empty(0, dtype=torch.bool)
    v = torch.empty(0, dtype=torch.float32)
    out = W.window_tensors(e64, eb, [("rank", None, None, "rows"),
                                     ("sum", v, eb, "rows"),
                                     ("min", v, None, "partition")], eb)
    assert [d.dtype for d, _ in out] == [torch.int64, torch.float64,
                                         torch.float32]
    assert [d.numel() for d, _ in out] == [0, 0, 0]
    assert out[0][1] is None and out[2][1] is None
    assert out[1][1].dtype == torch.bool and out[1][1].numel() == 0


def test_argument_validation():
    m = 8
    perm = torch.arange(m)
    part = torch.zeros(m, dtype=torch.bool)
    v = torch.arange(m, dtype=torch.int32)
    ok = torch.ones(m, dtype=torch.bool)
    good = ("sum", v, ok, "rows")
    with pytest.raises(TypeError, match="perm"):
        W.window_tensors(perm.to(torch.int32), part, [good])
    with pytest.raises(ValueError, match="perm"):
        W.window_tensors(perm.view(2, 4), part, [good])
    with pytest.raises(TypeError, match="part_flags"):
        W.window_tensors(perm, part.to(torch.int32), [good])
    with pytest.raises(ValueError, match="part_flags"):
        W.window_tensors(perm, part[:-1], [good])
    with pytest.raises(ValueError, match="peer_flags"):
        W.window_tensors(perm, part, [good], part[:-1])
    with pytest.raises(ValueError, match=r"funcs\[1\].*unknown function"):
        W.window_tensors(perm, part, [good, ("median", v, None, "rows")])
    with pytest.raises(ValueError, match=r"funcs\[1\].*unknown frame"):
        W.window_tensors(perm, part, [good, ("sum", v, None, "2 preceding")])
    with pytest.raises(ValueError, match=r"funcs\[0\].*peer_flags"):
        W.window_tensors(perm, part, [("rank", None, None, "rows")])
    with pytest.raises(ValueError, match=r"funcs\[0\].*needs values"):
        W.window_tensors(perm, part, [("min", None, None, "rows")])
    with pytest.raises(TypeError, match=r"funcs\[1\].*dtype"):
        W.window_tensors(perm, part, [good, ("sum", v.to(torch.float16),
                                             None, "rows")])
    with pytest.raises(ValueError, match=r"funcs\[1\].*1-D"):
        W.window_tensors(perm, part, [good, ("sum", v.view(2, 4), None,
                                             "rows")])
    with pytest.raises(ValueError, match=r"funcs\[1\].*rows"):
        W.window_tensors(perm, part, [good, ("sum", v[:-1], None, "rows")])
    with pytest.raises(TypeError, match=r"funcs\[1\].*valid"):
        W.window_tensors(perm, part, [good, ("sum", v, ok.to(torch.int32),
                                             "rows")])
    with pytest.raises(ValueError, match=r"funcs\[1\].*valid"):
        W.window_tensors(perm, part, [good, ("sum", v, ok[:-1], "rows")])
    with pytest.raises(ValueError, match=r"funcs\[0\]"):
        W.window_tensors(perm, part, [("sum", v, "rows")])
    if torch.cuda.is_available():
        with pytest.raises(ValueError, match=r"funcs\[0\].*devices"):
            W.window_tensors(perm, part, [("sum", v.cuda(), None, "rows")])
        with pytest.raises(ValueError, match="part_flags.*devices"):
            W.window_tensors(perm, part.cuda(), [good])


# ---------------------------------------------------------------------------
# GPU tier
# ---------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("part_pat", PARTS)
@pytest.mark.parametrize("m", SIZES)
def test_gpu_grid(m, part_pat):
    _run_grid("cuda", m, part_pat)


@pytest.mark.gpu
@pytest.mark.parametrize("null_pat", NULLS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_gpu_dtypes_and_nulls(dtype, null_pat):
    _run_dtype("cuda", dtype, null_pat)


@pytest.mark.gpu
@pytest.mark.parametrize("peer_pat", PEERS)
def test_gpu_peer_patterns(peer_pat):
    _run_peers("cuda", peer_pat)


@pytest.mark.gpu
@pytest.mark.parametrize("part_pat", ["one", "random5"])
def test_gpu_general_float_sums(part_pat):
    _run_general("cuda", part_pat)


@pytest.mark.gpu
def test_gpu_float_sums_are_deterministic():
    a = _run_general("cuda", "random5")
    b = _run_general("cuda", "random5")
    for (da, va), (db, vb) in zip(a, b):
        assert torch.equal(da, db) and torch.equal(va, vb)


@pytest.mark.gpu
def test_gpu_strided_inputs():
    _run_strided("cuda")


@pytest.mark.gpu
def test_gpu_table_level():
    _run_table("cuda")


@pytest.mark.gpu
def test_gpu_without_peer_flags():
    m = T + 1
    perm, part, _peer = make_structure(m, "random5", "all", 73)
    values = make_values(m, "int16", 73, perm)
    funcs = [("sum", values, None, "range"), ("count", None, None, "range")]
    want = oracle_loop(perm, part, np.ones(m, dtype=bool), funcs)
    compare(run_op("cuda", perm, part, part, funcs, with_peer=False), want,
            funcs)


@pytest.mark.gpu
@pytest.mark.parametrize("part_pat", ["one", "random5", "span"])
def test_gpu_carry_scan_takes_two_chunks(part_pat):
    """Vectorised oracle only. `span` keeps one partition open across the
    chunk border of the carry scan."""
    m = TWO_CHUNKS
    perm, part, peer, funcs = _numpy_case(m, part_pat, 81)
    if part_pat == "span":
        part[:] = False
        part[[0, T - 1, m - 2]] = True
        peer |= part
    want = oracle_numpy(perm, part, peer, funcs)
    got = run_op("cuda", perm, part, peer, funcs)
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
        perm, part, peer = make_structure(m, "random5", "ties", seed)
        values = make_values(m, "float64", seed, perm)
        valid = make_valid(m, "leading", part, perm, seed)
        return perm, part, peer, values, valid

    def specs(v, vl):
        return [("rank", None, None, "rows"), ("sum", v, vl, "partition"),
                ("max", v, vl, "rows"), ("avg", v, vl, "range")]

    perm, part, peer, values, valid = case(91)
    perm2, part2, peer2, values2, valid2 = case(92)
    funcs2 = specs(values2, valid2)
    want2 = oracle_loop(perm2, part2, peer2, funcs2)
    tp, tpart, tpeer = (to_torch(x, dev) for x in (perm, part, peer))
    tv, tvl = to_torch(values, dev), to_torch(valid, dev)
    W.window_tensors(tp, tpart, specs(tv, tvl), tpeer)  # warm up
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            out = W.window_tensors(tp, tpart, specs(tv, tvl), tpeer)
    torch.cuda.current_stream().wait_stream(side)
    for dst, src in ((tp, perm2), (tpart, part2), (tpeer, peer2),
                     (tv, values2), (tvl, valid2)):
        dst.copy_(to_torch(src, dev))
    graph.replay()
    torch.cuda.synchronize()
    compare([(d.cpu(), None if v is None else v.cpu()) for d, v in out],
            want2, funcs2)


def _routing_frame(dev, n):
    g = torch.Generator().manual_seed(110)
    part = torch.randint(0, 6, (n,), generator=g)
    vpart = torch.rand(n, generator=g) < 0.9
    score = torch.randint(-20, 20, (n,), generator=g).to(torch.float64) / 2
    vscore = torch.rand(n, generator=g) < 0.8
    code = torch.randint(0, 5, (n,), generator=g)
    qty = torch.randint(-3, 3, (n,), generator=g).to(torch.int32)
    return Frame({
        "part": Val(part.to(dev), vpart.to(dev)),
        "score": Val(score.to(dev), vscore.to(dev)),
        "code": Val(code.to(dev), None, ["d%d" % i for i in range(5)]),
        "qty": Val(qty.to(dev)),
    }, n)


@pytest.mark.gpu
def test_nds_window_routes_to_the_native_op(monkeypatch):
    shared = [("qty", True), ("score", True)]
    specs = [("rk", "rank", None, [("score", False)]),
             ("dr", "dense_rank", None, [("code", True), ("qty", False)]),
             ("rn", "row_number", None, shared),
             ("cs", "cumsum", "score", shared),
             ("sm", "sum", "score"), ("av", "avg", "score"),
             ("mn", "min", "score"), ("mx", "max", "qty")]
    plans = [Window(Scan(t), ["part"], specs) for t in ("t", "big")]
    plans.append(Window(Scan("t"), [],
                        [("rk", "rank", None, [("score", True)])]))
    cpu = Engine({}, device="cpu")
    cpu.register("t", _routing_frame("cpu", 2000))
    cpu.register("big", _routing_frame("cpu", 3000))
    want = [cpu.run(p).to_rows() for p in plans]
    gpu = Engine({}, device="cuda")
    gpu.register("t", _routing_frame("cuda", 2000))
    gpu.register("big", _routing_frame("cuda", 3000))

    def boom(*a, **k):
        raise AssertionError("the torch window expression must not run")

    monkeypatch.setattr(torch, "cumsum", boom)
    monkeypatch.setattr(torch, "cummax", boom)
    monkeypatch.setattr(torch.Tensor, "index_add_", boom)
    monkeypatch.setattr(torch.Tensor, "scatter_reduce_", boom)
    calls = []
    real = Engine._argsort

    def counting(self, f, by):
        calls.append(list(by))
        return real(self, f, by)

    monkeypatch.setattr(Engine, "_argsort", counting)
    got = []
    for p in plans:
        del calls[:]
        got.append(gpu.run(p).to_rows())
        if len(p.funcs) > 1:
            # eight specs, four distinct orders (the four aggregates have
            # none): specs that share an order share its sort
            assert len(calls) == 4
            assert sum(c == [("part", True)] + shared for c in calls) == 1
    monkeypatch.undo()
    for g, w in zip(got, want):
        assert len(g) == len(w)
        assert [repr(r) for r in g] == [repr(r) for r in w]
