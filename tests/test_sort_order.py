"""Sort order (ops/sort.py): sort_order_tensors, key_change_flags and the
table-level sort_order / sort_by_key, plus their routing into NDS Sort and
Window.

Comparisons are exact equality of the permutation. The oracle lives here
and uses neither the op nor torch's sort: per key, numpy integer codes
(`np.unique(x, return_inverse=True)`: NaN sorts last, all NaNs and both
zeros are equal), negated for descending and zeroed on null rows, plus a
null-flag array per key; the permutation is `np.lexsort` over
`[code_k, flag_k, ..., code_1, flag_1]`. lexsort is stable, so the expected
permutation is unique.
"""
import itertools

import numpy as np
import pytest
import torch

from spark_rapids_jni_amd.columnar import Column, DType, Table
from spark_rapids_jni_amd.nds.expr import Val
from spark_rapids_jni_amd.nds.plan import Engine, Frame, Scan, Sort, Window
from spark_rapids_jni_amd.ops import sort as S

INT_DTYPES = [torch.int8, torch.int16, torch.int32, torch.int64]
FLOAT_DTYPES = [torch.float32, torch.float64]
ALL_DTYPES = [torch.bool, torch.uint8] + INT_DTYPES + FLOAT_DTYPES


# ---------------------------------------------------------------------------
# oracle
# ---------------------------------------------------------------------------

def _lists(nk, valids, ascending, nulls_first):
    valids = [None] * nk if valids is None else list(valids)
    asc = [True] * nk if ascending is None else list(ascending)
    nf = list(asc) if nulls_first is None else \
        [a if f is None else f for a, f in zip(asc, nulls_first)]
    return valids, asc, nf


def _codes_flags(keys, valids=None, ascending=None, nulls_first=None):
    """Per key: (int64 codes, null flags) as numpy arrays."""
    valids, asc, nf = _lists(len(keys), valids, ascending, nulls_first)
    out = []
    for k, v, a, f in zip(keys, valids, asc, nf):
        x = k.detach().cpu().numpy()
        codes = np.unique(x, return_inverse=True)[1].astype(np.int64)
        codes = codes.reshape(-1)
        if not a:
            codes = -codes
        n = x.shape[0]
        if v is None:
            flags = np.zeros(n, dtype=np.int64)
        else:
            valid = v.detach().cpu().numpy() != 0
            codes = np.where(valid, codes, 0)
            flags = np.where(valid, 1, 0) if f else np.where(valid, 0, 1)
        out.append((codes, flags.astype(np.int64)))
    return out


def oracle(keys, valids=None, ascending=None, nulls_first=None):
    cf = _codes_flags(keys, valids, ascending, nulls_first)
    n = keys[0].numel()
    if n == 0:
        return torch.zeros(0, dtype=torch.int64)
    arrs = []
    for codes, flags in reversed(cf):
        arrs += [codes, flags]
    return torch.from_numpy(np.lexsort(arrs).astype(np.int64))


def check(keys, valids=None, ascending=None, nulls_first=None, key_bits=None):
    got = S.sort_order_tensors(keys, valids, ascending, nulls_first, key_bits)
    assert got.dtype == torch.int64 and got.device == keys[0].device
    want = oracle(keys, valids, ascending, nulls_first)
    assert torch.equal(got.cpu(), want)
    return got


# ---------------------------------------------------------------------------
# inputs (generated on the host, seeded, then moved)
# ---------------------------------------------------------------------------

def _gen(seed):
    return torch.Generator().manual_seed(seed)


def make_key(dtype, n, seed, dev, distinct=50):
    """Few distinct values (many ties) seeded with the dtype's extremes."""
    g = _gen(seed)
    if dtype == torch.bool:
        return (torch.rand(n, generator=g) < 0.5).to(dev)
    if dtype == torch.uint8:
        x = torch.randint(0, 256, (n,), generator=g).to(torch.uint8)
        x[:3] = torch.tensor([0, 255, 128], dtype=torch.uint8)[:n]
        return x.to(dev)
    if dtype in INT_DTYPES:
        ii = torch.iinfo(dtype)
        x = torch.randint(-distinct, distinct, (n,), generator=g).to(dtype)
        ext = torch.tensor([ii.min, ii.max, 0, -1, ii.min, ii.max],
                           dtype=dtype)
        pos = torch.randperm(n, generator=g)[:ext.numel()]
        x[pos] = ext[:pos.numel()]
        return x.to(dev)
    fi = torch.finfo(dtype)
    iv = torch.int32 if dtype == torch.float32 else torch.int64
    x = torch.randint(-distinct, distinct, (n,), generator=g).to(dtype) / 4
    # a NaN with another payload and the sign set
    odd_nan = torch.tensor([-1], dtype=iv).view(dtype)
    sub = torch.tensor([1], dtype=iv).view(dtype)  # smallest subnormal
    ext = torch.cat([
        torch.tensor([0.0, -0.0, float("inf"), float("-inf"), float("nan"),
                      fi.max, -fi.max, float("nan"), -0.0, 0.0], dtype=dtype),
        odd_nan, sub, -sub, odd_nan])
    pos = torch.randperm(n, generator=g)[:ext.numel()]
    x[pos] = ext[:pos.numel()]
    return x.to(dev)


def make_valid(n, seed, dev, p_null=0.3):
    return (torch.rand(n, generator=_gen(seed)) >= p_null).to(dev)


def garbage_nulls(x, valid, seed):
    """Null rows carry arbitrary data; it must not influence the order."""
    if x.dtype == torch.bool:
        return x
    junk = make_key(x.dtype, x.numel(), seed + 1000, x.device, distinct=100)
    return torch.where(valid, x, junk)


# ---------------------------------------------------------------------------
# shared case bodies (CPU tier and GPU tier run the same ones)
# ---------------------------------------------------------------------------

def run_dtype_case(dtype, n, dev):
    x = make_key(dtype, n, 7, dev)
    v = make_valid(n, 8, dev)
    xg = garbage_nulls(x, v, 9)
    for asc, nf in itertools.product([True, False], [True, False]):
        check([x], None, [asc], [nf])
        check([xg], [v], [asc], [nf])
    check([xg], [v.to(torch.uint8) * 2])       # defaults, non-bool validity
    check([xg], [v], [False])                  # desc defaults to nulls last


def run_min_next_to_nulls(dev):
    """Nulls order strictly before a valid iinfo.min (and strictly after a
    valid iinfo.max when descending): a fill value cannot do that."""
    for dtype in INT_DTYPES:
        ii = torch.iinfo(dtype)
        x = torch.tensor([ii.min, 5, ii.min, 0, ii.max, ii.min, ii.max, 3],
                         dtype=dtype, device=dev)
        v = torch.tensor([1, 1, 0, 1, 0, 1, 1, 0], dtype=torch.bool,
                         device=dev)
        got = check([x], [v]).tolist()
        assert got[:3] == [2, 4, 7]            # the nulls, in input order
        assert got[3:5] == [0, 5]              # then the valid minima
        got = check([x], [v], [False]).tolist()
        assert got[:1] == [6] and got[-3:] == [2, 4, 7]
    for dtype in FLOAT_DTYPES:
        x = torch.tensor([float("-inf"), 1.0, 0.0, float("-inf")],
                         dtype=dtype, device=dev)
        v = torch.tensor([1, 1, 0, 0], dtype=torch.bool, device=dev)
        assert check([x], [v]).tolist() == [2, 3, 0, 1]


def packing_cases(n, dev):
    """(name, keys, valids, ascending, key_bits)"""
    k = lambda dt, s: make_key(dt, n, s, dev, distinct=3)
    v = lambda s: make_valid(n, s, dev)
    hinted = torch.randint(0, 1024, (n,), generator=_gen(40)).to(dev)
    return [
        ("64 bits", [k(torch.int32, 1), k(torch.int32, 2)], None, None, None),
        ("65 bits", [k(torch.int32, 3), k(torch.int32, 4)], [v(5), None],
         None, None),
        ("two nullable int64", [k(torch.int64, 6), k(torch.int64, 7)],
         [v(8), v(9)], None, None),
        ("129 bits", [k(torch.int64, 16), k(torch.int64, 17)], [v(18), None],
         None, None),
        ("five mixed keys",
         [k(torch.int8, 10), k(torch.bool, 11), k(torch.int16, 12),
          k(torch.float32, 13), k(torch.int64, 14)],
         [None, None, v(15), None, None],
         [True, True, True, False, True], None),
        ("17 int8", [make_key(torch.int8, n, 20 + i, dev, distinct=1)
                     for i in range(17)], None, None, None),
        ("key_bits=10", [hinted], None, None, [10]),
        ("no hint", [hinted], None, None, None),
    ]


def run_packing(n, dev):
    got = {}
    for name, keys, valids, asc, bits in packing_cases(n, dev):
        got[name] = check(keys, valids, asc, None, bits)
    assert torch.equal(got["key_bits=10"], got["no hint"])


def run_stability(dev):
    x = torch.tensor([5, 3] * 3000, dtype=torch.int64, device=dev)
    want = torch.cat([torch.arange(1, 6000, 2), torch.arange(0, 6000, 2)])
    assert torch.equal(check([x]).cpu(), want)
    const = torch.full_like(x, 7)
    assert torch.equal(check([const, x]).cpu(), want)
    assert torch.equal(check([const]).cpu(), torch.arange(6000))


def run_direction(n, dev):
    x = make_key(torch.int32, n, 31, dev, distinct=5)
    asc = check([x], None, [True])
    desc = check([x], None, [False])
    assert not torch.equal(desc, asc.flip(0))  # ties keep input order


# ---------------------------------------------------------------------------
# CPU tier
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", ALL_DTYPES, ids=str)
def test_cpu_dtypes(dtype):
    run_dtype_case(dtype, 300, "cpu")


def test_cpu_min_next_to_nulls():
    run_min_next_to_nulls("cpu")


def test_cpu_packing_sets():
    run_packing(300, "cpu")


def test_cpu_stability_and_direction():
    run_stability("cpu")
    run_direction(300, "cpu")


def test_cpu_key_change_flags():
    _run_key_change(65, "cpu")


def test_cpu_empty_and_single():
    for n in (0, 1):
        x = torch.zeros(n, dtype=torch.int32)
        assert S.sort_order_tensors([x]).tolist() == list(range(n))


def test_argument_validation():
    a = torch.arange(8)
    with pytest.raises(TypeError):
        S.sort_order_tensors([a.to(torch.float16)])
    with pytest.raises(TypeError):
        S.sort_order_tensors([[1, 2, 3]])
    with pytest.raises(TypeError):
        S.sort_order_tensors([a], [torch.ones(8, dtype=torch.int32)])
    with pytest.raises(ValueError):
        S.sort_order_tensors([a, torch.arange(9)])
    with pytest.raises(ValueError):
        S.sort_order_tensors([a.view(2, 4)])
    with pytest.raises(ValueError):
        S.sort_order_tensors([a], [torch.ones(9, dtype=torch.bool)])
    with pytest.raises(ValueError):
        S.sort_order_tensors([a], ascending=[True, False])
    with pytest.raises(ValueError):
        S.sort_order_tensors([])
    for bad in (0, 65, -1):
        with pytest.raises(ValueError):
            S.sort_order_tensors([a], key_bits=[bad])
    with pytest.raises(ValueError):
        S.sort_order_tensors([a.to(torch.float64)], key_bits=[8])
    with pytest.raises(TypeError):
        S.key_change_flags([a], torch.arange(8, dtype=torch.int32))
    with pytest.raises(ValueError):
        S.key_change_flags([a], torch.arange(8).view(2, 4))
    t = Table([Column.from_torch(a)])
    with pytest.raises(ValueError):
        S.sort_order(t, ascending=[True, True])
    with pytest.raises(ValueError):
        S.sort_by_key(Table([Column.from_torch(torch.arange(9))]), t)
    with pytest.raises(NotImplementedError, match="STRING"):
        S.sort_order(Table([Column.from_pylist(["a", "b"], DType.STRING)]))


def test_cpu_table_level():
    _run_table("cpu")


# ---------------------------------------------------------------------------
# GPU tier
# ---------------------------------------------------------------------------

# 2048/2049: one-workgroup path / tiled path. 2048 * 2048 + 1: the first
# size at which the tile loop strides the grid.
SIZES = [0, 1, 2, 63, 64, 65, 2047, 2048, 2049, 4097, 2048 * 2048 + 1]


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_sizes(n):
    x = torch.randint(0, 1000, (n,), generator=_gen(n),
                      dtype=torch.int32).cuda()
    check([x])


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ALL_DTYPES, ids=str)
def test_dtypes_directions_nulls(dtype):
    for n in (2049, 300):
        run_dtype_case(dtype, n, "cuda")


@pytest.mark.gpu
def test_min_next_to_nulls():
    run_min_next_to_nulls("cuda")


@pytest.mark.gpu
@pytest.mark.parametrize("n", [2049, 5000])
def test_packing_boundaries(n):
    run_packing(n, "cuda")


@pytest.mark.gpu
def test_stability():
    run_stability("cuda")


@pytest.mark.gpu
def test_direction_is_not_reversal():
    for n in (300, 2049):
        run_direction(n, "cuda")


@pytest.mark.gpu
def test_misaligned_and_strided():
    n = 2049
    for dt in (torch.int8, torch.int16, torch.int32, torch.int64,
               torch.float64):
        base = make_key(dt, n + 1, 50, "cuda")
        vbase = make_valid(n + 1, 51, "cuda")
        k, v = base[1:], vbase[1:]
        assert k.data_ptr() % 16 != 0
        check([k], [v])
        check([k, base[:-1]], [None, v])
    wide = make_key(torch.int32, 2 * n, 52, "cuda")
    s = wide[::2]
    assert not s.is_contiguous()
    check([s])
    check([s, wide[1::2]], [make_valid(2 * n, 53, "cuda")[::2], None])


def _run_key_change(n, dev):
    a = make_key(torch.int32, n, 60, dev, distinct=3)
    va = make_valid(n, 61, dev)
    a = garbage_nulls(a, va, 62)
    b = make_key(torch.float64, n, 63, dev, distinct=2)
    keys, valids = [a, b], [va, None]
    perm = S.sort_order_tensors(keys, valids)
    want_perm = oracle(keys, valids)
    assert torch.equal(perm.cpu(), want_perm)
    cf = _codes_flags(keys, valids)
    p = want_perm.numpy()

    def expect(nkeys):
        out = np.zeros(n, dtype=bool)
        out[0] = True
        for codes, flags in cf[:nkeys]:
            out[1:] |= codes[p][1:] != codes[p][:-1]
            out[1:] |= flags[p][1:] != flags[p][:-1]
        return torch.from_numpy(out)

    got = S.key_change_flags(keys, perm, valids)
    assert got.dtype == torch.bool and got.shape == (n,)
    assert torch.equal(got.cpu(), expect(2))
    # prefix: only the first of the two sort keys (partition boundaries)
    got1 = S.key_change_flags(keys[:1], perm, valids[:1])
    assert torch.equal(got1.cpu(), expect(1))


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 65, 2049])
def test_key_change_flags(n):
    _run_key_change(n, "cuda")


@pytest.mark.gpu
def test_key_change_flags_more_than_one_launch_and_int64_nulls():
    n = 700
    keys = [make_key(torch.int8, n, 70 + i, "cuda", distinct=1)
            for i in range(17)]
    keys.append(make_key(torch.int64, n, 90, "cuda", distinct=2))
    valids = [None] * 17 + [make_valid(n, 91, "cuda")]
    perm = check(keys, valids)
    cf = _codes_flags(keys, valids)
    p = perm.cpu().numpy()
    want = np.zeros(n, dtype=bool)
    want[0] = True
    for codes, flags in cf:
        want[1:] |= (codes[p][1:] != codes[p][:-1]) | \
            (flags[p][1:] != flags[p][:-1])
    got = S.key_change_flags(keys, perm, valids)
    assert torch.equal(got.cpu(), torch.from_numpy(want))


def _run_table(dev):
    n = 400
    g = _gen(80)
    r = lambda lo, hi: torch.randint(lo, hi, (n,), generator=g).tolist()
    nul = lambda xs, m: [None if i % m == 0 else x for i, x in enumerate(xs)]
    big = 1 << 64
    # negative values whose low words order the other way round
    d128 = [(-3 * big + 5, -3 * big + 1, -big, -1, 0, 1, big + 1,
             2 * big, -big + 7, big - 1)[i % 10] for i in r(0, 10)]
    f64 = [(0.5, -0.0, 0.0, float("inf"), -2.5)[i] for i in r(0, 5)]
    cols = [
        Column.from_pylist(nul(r(-3, 3), 7), DType.INT32, dev),
        Column.from_pylist(nul(r(-10**12, 10**12), 5), DType.DECIMAL64, dev,
                           scale=2),
        Column.from_pylist(nul(d128, 4), DType.DECIMAL128, dev, scale=3),
        Column.from_pylist(r(0, 3), DType.TIMESTAMP_US, dev),
        Column.from_pylist(nul(f64, 6), DType.FLOAT64, dev),
    ]
    # primary keys with few values first, so later keys break ties
    order = [0, 3, 2, 4, 1]
    keys = Table([cols[i] for i in order])
    asc = [True, False, False, True, True]
    nfirst = [None, None, True, False, None]
    rows = list(zip(*[c.to_pylist() for c in keys.columns]))

    def rank(row):
        out = []
        for x, a, f in zip(row, asc, nfirst):
            f = a if f is None else f
            if x is None:
                out += [0 if f else 1, 0]
            else:
                out += [1 if f else 0, x if a else -x]
        return out

    want = sorted(range(n), key=lambda i: rank(rows[i]))  # sorted is stable
    got = S.sort_order(keys, asc, nfirst)
    assert got.dtype == torch.int64 and got.tolist() == want
    if dev != "cpu":  # the table gather is a device kernel
        values = Table(cols + [Column.from_torch(
            torch.arange(n, device=dev))])
        out = S.sort_by_key(values, keys, asc, nfirst)
        assert out.columns[-1].to_pylist() == want
        for c_out, c_in in zip(out.columns, values.columns):
            src = c_in.to_pylist()
            assert [repr(x) for x in c_out.to_pylist()] == \
                [repr(src[i]) for i in want]
    # defaults: all ascending, nulls first
    asc, nfirst = [True] * 5, [None] * 5
    want = sorted(range(n), key=lambda i: rank(rows[i]))
    assert S.sort_order(keys).tolist() == want
    with pytest.raises(NotImplementedError, match="STRING"):
        S.sort_order(Table([cols[0], Column.from_pylist(
            ["s"] * n, DType.STRING, dev)]))


@pytest.mark.gpu
def test_table_level():
    _run_table("cuda")


@pytest.mark.gpu
def test_runs_under_stream_capture():
    n = 5000
    a = make_key(torch.int32, n, 100, "cuda", distinct=4)
    b = make_key(torch.float64, n, 101, "cuda", distinct=20)
    va = make_valid(n, 102, "cuda")
    a2 = make_key(torch.int32, n, 103, "cuda", distinct=4)
    b2 = make_key(torch.float64, n, 104, "cuda", distinct=20)
    va2 = make_valid(n, 105, "cuda")
    want2 = oracle([a2, b2], [va2, None], [True, False])
    S.sort_order_tensors([a, b], [va, None], [True, False])  # warm up
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            out = S.sort_order_tensors([a, b], [va, None], [True, False])
    torch.cuda.current_stream().wait_stream(side)
    a.copy_(a2)
    b.copy_(b2)
    va.copy_(va2)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), want2)


def _routing_frame(dev, n):
    g = _gen(110)
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
def test_routing_without_torch_argsort(monkeypatch):
    plans = [
        Sort(Scan("t"), [("code", False), ("score", True)]),
        Window(Scan("t"), ["part"],
               [("rk", "rank", None, [("score", False)]),
                ("dr", "dense_rank", None, [("code", True), ("qty", False)]),
                ("rn", "row_number", None, [("qty", True), ("score", True)]),
                ("sm", "sum", "qty")]),
    ]
    # every sort of a frame of up to one tile is native; above it, sorts on
    # more than two keys are (Sort adds the other columns as tie-breakers)
    plans.append(Sort(Scan("big"), [("score", False)]))
    cpu = Engine({}, device="cpu")
    cpu.register("t", _routing_frame("cpu", 2000))
    cpu.register("big", _routing_frame("cpu", 3000))
    want = [cpu.run(p).to_rows() for p in plans]
    gpu = Engine({}, device="cuda")
    gpu.register("t", _routing_frame("cuda", 2000))
    gpu.register("big", _routing_frame("cuda", 3000))

    def boom(*a, **k):
        raise AssertionError("torch.argsort must not be called")

    monkeypatch.setattr(torch, "argsort", boom)
    got = [gpu.run(p) for p in plans]
    monkeypatch.undo()
    for g_, w_ in zip(got, want):
        rows = g_.to_rows()
        assert len(rows) == len(w_)
        # NaN != NaN: compare through repr
        assert [repr(x) for x in rows] == [repr(x) for x in w_]
