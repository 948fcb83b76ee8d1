"""Stream compaction (ops/compact.py): nonzero, fused column compaction,
fused multi-column gather and the table-level apply_boolean_mask.

All comparisons are exact; float columns are compared through an integer
view so NaN payloads and -0.0 count. The oracle is torch on the same device:
torch.nonzero(m).view(-1) and t[idx].

The 16-byte row case is passed the way the module documents it: the int64
pair buffer of a DECIMAL128 column (2n elements) viewed as a contiguous
(n, 2) tensor; the output is (k, 2).
"""
import pytest
import torch

from spark_rapids_jni_amd import _native
from spark_rapids_jni_amd.columnar import (Column, DType, Table,
                                           validity_from_bools)
from spark_rapids_jni_amd.nds.expr import Val
from spark_rapids_jni_amd.nds.plan import Frame
from spark_rapids_jni_amd.ops import compact


def _bits(t):
    """Integer view for exact comparison of any dtype."""
    t = t.contiguous()
    if t.dtype == torch.bool:
        return t.to(torch.uint8)
    if t.dtype.is_floating_point or t.dtype.is_complex:
        iv = {2: torch.int16, 4: torch.int32, 8: torch.int64,
              16: torch.int64}[t.element_size()]
        return t.view(iv)
    return t


def _same(a, b):
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype,
                                                       a.shape, b.shape)
    assert torch.equal(_bits(a), _bits(b))


def _oracle_idx(m, v=None):
    keep = m != 0
    if v is not None:
        keep = keep & (v != 0)
    return torch.nonzero(keep, as_tuple=False).view(-1)


# ---------------------------------------------------------------------------
# CPU tier
# ---------------------------------------------------------------------------

def _cpu_inputs(n=300):
    g = torch.Generator().manual_seed(3)
    m = torch.rand(n, generator=g) < 0.4
    v = torch.rand(n, generator=g) < 0.8
    a = torch.randint(-2**40, 2**40, (n,), generator=g)
    b = torch.randn(n, generator=g, dtype=torch.float64)
    c = torch.randint(-100, 100, (n,), generator=g).to(torch.int16)
    return m, v, [a, b, c]


def test_cpu_nonzero_fallback():
    m, v, _ = _cpu_inputs()
    _same(compact.nonzero(m), _oracle_idx(m))
    _same(compact.nonzero(m, v), _oracle_idx(m, v))
    _same(compact.nonzero(m.to(torch.uint8) * 255, v.to(torch.int8) * -1),
          _oracle_idx(m, v))
    e = compact.nonzero(torch.zeros(0, dtype=torch.bool))
    assert e.dtype == torch.int64 and e.numel() == 0


def test_cpu_compact_and_gather_fallback():
    m, v, ts = _cpu_inputs()
    idx = _oracle_idx(m, v)
    outs, k = compact.compact_tensors(ts, m, v)
    assert k == idx.numel()
    for o, t in zip(outs, ts):
        _same(o, t[idx])
    pairs = torch.arange(2 * m.numel()).view(-1, 2)
    (o,), k2 = compact.compact_tensors([pairs], m)
    _same(o, pairs[_oracle_idx(m)])
    assert k2 == int(m.sum())
    g = torch.Generator().manual_seed(4)
    gi = torch.randint(0, m.numel(), (77,), generator=g)
    for o, t in zip(compact.gather_tensors(ts, gi), ts):
        _same(o, t[gi])
    assert compact.gather_tensors([], gi) == []


def test_argument_validation():
    m = torch.ones(8, dtype=torch.bool)
    with pytest.raises(TypeError):
        compact.nonzero(torch.ones(8, dtype=torch.int32))
    with pytest.raises(TypeError):
        compact.nonzero(m, torch.ones(8, dtype=torch.float32))
    with pytest.raises(ValueError):
        compact.nonzero(m, torch.ones(9, dtype=torch.bool))
    with pytest.raises(ValueError):
        compact.nonzero(torch.ones(2, 4, dtype=torch.bool))
    with pytest.raises(TypeError):
        compact.compact_tensors([torch.arange(8)], m.to(torch.int64))
    with pytest.raises(ValueError):
        compact.compact_tensors([torch.arange(9)], m)
    with pytest.raises(ValueError):  # 24-byte rows
        compact.compact_tensors([torch.arange(24).view(8, 3)], m)
    with pytest.raises(TypeError):
        compact.gather_tensors([torch.arange(8)],
                               torch.zeros(3, dtype=torch.int32))
    with pytest.raises(ValueError):
        compact.gather_tensors([torch.arange(8), torch.arange(9)],
                               torch.zeros(3, dtype=torch.int64))
    tbl = Table([Column.from_torch(torch.arange(8))])
    with pytest.raises(ValueError):
        compact.apply_boolean_mask(tbl, torch.ones(7, dtype=torch.bool))
    with pytest.raises(TypeError):
        compact.apply_boolean_mask(tbl, Column.from_torch(torch.arange(8)))


def _frame(device, n=257):
    g = torch.Generator().manual_seed(11)
    a = torch.randint(-2**50, 2**50, (n,), generator=g)
    b = torch.randn(n, generator=g, dtype=torch.float64)
    b[5] = float("nan")
    b[6] = -0.0
    c = torch.randint(0, 7, (n,), generator=g).to(torch.int32)
    va = torch.rand(n, generator=g) < 0.7
    vc = torch.rand(n, generator=g) < 0.9
    m = torch.rand(n, generator=g) < 0.5
    f = Frame({"a": Val(a.to(device), va.to(device)),
               "b": Val(b.to(device)),
               "c": Val(c.to(device), vc.to(device), ["x%d" % i
                                                      for i in range(7)])}, n)
    return f, m.to(device)


def test_cpu_frame_mask_and_gather_unchanged():
    f, m = _frame("cpu")
    idx = torch.nonzero(m, as_tuple=False).view(-1)
    out = f.mask(m)
    assert out.nrows == idx.numel() and out.names() == f.names()
    for name, v in f.cols.items():
        _same(out.cols[name].data, v.data[idx])
        if v.valid is None:
            assert out.cols[name].valid is None
        else:
            _same(out.cols[name].valid, v.valid[idx])
        assert out.cols[name].dict is v.dict
    perm = torch.randperm(f.nrows, generator=torch.Generator().manual_seed(1))
    out = f.gather(perm[:100])
    assert out.nrows == 100
    for name, v in f.cols.items():
        _same(out.cols[name].data, v.data[perm[:100]])


# ---------------------------------------------------------------------------
# GPU tier
# ---------------------------------------------------------------------------

def _geom():
    g = _native.gpu()
    return (g.compact_tile_rows(), g.compact_max_grid(),
            g.compact_scan_chunk(), g.compact_max_cols())


def _sizes():
    # evaluated lazily: the extension may be absent where GPU tests skip
    T, G, S, _C = _geom()
    return [0, 1, 63, 64, 65, 255, 256, 257, T - 1, T, T + 1, 3 * T + 17,
            S * T + T + 5, (G + 1) * T + 17]


def _patterns(n, dev):
    g = torch.Generator(device=dev)
    g.manual_seed(1234 + n)
    pats = {"none": torch.zeros(n, dtype=torch.bool, device=dev),
            "all": torch.ones(n, dtype=torch.bool, device=dev)}
    if n:
        first = torch.zeros(n, dtype=torch.bool, device=dev)
        first[0] = True
        last = torch.zeros(n, dtype=torch.bool, device=dev)
        last[n - 1] = True
        pats["first"] = first
        pats["last"] = last
    pats["alt"] = (torch.arange(n, device=dev) % 2) == 1
    for d in (0.01, 0.5, 0.99):
        pats[f"rand{d}"] = torch.rand(n, device=dev, generator=g) < d
    return pats


@pytest.mark.gpu
@pytest.mark.parametrize("case", range(14))
def test_nonzero_sizes_and_patterns(case):
    n = _sizes()[case]
    for name, m in _patterns(n, "cuda").items():
        got = compact.nonzero(m)
        assert got.dtype == torch.int64 and got.is_cuda, name
        assert torch.equal(got, _oracle_idx(m)), (n, name)


@pytest.mark.gpu
@pytest.mark.parametrize("case", range(14))
def test_nonzero_dtypes_and_valid(case):
    n = _sizes()[case]
    dev = "cuda"
    g = torch.Generator(device=dev)
    g.manual_seed(99 + n)
    vals = torch.tensor([0, 1, 2, 255], dtype=torch.uint8, device=dev)
    mu8 = vals[torch.randint(0, 4, (n,), device=dev, generator=g)]
    mi8 = torch.where(torch.rand(n, device=dev, generator=g) < 0.5,
                      torch.tensor(-1, dtype=torch.int8, device=dev),
                      torch.tensor(0, dtype=torch.int8, device=dev))
    mb = torch.rand(n, device=dev, generator=g) < 0.5
    v = torch.rand(n, device=dev, generator=g) < 0.7
    for m in (mu8, mi8, mb):
        assert torch.equal(compact.nonzero(m), _oracle_idx(m)), m.dtype
        for vv in (v, v.to(torch.uint8) * 2, v.to(torch.int8) * -1):
            want = torch.nonzero(m.bool() & vv.bool(), as_tuple=False).view(-1)
            assert torch.equal(compact.nonzero(m, vv), want), (m.dtype,
                                                               vv.dtype)


@pytest.mark.gpu
def test_nonzero_misaligned_views():
    T = _geom()[0]
    n = 3 * T + 17
    g = torch.Generator(device="cuda")
    g.manual_seed(5)
    big_m = torch.rand(n + 3, device="cuda", generator=g) < 0.5
    big_v = (torch.rand(n + 3, device="cuda", generator=g) < 0.8).to(
        torch.uint8)
    for om in (1, 3):
        m = big_m[om:om + n]
        assert m.data_ptr() % 4 == om
        assert torch.equal(compact.nonzero(m), _oracle_idx(m))
        for ov in (1, 3):
            v = big_v[ov:ov + n]
            assert torch.equal(compact.nonzero(m, v), _oracle_idx(m, v))
            src = torch.arange(n, device="cuda", dtype=torch.int32)
            (o,), k = compact.compact_tensors([src], m, v)
            _same(o, src[_oracle_idx(m, v)])
    # a strided mask is made contiguous
    ms = big_m[::2]
    assert torch.equal(compact.nonzero(ms), _oracle_idx(ms))


def _columns(n, dev, seed):
    """One tensor of each row width 1, 2, 4, 8, 16 (+ float64 specials)."""
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    r = lambda lo, hi, dt: torch.randint(lo, hi, (n,), device=dev,
                                         generator=g).to(dt)
    f64 = torch.randn(n, device=dev, generator=g, dtype=torch.float64)
    if n:
        f64[::7] = float("nan")
        f64[1::7] = -0.0
        # a NaN with a non-canonical payload
        f64.view(torch.int64)[2::7] = 0x7ff0000000000abc
    dec = torch.randint(-2**62, 2**62, (2 * n,), device=dev, generator=g)
    return [r(-128, 128, torch.int8), r(0, 2, torch.bool),
            r(-2**15, 2**15, torch.int16), r(-2**31, 2**31, torch.int32),
            torch.randn(n, device=dev, generator=g),
            r(-2**62, 2**62, torch.int64), f64, dec.view(n, 2)]


@pytest.mark.gpu
@pytest.mark.parametrize("density", [0.0, 0.01, 0.5, 0.99, 1.0])
def test_compact_tensors_all_widths(density):
    T = _geom()[0]
    n = 3 * T + 17
    dev = "cuda"
    g = torch.Generator(device=dev)
    g.manual_seed(21)
    m = torch.rand(n, device=dev, generator=g) < density
    v = torch.rand(n, device=dev, generator=g) < 0.9
    cols = _columns(n, dev, 8)
    for valid in (None, v):
        idx = _oracle_idx(m, valid)
        outs, k = compact.compact_tensors(cols, m, valid)
        assert k == idx.numel()
        if density == 0.0:
            assert k == 0
        if density == 1.0 and valid is None:
            assert k == n
        for o, t in zip(outs, cols):
            _same(o, t[idx])


@pytest.mark.gpu
def test_compact_tensors_decimal128_column():
    n = 1000
    vals = [(-1) ** i * (i * 10**25 + i) for i in range(n)]
    col = Column.from_pylist(vals, DType.DECIMAL128, "cuda")
    m = (torch.arange(n, device="cuda") % 3) == 0
    (o,), k = compact.compact_tensors([col.data.view(n, 2)], m)
    out = Column(DType.DECIMAL128, k, o.view(-1))
    assert out.to_pylist() == vals[::3]


@pytest.mark.gpu
def test_compact_tensors_more_than_one_launch_and_offset_views():
    T, _G, _S, C = _geom()
    n = T + 300
    dev = "cuda"
    g = torch.Generator(device=dev)
    g.manual_seed(77)
    m = torch.rand(n, device=dev, generator=g) < 0.3
    idx = _oracle_idx(m)
    dts = [torch.int8, torch.int16, torch.int32, torch.int64, torch.float64]
    cols = []
    for i in range(C + 1):
        dt = dts[i % len(dts)]
        big = torch.randint(-100, 100, (n + 5,), device=dev,
                            generator=g).to(dt)
        off = 1 + i % 3   # data_ptr aligned to the element only
        cols.append(big[off:off + n])
    assert any(c.data_ptr() % 16 for c in cols)
    outs, k = compact.compact_tensors(cols, m)
    assert k == idx.numel() and len(outs) == C + 1
    for o, t in zip(outs, cols):
        _same(o, t[idx])
    # the gather takes the same descriptor path
    gi = torch.randint(0, n, (2 * n,), device=dev, generator=g)
    for o, t in zip(compact.gather_tensors(cols, gi), cols):
        _same(o, t[gi])
    # 16-byte rows at 8-byte alignment
    bigp = torch.randint(-2**62, 2**62, (2 * n + 1,), device=dev, generator=g)
    pairs = bigp[1:].view(n, 2)
    assert pairs.data_ptr() % 16 == 8
    (o,), _k = compact.compact_tensors([pairs], m)
    _same(o, pairs[idx])
    (o,) = compact.gather_tensors([pairs], gi)
    _same(o, pairs[gi])


@pytest.mark.gpu
def test_gather_tensors():
    T = _geom()[0]
    n = 2 * T + 5
    dev = "cuda"
    cols = _columns(n, dev, 13)
    g = torch.Generator(device=dev)
    g.manual_seed(2)
    maps = [torch.randint(0, n, (3 * n + 1,), device=dev, generator=g),
            torch.arange(n, device=dev),
            torch.arange(n - 1, -1, -1, device=dev),
            torch.empty(0, dtype=torch.int64, device=dev)]
    for gi in maps:
        outs = compact.gather_tensors(cols, gi)
        for o, t in zip(outs, cols):
            _same(o, t[gi])


@pytest.mark.gpu
def test_gather_tensors_out_of_range_is_zero():
    n = 500
    cols = _columns(n, "cuda", 14)
    gi = torch.tensor([3, n, 4, -1, n - 1, 2**40, 0], device="cuda")
    ok = torch.tensor([1, 0, 1, 0, 1, 0, 1], device="cuda").bool()
    safe = torch.where(ok, gi, torch.zeros_like(gi))
    for o, t in zip(compact.gather_tensors(cols, gi), cols):
        want = t[safe]
        want[~ok] = 0
        _same(o, want)


@pytest.mark.gpu
def test_apply_boolean_mask_table():
    from spark_rapids_jni_amd import exec as ex
    from spark_rapids_jni_amd.ops.copying import gather
    n = 700
    dev = "cuda"
    ints = Column.from_pylist([None if i % 5 == 0 else i * 3
                               for i in range(n)], DType.INT64, dev)
    strs = Column.from_pylist([None if i % 7 == 0 else "s" * (i % 4) + str(i)
                               for i in range(n)], DType.STRING, dev)
    lens = [i % 4 for i in range(n)]
    offs = [0]
    for ln in lens:
        offs.append(offs[-1] + ln)
    child = Column.from_torch(torch.arange(offs[-1], dtype=torch.int32,
                                           device=dev))
    lst = Column(DType.LIST, n, None, None,
                 torch.tensor(offs, dtype=torch.int32, device=dev),
                 children=[child])
    tbl = Table([ints, strs, lst])
    mvals = [None if i % 11 == 0 else (i % 3 != 0) for i in range(n)]
    mcol = Column.from_pylist(mvals, DType.BOOL8, dev)
    keep = [i for i, x in enumerate(mvals) if x]
    want = gather(tbl, torch.nonzero(
        torch.tensor([bool(x) for x in mvals], device=dev),
        as_tuple=False).view(-1))
    got = compact.apply_boolean_mask(tbl, mcol)
    assert got.num_rows == len(keep)
    for gc, wc, src in zip(got.columns, want.columns, tbl.columns):
        assert gc.to_pylist() == wc.to_pylist()
        host = src.to_pylist()
        assert gc.to_pylist() == [host[i] for i in keep]
    # byte-tensor mask, through the exec entry point
    mt = torch.tensor([bool(x) for x in mvals], device=dev)
    got2 = ex.apply_boolean_mask(tbl, mt)
    for gc, wc in zip(got2.columns, want.columns):
        assert gc.to_pylist() == wc.to_pylist()


@pytest.mark.gpu
def test_routing_without_torch_nonzero(monkeypatch):
    from spark_rapids_jni_amd import exec as ex
    f, m = _frame("cuda", n=5000)
    fc, mc = _frame("cpu", n=5000)
    want_rows = fc.mask(mc).to_rows()
    tbl = Table([Column.from_torch(torch.arange(5000, device="cuda"))])

    def boom(*a, **k):
        raise AssertionError("torch.nonzero must not be called")

    monkeypatch.setattr(torch, "nonzero", boom)
    out = f.mask(m)
    t2 = ex.apply_boolean_mask(tbl, m)
    monkeypatch.undo()
    got_rows = out.to_rows()
    assert len(got_rows) == len(want_rows)
    for g_, w_ in zip(got_rows, want_rows):
        # NaN != NaN: compare through repr
        assert repr(g_) == repr(w_)
    assert t2.columns[0].to_pylist() == \
        torch.nonzero(mc, as_tuple=False).view(-1).tolist()
    # gather on the GPU frame equals the CPU frame
    perm = torch.randperm(5000, generator=torch.Generator().manual_seed(9))
    gr = f.gather(perm.cuda()).to_rows()
    cr = fc.gather(perm).to_rows()
    assert [repr(x) for x in gr] == [repr(x) for x in cr]


@pytest.mark.gpu
def test_nonzero_raises_under_capture():
    m = torch.ones(1000, dtype=torch.bool, device="cuda")
    x = torch.zeros(8, device="cuda")
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y = x + 1  # keep the captured graph non-empty
        with pytest.raises(RuntimeError, match="capture"):
            compact.nonzero(m)
        with pytest.raises(RuntimeError, match="capture"):
            compact.compact_tensors([x], m[:8])
    del y


@pytest.mark.gpu
def test_gather_tensors_replays_in_graph():
    from spark_rapids_jni_amd.graphs import CapturedPipeline
    n = 3000
    cols = _columns(n, "cuda", 15)
    g = torch.Generator(device="cuda")
    g.manual_seed(6)
    gi = torch.randint(0, n, (4096,), device="cuda", generator=g)
    # one linear chain: a single fused gather launch
    pipe = CapturedPipeline(lambda idx: compact.gather_tensors(cols, idx),
                            [gi.clone()])
    for _ in range(2):
        gi2 = torch.randint(0, n, (4096,), device="cuda", generator=g)
        outs = pipe.replay(gi2)
        torch.cuda.synchronize()
        for o, t in zip(outs, cols):
            _same(o, t[gi2])
