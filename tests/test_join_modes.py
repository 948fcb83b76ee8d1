"""Semi, anti, left-outer and full-outer probes of a HashJoinTable
(probe_matches, semi_select, left_outer_join, full_outer_join), their native
entry points, their NDS routing and the fused outer-join gather.

The oracle is a Python dict from key to the list of build rows, built on the
CPU; numpy only expands it over the probe rows."""
import numpy as np
import pytest
import torch

from spark_rapids_jni_amd.columnar import Column, DType, Table

pytestmark = pytest.mark.gpu

INT64_MIN, INT64_MAX = -2**63, 2**63 - 1
INT32_MIN, INT32_MAX = -2**31, 2**31 - 1
MASKS = ("none", "some", "all")
# (name, build kwargs, torch key dtype)
LAYOUTS = {
    "wide": (dict(narrow=False), torch.int64),
    "narrow": (dict(narrow=True), torch.int64),
    "narrow_i32": (dict(), torch.int32),
    "dense": (dict(dense=True), torch.int64),
    "dense_i32": (dict(dense=True), torch.int32),
}
DENSE_KMIN, DENSE_RANGE, DENSE_ROWS = -700, 1500, 1000
HASHED_RANGE = 1000  # build keys of the hashed layouts lie in [0, 1000)


def _tile(layout):
    from spark_rapids_jni_amd import _native
    return _native.gpu().JOIN_PROBE_TILE[layout.split("_")[0]]


def _sizes(layout):
    t = _tile(layout)
    return [0, 1, 7, 8, 9, 63, 64, 65, t - 1, t, t + 1, 2 * t + 65]


def _big(layout):
    # the smallest size at which a workgroup takes a second tile
    return 2**22 + _tile(layout) + 65


def _null_mask(rng, n, mask):
    """True = valid; None for no mask."""
    if mask == "none":
        return None
    if mask == "all":
        return np.zeros(n, dtype=bool)
    return rng.random(n) >= 0.1


def _column(keys, valid, dtype):
    t = torch.from_numpy(keys.astype(np.int64)).to(dtype).cuda()
    dt = DType.INT64 if dtype == torch.int64 else DType.INT32
    if valid is None:
        return Column.from_torch(t, dtype=dt)
    return Column.from_torch(t, valid=valid.tolist(), dtype=dt)


def _build_keys(layout, mask):
    """(keys int64 ndarray, valid bool ndarray or None) of the build side."""
    rng = np.random.default_rng(5)
    if layout.startswith("dense"):
        keys = DENSE_KMIN + rng.permutation(DENSE_RANGE)[:DENSE_ROWS]
        # both ends of the range are build keys
        keys[0], keys[1] = DENSE_KMIN, DENSE_KMIN + DENSE_RANGE - 1
        keys = np.unique(keys)
        rng.shuffle(keys)
    else:
        # keys repeated 1, 2 and 5 times and one key repeated 300 times
        distinct = rng.permutation(HASHED_RANGE)[:391]
        reps = np.concatenate([np.full(130, 1), np.full(130, 2),
                               np.full(130, 5), [300]])
        keys = np.repeat(distinct, reps)
        rng.shuffle(keys)
    return keys.astype(np.int64), _null_mask(rng, len(keys), mask)


_TABLES = {}


def _table(layout, mask):
    """(table, oracle dict key -> build rows, build column, n build rows),
    built once per layout and mask."""
    from spark_rapids_jni_amd.ops.join import HashJoinTable
    if (layout, mask) not in _TABLES:
        kwargs, dtype = LAYOUTS[layout]
        keys, valid = _build_keys(layout, mask)
        col = _column(keys, valid, dtype)
        tbl = HashJoinTable.build(col, **kwargs)
        assert tbl.layout == layout.split("_")[0]
        d = {}
        for r, k in enumerate(keys.tolist()):
            if valid is None or valid[r]:
                d.setdefault(k, []).append(r)
        _TABLES[(layout, mask)] = (tbl, d, col, len(keys))
    return _TABLES[(layout, mask)]


def _probe_keys(layout, mask, n, seed=0):
    rng = np.random.default_rng(1000 + seed + n)
    i32 = layout.endswith("_i32")
    if layout.startswith("dense"):
        lo, hi = DENSE_KMIN, DENSE_KMIN + DENSE_RANGE - 1
        keys = rng.integers(lo - 50, hi + 50, n).astype(np.int64)
        special = [lo, hi, lo - 1, hi + 1]
        if i32:
            special += [INT32_MIN, INT32_MAX]
        else:
            special += [lo + 2**32, lo - 2**32, hi + 2**32, hi - 2**32,
                        INT64_MIN, INT64_MAX]
    else:
        # twice the build range: many probes miss into occupied slots
        keys = rng.integers(0, 2 * HASHED_RANGE, n).astype(np.int64)
        special = ([INT32_MIN, INT32_MAX] if i32 else
                   [2**32, -2**32, 5 + 2**32, INT64_MIN, INT64_MAX])
    if n:
        at = rng.permutation(n)[:len(special)]
        keys[at] = np.array(special[:len(at)], dtype=np.int64)
    return keys, _null_mask(rng, n, mask)


class _Oracle:
    """What the dict says about a probe: flags, and the left outer pairs in
    (probe row, build row) order with -1 for an unmatched probe row."""

    def __init__(self, d, nbuild, pkeys, pvalid):
        ukeys = np.array(sorted(d), dtype=np.int64)
        counts = np.array([len(d[k]) for k in sorted(d)], dtype=np.int64)
        flat = np.array([r for k in sorted(d) for r in d[k]], dtype=np.int64)
        starts = np.cumsum(counts) - counts
        n = len(pkeys)
        if len(ukeys) and n:
            pos = np.minimum(np.searchsorted(ukeys, pkeys), len(ukeys) - 1)
            found = ukeys[pos] == pkeys
        else:
            pos = np.zeros(n, dtype=np.int64)
            found = np.zeros(n, dtype=bool)
        if pvalid is not None:
            found &= pvalid
        self.flags = found
        self.semi = np.nonzero(found)[0]
        self.anti = np.nonzero(~found)[0]
        nout = np.where(found, counts[pos] if len(ukeys) else 0, 1)
        self.pi = np.repeat(np.arange(n, dtype=np.int64), nout)
        off = np.arange(nout.sum()) - np.repeat(np.cumsum(nout) - nout, nout)
        fr = np.repeat(found, nout)
        src = np.repeat(starts[pos] if len(ukeys) else pos, nout) + off
        self.bi = np.where(fr, flat[np.where(fr, src, 0)] if len(flat) else -1,
                           -1)
        self.matched_pairs = int(np.where(found, nout, 0).sum())
        self.unmatched_probe = int((~found).sum())
        hit = np.zeros(nbuild, dtype=bool)
        hit[self.bi[self.bi >= 0]] = True
        self.build_matched = hit
        self.unmatched_build = np.nonzero(~hit)[0]


def _dev(a, dtype=torch.int64):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).cuda()


def _sort_pairs(bi, pi, nbuild):
    """Pairs ordered by (probe row, build row); -1 sorts first on both."""
    key = (pi.long() + 1) * (nbuild + 2) + (bi.long() + 1)
    order = torch.sort(key)[1]
    return bi.long()[order], pi.long()[order]


def _assert_pairs(bi, pi, ebi, epi, nbuild):
    sb, sp = _sort_pairs(bi, pi, nbuild)
    eb, ep = _sort_pairs(_dev(ebi), _dev(epi), nbuild)
    assert sb.numel() == eb.numel()
    assert torch.equal(sp, ep) and torch.equal(sb, eb)


def _check_all(tbl, d, nbuild, p, orc, hints=True, composition=True):
    from spark_rapids_jni_amd.ops.join import make_left_outer
    # semi / anti: exactly the oracle's ascending rows
    for anti, exp in ((False, orc.semi), (True, orc.anti)):
        sel = tbl.semi_select(p, anti=anti)
        assert sel.dtype == torch.int64
        assert torch.equal(sel, _dev(exp))
        fl = tbl.probe_matches(p, anti=anti)
        assert fl.dtype == torch.uint8
        assert torch.equal(fl, _dev(orc.flags ^ anti, torch.uint8))
    # left outer
    total = orc.matched_pairs + orc.unmatched_probe
    assert total == len(orc.pi)
    for hint in ((None, total, 10) if hints else (None,)):
        bi, pi, bm = tbl.left_outer_join(p, out_hint=hint,
                                         track_build_matches=True)
        assert bi.dtype == torch.int32 and pi.dtype == torch.int64
        assert bi.numel() == total and pi.numel() == total
        _assert_pairs(bi, pi, orc.bi, orc.pi, nbuild)
        assert torch.equal(bm, tbl.mark_matches(p))
        assert torch.equal(bm.bool(), _dev(orc.build_matched, torch.bool))
    bi2, pi2 = tbl.left_outer_join(p)
    assert bi2.numel() == total
    if composition:
        ib, ip = tbl.inner_join(p)
        assert ib.numel() == orc.matched_pairs
        cb, cp = make_left_outer(len(orc.flags), ib, ip)
        sb, sp = _sort_pairs(bi2, pi2, nbuild)
        tb, tp = _sort_pairs(cb, cp, nbuild)
        assert torch.equal(sb, tb) and torch.equal(sp, tp)
    # full outer: the left outer pairs, then unmatched build rows ascending
    fb, fp = tbl.full_outer_join(p)
    assert fb.dtype == torch.int64 and fp.dtype == torch.int64
    nub = len(orc.unmatched_build)
    assert fb.numel() == total + nub
    assert torch.equal(fb[total:], _dev(orc.unmatched_build))
    assert bool((fp[total:] == -1).all())
    _assert_pairs(fb[:total], fp[:total], orc.bi, orc.pi, nbuild)


def _cases():
    out = []
    for layout in LAYOUTS:
        for mask in MASKS:
            out.append((layout, mask))
    return out


@pytest.mark.parametrize("layout,mask", _cases())
def test_modes_every_size(layout, mask):
    tbl, d, _col, nbuild = _table(layout, mask)
    _kwargs, dtype = LAYOUTS[layout]
    for n in _sizes(layout):
        pkeys, pvalid = _probe_keys(layout, mask, n)
        p = _column(pkeys, pvalid, dtype)
        _check_all(tbl, d, nbuild, p, _Oracle(d, nbuild, pkeys, pvalid))


@pytest.mark.parametrize("layout", ["wide", "narrow", "dense"])
def test_modes_second_tile_of_a_workgroup(layout):
    """2^22 + tile + 65 rows: the grid is capped at 2^22 rows per pass, so
    some workgroups run the tile loop twice."""
    tbl, d, _col, nbuild = _table(layout, "some")
    n = _big(layout)
    pkeys, pvalid = _probe_keys(layout, "some", n)
    t = torch.from_numpy(pkeys).cuda()
    from spark_rapids_jni_amd.ops.aggregate import _validity_from_bool
    p = Column(DType.INT64, n, t, _validity_from_bool(_dev(pvalid,
                                                           torch.bool)),
               null_count=None)
    orc = _Oracle(d, nbuild, pkeys, pvalid)
    assert torch.equal(tbl.semi_select(p), _dev(orc.semi))
    assert torch.equal(tbl.semi_select(p, anti=True), _dev(orc.anti))
    bi, pi, bm = tbl.left_outer_join(p, track_build_matches=True)
    assert bi.numel() == orc.matched_pairs + orc.unmatched_probe
    _assert_pairs(bi, pi, orc.bi, orc.pi, nbuild)
    assert torch.equal(bm.bool(), _dev(orc.build_matched, torch.bool))


def _two_key_case(mask):
    rng = np.random.default_rng(21)
    nb, n = 700, 2048 + 65
    b1, b2 = rng.integers(0, 40, nb), rng.integers(-5, 20, nb)
    p1, p2 = rng.integers(-3, 45, n), rng.integers(-8, 24, n)
    bv1, bv2 = _null_mask(rng, nb, mask), _null_mask(rng, nb, mask)
    pv1, pv2 = _null_mask(rng, n, mask), _null_mask(rng, n, mask)
    return (b1, b2, bv1, bv2), (p1, p2, pv1, pv2)


@pytest.mark.parametrize("mask", MASKS)
def test_modes_packed_two_keys(mask):
    from spark_rapids_jni_amd.ops.join import HashJoinTable
    (b1, b2, bv1, bv2), (p1, p2, pv1, pv2) = _two_key_case(mask)
    bt = Table([_column(b1, bv1, torch.int32), _column(b2, bv2, torch.int64)])
    pt = Table([_column(p1, pv1, torch.int32), _column(p2, pv2, torch.int64)])
    tbl = HashJoinTable.build(bt)
    assert tbl.i64_fast and getattr(tbl, "_pack", None) is not None
    d = {}
    for r in range(len(b1)):
        if (bv1 is None or bv1[r]) and (bv2 is None or bv2[r]):
            d.setdefault(int(b1[r]) * 1000 + int(b2[r]), []).append(r)
    pvalid = None
    if pv1 is not None:
        pvalid = pv1 & pv2
    orc = _Oracle(d, len(b1), p1.astype(np.int64) * 1000 + p2, pvalid)
    _check_all(tbl, d, len(b1), pt, orc)


@pytest.mark.parametrize("kind", ["string", "forced"])
def test_modes_generic_fallback(kind):
    from spark_rapids_jni_amd.ops.join import HashJoinTable
    rng = np.random.default_rng(8)
    bk = rng.integers(0, 300, 500)
    pk = rng.integers(0, 600, 2113)
    bvalid, pvalid = rng.random(500) >= 0.1, rng.random(2113) >= 0.1
    if kind == "string":
        b = Column.from_pylist([f"k{k}" if v else None
                                for k, v in zip(bk, bvalid)], DType.STRING,
                               "cuda")
        p = Column.from_pylist([f"k{k}" if v else None
                                for k, v in zip(pk, pvalid)], DType.STRING,
                               "cuda")
        tbl = HashJoinTable.build(b)
    else:
        b = _column(bk, bvalid, torch.int64)
        p = _column(pk, pvalid, torch.int64)
        tbl = HashJoinTable.build(b, force_generic=True)
    assert tbl.layout == "generic" and not tbl.i64_fast
    d = {}
    for r, k in enumerate(bk.tolist()):
        if bvalid[r]:
            d.setdefault(k, []).append(r)
    _check_all(tbl, d, 500, p, _Oracle(d, 500, pk.astype(np.int64), pvalid))


@pytest.mark.parametrize("layout", ["wide", "narrow", "narrow_i32", "dense",
                                    "dense_i32"])
@pytest.mark.parametrize("anti", [0, 1])
def test_flag_buffer_contract(layout, anti):
    """Through the native entry point: every byte below nprobe is 0 or 1 and
    nothing is written from the padded length on."""
    from spark_rapids_jni_amd import _native
    from spark_rapids_jni_amd.ops.join import PROBE_FLAG, _narrow_keys
    g = _native.gpu()
    stream = _native.current_stream()
    tbl, d, _col, nbuild = _table(layout, "some")
    _kwargs, dtype = LAYOUTS[layout]
    guard = 4096
    for n in (1, 9, _tile(layout) + 1):
        pkeys, pvalid = _probe_keys(layout, "some", n)
        p = _column(pkeys, pvalid, dtype)
        padded = (n + 15) // 16 * 16
        buf = torch.full((padded + guard,), 0xAA, dtype=torch.uint8,
                         device="cuda")
        pv = p.validity.data_ptr()
        if tbl.layout == "wide":
            g.join_probe_mode_i64(p.data.data_ptr(), pv, n,
                                  tbl.slots.data_ptr(), tbl.capacity, 0, 0, 0,
                                  0, 0, 0, PROBE_FLAG, buf.data_ptr(), anti,
                                  stream)
        else:
            data, key_i32 = _narrow_keys(p)
            fn = (g.join_probe_mode_d32 if tbl.layout == "dense"
                  else g.join_probe_mode_n32)
            fn(data.data_ptr(), key_i32, pv, n, tbl.slots.data_ptr(),
               tbl.capacity, tbl.kmin, 0, 0, 0, 0, 0, 0, PROBE_FLAG,
               buf.data_ptr(), anti, stream)
        host = buf.cpu().numpy()
        assert set(np.unique(host[:n]).tolist()) <= {0, 1}
        assert (host[padded:] == 0xAA).all()
        orc = _Oracle(d, nbuild, pkeys, pvalid)
        assert (host[:n] == (orc.flags ^ bool(anti))).all()


# ---------------------------------------------------------------------------
# NDS routing
# ---------------------------------------------------------------------------

class _Spy:
    """Forwards to the native module and records the name of each call."""

    def __init__(self, mod):
        self._mod = mod
        self.calls = []

    def __getattr__(self, name):
        fn = getattr(self._mod, name)
        if not callable(fn):
            return fn

        def wrapped(*args):
            self.calls.append(name)
            return fn(*args)
        return wrapped


def _vals(dtype, seed):
    from spark_rapids_jni_amd.nds.expr import Val
    gen = torch.Generator().manual_seed(seed)
    lk = torch.randint(0, 400, (3001,), generator=gen).to(dtype)
    rk = torch.randint(100, 300, (500,), generator=gen).to(dtype)
    lv = torch.rand(3001, generator=gen) >= 0.1
    rv = torch.rand(500, generator=gen) >= 0.1
    return ([Val(lk.cuda(), lv.cuda())], [Val(rk.cuda(), rv.cuda())],
            [Val(lk, lv)], [Val(rk, rv)])


def _lex(li, ri):
    return sorted(zip(li.cpu().tolist(), ri.cpu().tolist()))


@pytest.mark.parametrize("dtype", [torch.int64, torch.int32])
@pytest.mark.parametrize("how", ["semi", "anti", "left", "full"])
def test_nds_join_routes_to_the_fast_table(monkeypatch, how, dtype):
    from spark_rapids_jni_amd import _native
    from spark_rapids_jni_amd.nds.plan import CpuBackend, GpuBackend
    gl, gr, cl, cr = _vals(dtype, 3)
    spy = _Spy(_native.gpu())
    monkeypatch.setattr(_native, "gpu", lambda: spy)
    li, ri = GpuBackend().join(gl, gr, how, 3001)
    monkeypatch.undo()
    for name in ("join_build", "join_semi", "join_probe_count",
                 "join_probe_fill"):
        assert name not in spy.calls
    assert any(c.startswith("join_probe_mode_") for c in spy.calls)
    eli, eri = CpuBackend().join(cl, cr, how, 3001)
    if how in ("semi", "anti"):
        assert ri is None and torch.equal(li.cpu(), eli)
    else:
        assert _lex(li, ri) == _lex(eli, eri)


@pytest.mark.parametrize("how", ["left", "full"])
def test_nds_ordered_outer_join_keeps_its_row_order(how):
    """matched pairs by (left row, right row), then unmatched left rows
    ascending, then unmatched right rows ascending: inner join, sort,
    make_left_outer / make_full_outer."""
    from spark_rapids_jni_amd.nds.plan import GpuBackend, _val_to_column
    from spark_rapids_jni_amd.ops.join import (HashJoinTable, make_full_outer,
                                               make_left_outer)
    gl, gr, _cl, _cr = _vals(torch.int64, 4)
    li, ri = GpuBackend(ordered_joins=True).join(gl, gr, how, 3001)
    tbl = HashJoinTable.build([_val_to_column(v) for v in gr])
    bi, pi, matched = tbl.inner_join([_val_to_column(v) for v in gl],
                                     track_build_matches=True)
    pairs = list(zip(pi.cpu().tolist(), bi.cpu().tolist()))
    order = sorted(range(len(pairs)), key=pairs.__getitem__)
    order = torch.tensor(order, dtype=torch.int64, device="cuda")
    bi, pi = bi[order], pi[order]
    if how == "left":
        eb, ep = make_left_outer(3001, bi, pi)
    else:
        eb, ep = make_full_outer(matched, bi, pi, 3001)
    assert li.dtype == torch.int64 and ri.dtype == torch.int64
    assert torch.equal(li, ep) and torch.equal(ri, eb)


@pytest.mark.parametrize("with_valid", [False, True])
def test_frame_gather_null_for_neg(with_valid):
    from spark_rapids_jni_amd.nds.expr import Val
    from spark_rapids_jni_amd.nds.plan import Frame
    gen = torch.Generator().manual_seed(12)
    n = 300
    cols = {}
    for name, dt in (("a", torch.int64), ("b", torch.int32),
                     ("c", torch.float64), ("d", torch.int8)):
        data = torch.randint(-50, 50, (n,), generator=gen).to(dt).cuda()
        valid = ((torch.rand(n, generator=gen) >= 0.2).cuda()
                 if with_valid and name != "b" else None)
        cols[name] = Val(data, valid)
    idx = torch.randint(-1, n, (1000,), generator=gen)
    idx[0], idx[1], idx[2] = -1, 0, n - 1
    idx = idx.cuda()
    out = Frame(cols, n).gather(idx, null_for_neg=True)
    assert out.nrows == 1000
    neg = idx < 0
    safe = idx.clamp(min=0)
    for name, v in cols.items():
        o = out.cols[name]
        ev = (v.valid[safe] if v.valid is not None else
              torch.ones(1000, dtype=torch.bool, device="cuda")) & ~neg
        assert o.valid.dtype == torch.bool and torch.equal(o.valid, ev)
        assert o.data.dtype == v.data.dtype
        assert torch.equal(o.data[ev], v.data[safe][ev])
    # the empty side of an outer join: every row null
    empty = Frame({"a": Val(torch.empty(0, dtype=torch.int64, device="cuda"),
                            None)}, 0)
    o = empty.gather(torch.full((5,), -1, dtype=torch.int64, device="cuda"),
                     null_for_neg=True)
    assert o.nrows == 5 and not bool(o.cols["a"].valid.any())


def test_packed_semi_select_packs_its_probe_keys_once(monkeypatch):
    """One pack of the probe keys, with no read-back of its own: the kept-row
    count of the compaction is the only one."""
    from spark_rapids_jni_amd.ops import join as join_mod
    (b1, b2, bv1, bv2), (p1, p2, pv1, pv2) = _two_key_case("some")
    bt = Table([_column(b1, bv1, torch.int32), _column(b2, bv2, torch.int64)])
    pt = Table([_column(p1, pv1, torch.int32), _column(p2, pv2, torch.int64)])
    tbl = join_mod.HashJoinTable.build(bt)
    assert getattr(tbl, "_pack", None) is not None
    calls = []
    real = join_mod._pack_keys

    def counting(cols, mins, widths, drop_all_valid=True):
        calls.append(drop_all_valid)
        return real(cols, mins, widths, drop_all_valid)
    monkeypatch.setattr(join_mod, "_pack_keys", counting)
    for anti in (False, True):
        del calls[:]
        tbl.semi_select(pt, anti=anti)
        assert calls == [False]
        del calls[:]
        tbl.probe_matches(pt, anti=anti)
        assert calls == [False]
    # all valid and in range: the mask is kept, and the result is the same
    inside = Table([_column(b1, None, torch.int32),
                    _column(b2, None, torch.int64)])
    monkeypatch.undo()
    assert torch.equal(tbl.semi_select(inside),
                       torch.sort(tbl.semi_join(inside))[0])


def test_mode_entry_points_reject_other_modes():
    """The inner probe has entry points of its own: mode is 1 or 2, and the
    flag mode needs its buffer."""
    from spark_rapids_jni_amd import _native
    from spark_rapids_jni_amd.ops.join import PROBE_FLAG
    g = _native.gpu()
    tbl, _d, col, _n = _table("wide", "none")
    for mode in (0, 3, -1):
        with pytest.raises(ValueError):
            g.join_probe_mode_i64(col.data.data_ptr(), 0, col.size,
                                  tbl.slots.data_ptr(), tbl.capacity, 0, 0, 0,
                                  0, 0, 0, mode, 0, 0,
                                  _native.current_stream())
    with pytest.raises(ValueError):
        g.join_probe_mode_i64(col.data.data_ptr(), 0, col.size,
                              tbl.slots.data_ptr(), tbl.capacity, 0, 0, 0, 0,
                              0, 0, PROBE_FLAG, 0, 0,
                              _native.current_stream())
