"""Narrow (8-byte slot) join table: every case compares sorted
(probe_idx, build_idx) pairs with the generic table's inner_join."""
import random

import pytest
import torch

from spark_rapids_jni_amd.columnar import Column, DType, Table

pytestmark = pytest.mark.gpu

INT64_MIN, INT64_MAX = -2**63, 2**63 - 1


def _sorted_pairs(bi, pi):
    return sorted(zip(pi.cpu().tolist(), bi.cpu().tolist()))


def _generic_pairs(build, probe):
    from spark_rapids_jni_amd.ops.join import HashJoinTable
    bi, pi = HashJoinTable.build(build, force_generic=True).inner_join(probe)
    return _sorted_pairs(bi, pi)


def _i64(vals):
    return Column.from_pylist(vals, DType.INT64, "cuda")


class _Spy:
    """Forwards to the native module and records (name, args) of each call."""

    def __init__(self, mod):
        self._mod = mod
        self.calls = []

    def __getattr__(self, name):
        fn = getattr(self._mod, name)

        def wrapped(*args):
            self.calls.append((name, args))
            return fn(*args)
        return wrapped


@pytest.fixture(scope="module")
def forced_case():
    """Case 1 inputs and their reference pairs, computed once."""
    rnd = random.Random(11)
    kmin = -7
    bvals = [rnd.randint(kmin, kmin + 1500) if rnd.random() > 0.02 else None
             for _ in range(3000)]
    bvals[5] = kmin            # offset 0 is a real key here
    bvals[6] = kmin + 1500
    pvals = [rnd.randint(kmin - 50, kmin + 2000) if rnd.random() > 0.02
             else None for _ in range(9001)]
    pvals[0] = kmin
    b, p = _i64(bvals), _i64(pvals)
    return b, p, _generic_pairs(b, p)


@pytest.mark.parametrize("hint", [None, "exact", "small"])
def test_forced_narrow_int64(forced_case, hint):
    from spark_rapids_jni_amd.ops.join import HashJoinTable
    b, p, ref = forced_case
    tbl = HashJoinTable.build(b, narrow=True)
    assert tbl.layout == "narrow" and tbl.i64_fast
    assert tbl.kmin == -7 and tbl.capacity == 16384
    assert tbl.slots.numel() == tbl.capacity
    out_hint = {None: None, "exact": len(ref), "small": len(ref) // 3}[hint]
    bi, pi = tbl.inner_join(p, out_hint=out_hint)
    assert len(ref) > 9001  # duplicates: more pairs than probe rows
    assert _sorted_pairs(bi, pi) == ref


def test_offset_zero_does_not_match_empty_slots():
    """kmin comes from the dtype (-2^31) and is not a build key, so a probe
    of kmin has offset 0, the same low word as an empty slot."""
    from spark_rapids_jni_amd.ops.join import HashJoinTable
    for nb in (5, 3000):       # 5 rows in 64 slots: a mostly empty table
        bk = torch.arange(1, nb + 1, dtype=torch.int32, device="cuda") * 7
        b = Column.from_torch(bk)
        tbl = HashJoinTable.build(b)
        assert tbl.layout == "narrow" and tbl.kmin == -2**31
        only_kmin = Column.from_torch(torch.full(
            (1000,), -2**31, dtype=torch.int32, device="cuda"))
        bi, pi = tbl.inner_join(only_kmin)
        assert bi.numel() == 0 and pi.numel() == 0
        mixed = Column.from_torch(torch.tensor(
            [-2**31, 7, -2**31, 14, 0, 7 * nb], dtype=torch.int32,
            device="cuda"))
        bi, pi = tbl.inner_join(mixed)
        assert _sorted_pairs(bi, pi) == [(1, 0), (3, 1), (5, nb - 1)]
        assert _sorted_pairs(bi, pi) == _generic_pairs(b, mixed)
    # packed two-key table: kmin = 0 is the packed value of (min1, min2),
    # which no build row has
    b1 = [0, 1, 1, 2]
    b2 = [5, 4, 5, 5]          # (0, 4) -> packed 0 is absent
    bt = Table([Column.from_pylist(b1, DType.INT32, "cuda"),
                Column.from_pylist(b2, DType.INT32, "cuda")])
    pt = Table([Column.from_pylist([0, 0, 2, 0], DType.INT32, "cuda"),
                Column.from_pylist([4, 5, 5, 4], DType.INT32, "cuda")])
    tbl = HashJoinTable.build(bt)
    assert tbl.layout == "narrow" and tbl.kmin == 0
    bi, pi = tbl.inner_join(pt)
    assert _sorted_pairs(bi, pi) == [(1, 0), (2, 3)]
    assert _sorted_pairs(bi, pi) == _generic_pairs(bt, pt)


def test_probe_keys_do_not_alias_through_truncation():
    from spark_rapids_jni_amd.ops.join import HashJoinTable
    rnd = random.Random(3)
    bvals = [rnd.randint(-1000, 1000) for _ in range(500)]
    pvals = []
    for k in bvals[:200]:
        pvals += [k + 2**32, k, k - 2**32]
    pvals += [INT64_MIN, INT64_MAX, INT64_MIN + 1, INT64_MAX - 1]
    b, p = _i64(bvals), _i64(pvals)
    tbl = HashJoinTable.build(b, narrow=True)
    assert tbl.layout == "narrow"
    bi, pi = tbl.inner_join(p)
    got = _sorted_pairs(bi, pi)
    assert got == _generic_pairs(b, p)
    # only the middle row of each triple matches
    assert got and all(j % 3 == 1 and j < 600 for j, _ in got)


def test_range_edge():
    from spark_rapids_jni_amd.ops import join as J
    lo = -2**40
    assert J._fits_narrow(lo, lo + 2**32 - 1)
    assert not J._fits_narrow(lo, lo + 2**32)
    assert not J._fits_narrow(INT64_MIN, INT64_MAX)
    # a span of exactly 2^32 - 1: both ends land in the table and match
    bvals = [lo, lo + 2**32 - 1, lo + 17, lo + 2**31]
    b = _i64(bvals)
    tbl = J.HashJoinTable.build(b, narrow=True)
    assert tbl.layout == "narrow" and tbl.kmin == lo
    p = _i64(bvals + [lo - 1, lo + 2**32, lo + 2**32 + 17, lo - 2**32 + 17])
    bi, pi = tbl.inner_join(p)
    assert _sorted_pairs(bi, pi) == [(0, 0), (1, 1), (2, 2), (3, 3)]
    assert _sorted_pairs(bi, pi) == _generic_pairs(b, p)
    # one more and it no longer fits
    wide = _i64([lo, lo + 2**32])
    with pytest.raises(ValueError):
        J.HashJoinTable.build(wide, narrow=True)
    assert J.HashJoinTable.build(wide).layout == "wide"


def test_auto_rule_at_scan_threshold():
    """From NARROW_SCAN_MIN_ROWS rows an int64 build is range-scanned: a
    span below 2^32 goes narrow, a span of exactly 2^32 stays wide."""
    from spark_rapids_jni_amd.ops import join as J
    n = J.NARROW_SCAN_MIN_ROWS
    keys = torch.arange(n, dtype=torch.int64, device="cuda") * 3 + 100
    probe = Column.from_torch(torch.tensor(
        [100, 101, 103, 3 * (n - 1) + 100, 3 * n + 100, 100 + 2**32],
        dtype=torch.int64, device="cuda"))
    tbl = J.HashJoinTable.build(Column(DType.INT64, n, keys))
    assert tbl.layout == "narrow" and tbl.kmin == 100
    bi, pi = tbl.inner_join(probe)
    assert _sorted_pairs(bi, pi) == [(0, 0), (2, 1), (3, n - 1)]
    keys[-1] = 100 + 2**32
    tbl = J.HashJoinTable.build(Column(DType.INT64, n, keys))
    assert tbl.layout == "wide"
    assert tbl.slots.numel() == 2 * tbl.capacity
    bi, pi = tbl.inner_join(probe)
    assert _sorted_pairs(bi, pi) == [(0, 0), (2, 1), (5, n - 1)]
    with pytest.raises(ValueError):
        J.HashJoinTable.build(Column(DType.INT64, n, keys), narrow=True)


def test_chains_of_duplicates():
    from spark_rapids_jni_amd.ops.join import HashJoinTable
    rnd = random.Random(5)
    distinct = [1000 + 37 * i for i in range(64)]
    bvals = distinct * 64
    rnd.shuffle(bvals)
    b = _i64(bvals)
    tbl = HashJoinTable.build(b, narrow=True)
    assert tbl.layout == "narrow"
    pvals = [rnd.choice(distinct) if rnd.random() < 0.7
             else rnd.randint(900, 4000) for _ in range(203)]
    p = _i64(pvals)
    ref = _generic_pairs(b, p)
    assert len(ref) >= 64 * 100
    for hint in (None, len(ref), 10):
        bi, pi = tbl.inner_join(p, out_hint=hint)
        assert _sorted_pairs(bi, pi) == ref


def test_one_batch_mixed_match_counts():
    """Eight probe rows, one lane's batch: 0, 1 and 64 matches mixed."""
    from spark_rapids_jni_amd.ops.join import HashJoinTable
    bvals = [50] * 64 + [60] + [70 + i for i in range(20)]
    b = _i64(bvals)
    tbl = HashJoinTable.build(b, narrow=True)
    p = _i64([50, 60, 61, 50, 0, 60, 71, 49])
    ref = _generic_pairs(b, p)
    assert len(ref) == 64 + 1 + 64 + 1 + 1
    for hint in (None, len(ref), 1):
        bi, pi = tbl.inner_join(p, out_hint=hint)
        assert _sorted_pairs(bi, pi) == ref


def test_build_matches_agree_with_wide(forced_case):
    from spark_rapids_jni_amd.ops.join import HashJoinTable
    b, p, ref = forced_case
    nt = HashJoinTable.build(b, narrow=True)
    wt = HashJoinTable.build(b, narrow=False)
    assert nt.layout == "narrow" and wt.layout == "wide"
    nb, npi, nm = nt.inner_join(p, track_build_matches=True)
    wb, wpi, wm = wt.inner_join(p, track_build_matches=True)
    assert _sorted_pairs(nb, npi) == ref == _sorted_pairs(wb, wpi)
    assert torch.equal(nm, wm)
    assert 0 < int(nm.sum().item()) < b.size
    # capacity-0 mark-only probe
    assert torch.equal(nt.mark_matches(p), wm)
    assert torch.equal(wt.mark_matches(p), wm)


def test_int32_columns_are_read_in_place(monkeypatch):
    from spark_rapids_jni_amd import _native
    from spark_rapids_jni_amd.ops.join import HashJoinTable
    n = 40_000
    gen = torch.Generator(device="cuda").manual_seed(9)
    bk = torch.randint(-2**31, 2**31 - 1, (n,), dtype=torch.int32,
                       device="cuda", generator=gen)
    bk[0], bk[1] = -2**31, 2**31 - 1
    pk = torch.cat([bk[:n // 2],
                    torch.randint(-2**31, 2**31 - 1, (n,), dtype=torch.int32,
                                  device="cuda", generator=gen)])
    b, p = Column.from_torch(bk), Column.from_torch(pk)
    ref = _generic_pairs(b, p)
    spy = _Spy(_native.gpu())
    monkeypatch.setattr(_native, "gpu", lambda: spy)
    tbl = HashJoinTable.build(b)
    bi, pi = tbl.inner_join(p)
    monkeypatch.undo()
    assert tbl.layout == "narrow" and tbl.kmin == -2**31
    assert _sorted_pairs(bi, pi) == ref and len(ref) >= n // 2
    names = [c[0] for c in spy.calls]
    assert names == ["join_build_n32", "join_probe_n32", "join_probe_n32"]
    # (keys pointer, key_i32): the kernels got the int32 columns themselves
    assert spy.calls[0][1][:2] == (b.data.data_ptr(), 1)
    for _, args in spy.calls[1:]:
        assert args[:2] == (p.data.data_ptr(), 1)
    # an int64 probe column of the same values against the same table (the
    # generic table compares key bytes, so its probe keeps the build's dtype)
    p64 = Column.from_torch(pk[:1000].to(torch.int64))
    bi, pi = tbl.inner_join(p64)
    assert _sorted_pairs(bi, pi) == \
        _generic_pairs(b, Column.from_torch(pk[:1000].clone()))


def test_packed_two_key_join_is_narrow():
    from spark_rapids_jni_amd.ops.join import HashJoinTable
    n = 30_000
    b1 = [i % 500 for i in range(n)]
    b2 = [None if i % 23 == 9 else (i * 7) % 40 - 20 for i in range(n)]
    p1 = b1[:n // 2] + [(i * 3) % 700 for i in range(n // 2)]
    p2 = b2[:n // 2] + [None if i % 17 == 3 else (i * 5) % 44 - 22
                        for i in range(n // 2)]
    bt = Table([Column.from_pylist(b1, DType.INT32, "cuda"),
                Column.from_pylist(b2, DType.INT64, "cuda")])
    pt = Table([Column.from_pylist(p1, DType.INT32, "cuda"),
                Column.from_pylist(p2, DType.INT64, "cuda")])
    tbl = HashJoinTable.build(bt)
    assert tbl.layout == "narrow" and tbl.kmin == 0
    assert getattr(tbl, "_pack", None) is not None
    bi, pi = tbl.inner_join(pt)
    assert bi.numel() > 0
    assert _sorted_pairs(bi, pi) == _generic_pairs(bt, pt)
    # a width product past 2^32 keeps the wide table
    wide = Table([Column.from_pylist([0, 2**20], DType.INT64, "cuda"),
                  Column.from_pylist([0, 2**20], DType.INT64, "cuda")])
    wt = HashJoinTable.build(wide)
    assert wt.layout == "wide" and wt._pack is not None
    with pytest.raises(ValueError):
        HashJoinTable.build(wide, narrow=True)


def test_empty_build_and_empty_probe():
    from spark_rapids_jni_amd.ops.join import HashJoinTable
    empty32 = Column.from_torch(torch.empty(0, dtype=torch.int32,
                                            device="cuda"))
    empty64 = Column.from_torch(torch.empty(0, dtype=torch.int64,
                                            device="cuda"))
    some32 = Column.from_torch(torch.arange(100, dtype=torch.int32,
                                            device="cuda"))
    some64 = Column.from_torch(torch.arange(100, dtype=torch.int64,
                                            device="cuda"))
    for build, probe in ((empty32, some32), (some32, empty32),
                         (empty32, empty32)):
        tbl = HashJoinTable.build(build)
        assert tbl.layout == "narrow"
        bi, pi = tbl.inner_join(probe)
        assert bi.numel() == 0 and pi.numel() == 0
        assert tbl.mark_matches(probe).numel() == build.size
    for build, probe in ((empty64, some64), (some64, empty64)):
        tbl = HashJoinTable.build(build, narrow=True)
        assert tbl.layout == "narrow"
        bi, pi = tbl.inner_join(probe, out_hint=4)
        assert bi.numel() == 0 and pi.numel() == 0


def test_auto_rule_small_int64_build_is_wide():
    """Below NARROW_SCAN_MIN_ROWS an int64 build keeps the 16-byte layout
    (callers hand tbl.slots of such a build to join_probe_i64 directly)."""
    from spark_rapids_jni_amd.ops import join as J
    assert J.NARROW_SCAN_MIN_ROWS > 200_000
    n = 200_000
    keys = torch.randint(0, n // 2, (n,), dtype=torch.int64, device="cuda")
    tbl = J.HashJoinTable.build(Column(DType.INT64, n, keys))
    assert tbl.layout == "wide" and tbl.i64_fast
    assert tbl.slots.numel() == 2 * tbl.capacity
