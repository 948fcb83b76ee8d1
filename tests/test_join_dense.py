"""Dense (direct-address) join table: every case compares sorted
(probe_idx, build_idx) pairs with the generic table's inner_join."""
import random

import pytest
import torch

from spark_rapids_jni_amd.columnar import Column, DType

pytestmark = pytest.mark.gpu

INT64_MIN, INT64_MAX = -2**63, 2**63 - 1


def _sorted_pairs(bi, pi):
    return sorted(zip(pi.cpu().tolist(), bi.cpu().tolist()))


def _generic(build):
    from spark_rapids_jni_amd.ops.join import HashJoinTable
    return HashJoinTable.build(build, force_generic=True)


def _generic_pairs(build, probe):
    bi, pi = _generic(build).inner_join(probe)
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


KMIN = -7
SPAN = 2800           # key range of the forced case: below 2 * 1500


@pytest.fixture(scope="module")
def forced_case():
    """~1500 distinct keys, a shuffled subset of [KMIN, KMIN + SPAN), 2 %
    nulls (their data word is 0, inside the range); both ends present."""
    rnd = random.Random(17)
    inner = rnd.sample(range(KMIN + 1, KMIN + SPAN - 1), 1498)
    bvals = [KMIN, KMIN + SPAN - 1] + inner
    rnd.shuffle(bvals)
    bvals = [None if (rnd.random() < 0.02 and v not in (KMIN, KMIN + SPAN - 1))
             else v for v in bvals]
    pvals = [rnd.randint(KMIN - 50, KMIN + SPAN + 50)
             if rnd.random() > 0.03 else None for _ in range(3000)]
    pvals[:10] = [KMIN, KMIN + SPAN - 1, KMIN - 1, KMIN + SPAN,
                  KMIN + 2**32, KMIN - 2**32 + 17, INT64_MIN, INT64_MAX,
                  KMIN + 17, None]
    b, p = _i64(bvals), _i64(pvals)
    return b, p, _generic_pairs(b, p)


@pytest.mark.parametrize("hint", [None, "exact", "small"])
def test_forced_dense_int64(forced_case, hint):
    from spark_rapids_jni_amd.ops.join import HashJoinTable
    b, p, ref = forced_case
    assert b.size == 1500 and b.validity is not None
    tbl = HashJoinTable.build(b, dense=True)
    assert tbl.layout == "dense" and tbl.i64_fast
    assert tbl.kmin == KMIN and tbl.capacity == SPAN <= 2 * b.size
    assert tbl.slots.numel() == SPAN and tbl.slots.element_size() == 4
    out_hint = {None: None, "exact": len(ref), "small": 10}[hint]
    bi, pi = tbl.inner_join(p, out_hint=out_hint)
    got = _sorted_pairs(bi, pi)
    assert got == ref and len(ref) > 1000
    # rows 0 and 1 (both ends of the range) match, rows 2..7 cannot
    assert [j for j, _ in got if j < 8] == [0, 1]


@pytest.mark.parametrize("kmin", [INT64_MIN + 3, INT64_MAX - 149])
def test_extreme_kmin(kmin):
    """Offsets are unsigned differences: they must not overflow or alias at
    either end of the int64 domain."""
    from spark_rapids_jni_amd.ops.join import HashJoinTable
    rnd = random.Random(23)
    span = 150
    bvals = [kmin, kmin + span - 1] + rnd.sample(
        range(kmin + 1, kmin + span - 1), 98)
    rnd.shuffle(bvals)
    pvals = list(bvals) + [INT64_MIN, INT64_MAX, INT64_MIN + 1,
                           INT64_MAX - 1, 0, -1, 1]
    for d in (1, 2, span, 2**32, 2**62):
        for v in (kmin - d, kmin + span - 1 + d):
            if INT64_MIN <= v <= INT64_MAX:
                pvals.append(v)
            else:               # what the subtraction would wrap to
                pvals.append((v - INT64_MIN) % 2**64 + INT64_MIN)
    b, p = _i64(bvals), _i64(pvals)
    tbl = HashJoinTable.build(b, dense=True)
    assert tbl.layout == "dense" and tbl.kmin == kmin
    assert tbl.capacity == span
    bi, pi = tbl.inner_join(p)
    got = _sorted_pairs(bi, pi)
    assert got == _generic_pairs(b, p) and len(got) >= 100


PROBE_SIZES = [0, 1, 7, 8, 9, 15, 16, 17, 511, 512, 513, 64 * 16 + 1]


@pytest.mark.parametrize("nbuild", [0, 1, 9])
def test_tails(nbuild):
    from spark_rapids_jni_amd.ops.join import HashJoinTable
    rnd = random.Random(nbuild)
    bvals = [40 + (5 * i) % 9 for i in range(nbuild)]   # distinct, range <= 9
    b = _i64(bvals)
    tbl = HashJoinTable.build(b, dense=True)
    assert tbl.layout == "dense"
    assert tbl.capacity == (max(bvals) - min(bvals) + 1 if nbuild else 1)
    ref_tbl = _generic(b)
    for nprobe in PROBE_SIZES:
        for with_valid in (False, True):
            pvals = [rnd.randint(36, 52) for _ in range(nprobe)]
            if nprobe:
                pvals[-1] = 40       # the last row of the tail batch matches
            if with_valid:
                pvals = [None if i % 5 == 3 else v
                         for i, v in enumerate(pvals)]
            p = _i64(pvals)
            assert (p.validity is not None) == (with_valid and nprobe > 3)
            bi, pi = tbl.inner_join(p)
            ref = _sorted_pairs(*ref_tbl.inner_join(p))
            assert _sorted_pairs(bi, pi) == ref, (nbuild, nprobe, with_valid)
            if nbuild and nprobe and pvals[-1] is not None:
                assert ref[-1][0] == nprobe - 1


def test_tails_past_the_batch_threshold():
    """A table of more than 2^26 slots takes the probe kernels' 8-row batch
    (16 below): the smallest build that gets there, every even key of a
    range of 2^26 + 1."""
    from spark_rapids_jni_amd.ops.join import HashJoinTable
    n = 2**25 + 1
    bk = torch.arange(n, dtype=torch.int32, device="cuda") * 2 - 1000
    b = Column.from_torch(bk)
    tbl = HashJoinTable.build(b, dense=True)
    assert tbl.layout == "dense" and tbl.kmin == -1000
    assert tbl.capacity == 2**26 + 1
    ref_tbl = _generic(b)
    rnd = random.Random(8)
    hi = 2 * (n - 1) - 1000                 # the largest build key
    for nprobe in PROBE_SIZES + [20001]:
        for with_valid in (False, True):
            pvals = [rnd.choice([-1000, -999, -1001, hi, hi + 1, hi - 1,
                                 rnd.randint(-2000, hi + 1000)])
                     for _ in range(nprobe)]
            if nprobe:
                pvals[-1] = hi
            if with_valid:
                pvals = [None if i % 5 == 3 else v
                         for i, v in enumerate(pvals)]
            p = Column.from_pylist(pvals, DType.INT32, "cuda")
            ref = _sorted_pairs(*ref_tbl.inner_join(p))
            for hint in ((None, 10) if nprobe == 20001 else (None,)):
                bi, pi = tbl.inner_join(p, out_hint=hint)
                assert _sorted_pairs(bi, pi) == ref, (nprobe, with_valid)
            if nprobe and pvals[-1] is not None:
                assert ref[-1] == (nprobe - 1, n - 1)


@pytest.mark.parametrize("tdt", [torch.int32, torch.int16])
def test_int32_and_int16_key_columns(monkeypatch, tdt):
    from spark_rapids_jni_amd import _native
    from spark_rapids_jni_amd.ops.join import HashJoinTable
    n = 3000
    gen = torch.Generator(device="cuda").manual_seed(5)
    bk = (torch.randperm(2 * n, device="cuda", generator=gen)[:n] - 1234
          ).to(tdt)
    pk = torch.cat([bk[:n // 2],
                    torch.randint(-3000, 6000, (n + 7,), device="cuda",
                                  generator=gen).to(tdt)])
    b, p = Column.from_torch(bk), Column.from_torch(pk)
    ref = _generic_pairs(b, p)
    spy = _Spy(_native.gpu())
    monkeypatch.setattr(_native, "gpu", lambda: spy)
    tbl = HashJoinTable.build(b, dense=True)
    bi, pi = tbl.inner_join(p)
    monkeypatch.undo()
    assert tbl.layout == "dense" and tbl.kmin == int(bk.min().item())
    assert tbl.capacity <= 2 * n
    assert _sorted_pairs(bi, pi) == ref and len(ref) >= n // 2
    names = [c[0] for c in spy.calls]
    assert names == ["join_build_d32", "join_probe_d32", "join_probe_d32"]
    assert all(args[1] == 1 for _, args in spy.calls)   # key_i32
    if tdt == torch.int32:
        # the kernels got the int32 columns themselves, not a copy
        assert spy.calls[0][1][0] == b.data.data_ptr()
        for _, args in spy.calls[1:]:
            assert args[0] == p.data.data_ptr()
    # an int64 probe column of the same values against the same table (the
    # generic table compares key bytes, so its probe keeps the build's dtype)
    p64 = Column.from_torch(pk.to(torch.int64))
    bi, pi = tbl.inner_join(p64)
    assert _sorted_pairs(bi, pi) == ref
    # and the other way round: int64 build, narrower probe
    b64 = Column.from_torch(bk.to(torch.int64))
    t64 = HashJoinTable.build(b64, dense=True)
    assert t64.layout == "dense"
    bi, pi = t64.inner_join(p)
    assert _sorted_pairs(bi, pi) == ref


def test_build_matches_agree_with_wide(forced_case):
    from spark_rapids_jni_amd.ops.join import HashJoinTable
    b, p, ref = forced_case
    dt = HashJoinTable.build(b, dense=True)
    wt = HashJoinTable.build(b, narrow=False)
    assert dt.layout == "dense" and wt.layout == "wide"
    db, dpi, dm = dt.inner_join(p, track_build_matches=True)
    wb, wpi, wm = wt.inner_join(p, track_build_matches=True)
    assert _sorted_pairs(db, dpi) == ref == _sorted_pairs(wb, wpi)
    assert torch.equal(dm, wm)
    assert 0 < int(dm.sum().item()) < b.size
    # capacity-0 mark-only probe
    assert torch.equal(dt.mark_matches(p), wm)


@pytest.mark.parametrize("anti", [False, True])
def test_semi_and_anti_on_dense_table(forced_case, anti):
    """n = 1500 and capacity = 2800 are no powers of two: the generic table
    behind semi_join is sized from the row count."""
    from spark_rapids_jni_amd.ops.join import HashJoinTable
    b, p, _ = forced_case
    tbl = HashJoinTable.build(b, dense=True)
    assert tbl.layout == "dense" and tbl.capacity & (tbl.capacity - 1)
    got = tbl.semi_join(p, anti=anti)
    ref = _generic(b).semi_join(p, anti=anti)
    assert sorted(got.cpu().tolist()) == sorted(ref.cpu().tolist())
    assert 0 < got.numel() < p.size
    assert tbl._generic.capacity == 4096


def test_duplicates_and_sparse_ranges_raise():
    from spark_rapids_jni_amd.ops.join import HashJoinTable
    keys = torch.randperm(2000, dtype=torch.int64, device="cuda")
    assert HashJoinTable.build(Column.from_torch(keys.clone()),
                               dense=True).layout == "dense"
    keys[77] = keys[1400]
    with pytest.raises(ValueError):
        HashJoinTable.build(Column.from_torch(keys), dense=True)
    # range 2n + 1 with n = 40: past the 64-slot floor
    n = 40
    sparse = torch.arange(n, dtype=torch.int64, device="cuda")
    sparse[-1] = 2 * n - 1
    assert HashJoinTable.build(Column.from_torch(sparse.clone()),
                               dense=True).capacity == 2 * n
    sparse[-1] = 2 * n
    with pytest.raises(ValueError):
        HashJoinTable.build(Column.from_torch(sparse), dense=True)
    # other layouts cannot be forced together with dense
    with pytest.raises(ValueError):
        HashJoinTable.build(Column.from_torch(keys), dense=True, narrow=True)


def test_auto_rule_at_scan_threshold():
    from spark_rapids_jni_amd.ops import join as J
    n = J.NARROW_SCAN_MIN_ROWS
    gen = torch.Generator(device="cuda").manual_seed(3)
    perm = torch.randperm(n, dtype=torch.int64, device="cuda", generator=gen)
    keys = perm + 100
    top = int((perm == n - 1).nonzero().item())     # row of the largest key
    mid = int((perm == n // 2).nonzero().item())
    low = int((perm == 5).nonzero().item())

    def col(k):
        return Column(DType.INT64, n, k)

    def check(tbl, k, pvals):
        p = _i64(pvals)
        bi, pi = tbl.inner_join(p)
        got = _sorted_pairs(bi, pi)
        assert got == _generic_pairs(col(k), p)
        return got

    base_probe = [100, 99, 105, 100 + n // 2, 100 + n - 1, 100 + n,
                  100 + 2 * n - 1, 100 + 2 * n, 100 + 2**32]
    tbl = J.HashJoinTable.build(col(keys))
    assert tbl.layout == "dense" and tbl.kmin == 100 and tbl.capacity == n
    got = check(tbl, keys, base_probe)
    assert [j for j, _ in got] == [0, 2, 3, 4]
    assert (2, low) in got and (4, top) in got

    k2 = keys.clone()
    k2[top] = 100 + 2 * n - 1                       # range exactly 2n
    tbl = J.HashJoinTable.build(col(k2))
    assert tbl.layout == "dense" and tbl.capacity == 2 * n
    assert [j for j, _ in check(tbl, k2, base_probe)] == [0, 2, 3, 6]

    k3 = keys.clone()
    k3[top] = 100 + 2 * n                           # range 2n + 1
    tbl = J.HashJoinTable.build(col(k3))
    assert tbl.layout == "narrow" and tbl.kmin == 100
    assert [j for j, _ in check(tbl, k3, base_probe)] == [0, 2, 3, 7]

    k4 = keys.clone()
    k4[mid] = 105                                   # one key duplicated
    tbl = J.HashJoinTable.build(col(k4))
    assert tbl.layout == "narrow" and tbl.kmin == 100
    got = check(tbl, k4, base_probe)
    assert sorted(b for j, b in got if j == 2) == sorted([low, mid])
    assert [j for j, _ in got] == [0, 2, 2, 4]

    assert J.HashJoinTable.build(col(keys), dense=False).layout == "narrow"
    assert J.HashJoinTable.build(col(keys), narrow=False).layout == "wide"
    assert J.HashJoinTable.build(col(keys), narrow=True).layout == "narrow"
