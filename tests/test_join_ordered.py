"""Ordered build keys (row i holds key kmin + i): the key scan kernel, the
routing to the table-free "ordered" layout and every probe method on it.
The oracle is a dict join on the CPU; pairs are compared as sorted lists."""
import random

import pytest
import torch

from spark_rapids_jni_amd.columnar import Column, DType

pytestmark = pytest.mark.gpu

INT64_MIN, INT64_MAX = -2**63, 2**63 - 1
M64 = 2**64


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


def _wrap(v):
    """v as the int64 that two's complement arithmetic gives."""
    return (v - INT64_MIN) % M64 + INT64_MIN


def _col(vals, dtype=DType.INT64):
    tdt = torch.int64 if dtype == DType.INT64 else torch.int32
    if not vals:
        return Column.from_torch(torch.empty(0, dtype=tdt, device="cuda"))
    return Column.from_pylist(vals, dtype, "cuda")


# ---------------------------------------------------------------------------
# the scan kernel
# ---------------------------------------------------------------------------
# a workgroup of 256 threads takes vectors 256 w .. 256 w + 255 first: with
# two int64 keys per 16-byte load its first row is 512 w
WG_ROWS = 512
# 4 loads of 2 keys per thread and iteration: 6 workgroups and a ragged tail
N_MANY = 5 * 2048 + 37
SCAN_SIZES = [1, 2, 63, 64, 65, 2047, 2048, 2049, N_MANY]


def _definition(keys, valid):
    """(min, max, flag) by the definition: flag is what the kernel reports,
    every row valid and key[i] - key[0] == i in unsigned arithmetic."""
    flag = all(valid) and all((k - keys[0]) % M64 == i
                              for i, k in enumerate(keys))
    return min(keys), max(keys), flag


def _mask(valid):
    n = len(valid)
    m = torch.zeros((n + 63) // 64 * 8, dtype=torch.uint8)
    for i, v in enumerate(valid):
        if v:
            m[i >> 3] |= 1 << (i & 7)
    # bits of rows at or past n in the last byte: set, and must be ignored
    if n & 7:
        m[n >> 3] |= (0xff << (n & 7)) & 0xff
    return m.cuda()


def _check_scan(keys, tdt=torch.int64, valid=None, offset=0):
    """Runs the kernel on `keys` and compares with torch.aminmax and the
    definition. offset > 0 places the keys that many elements into a buffer,
    which takes the kernel off its 16-byte load path."""
    from spark_rapids_jni_amd import _native
    from spark_rapids_jni_amd.ops import join as J
    n = len(keys)
    buf = torch.zeros(n + offset, dtype=tdt, device="cuda")
    data = buf[offset:]
    data.copy_(torch.tensor(keys, dtype=tdt))
    key_i32 = 1 if tdt == torch.int32 else 0
    vmask = _mask(valid) if valid is not None else None
    out = torch.empty(3, dtype=torch.int64, device="cuda")
    _native.gpu().join_scan_keys(
        data.data_ptr(), key_i32, vmask.data_ptr() if vmask is not None else 0,
        n, out.data_ptr(), _native.current_stream())
    lo, hi, flag = out.cpu().tolist()
    tlo, thi = torch.aminmax(data)
    assert (lo, hi) == (int(tlo), int(thi))
    dlo, dhi, dflag = _definition(keys, valid or [True] * n)
    assert (lo, hi, bool(flag)) == (dlo, dhi, dflag)
    # what the host accepts: the flag and a range of exactly n keys
    got = J._scan_keys(data, key_i32, vmask, n)
    assert got == (dlo, dhi, dflag and dhi - dlo == n - 1)
    return got[2]


@pytest.mark.parametrize("n", SCAN_SIZES)
def test_scan_ordered_keys(n):
    for kmin in (0, 100, INT64_MIN + 3, INT64_MAX - n + 1):
        assert _check_scan([kmin + i for i in range(n)])
    # 8-byte aligned only: the one-key-per-load path
    assert _check_scan([100 + i for i in range(n)], offset=1)
    assert _check_scan([-5 + i for i in range(n)], torch.int32)
    assert _check_scan([-5 + i for i in range(n)], torch.int32, offset=1)
    assert _check_scan([7 + i for i in range(n)], valid=[True] * n)


@pytest.mark.parametrize("n", [2, 65, 2049, N_MANY])
def test_scan_wraps_past_int64_max(n):
    """key[i] - key[0] == i holds in unsigned arithmetic; the range does not."""
    for first in (INT64_MAX, INT64_MAX - n + 2, INT64_MAX - (n - 1) // 2):
        keys = [_wrap(first + i) for i in range(n)]
        assert min(keys) == INT64_MIN and max(keys) == INT64_MAX
        assert not _check_scan(keys)


@pytest.mark.parametrize("n", [2, 64, 65, 2049, N_MANY])
def test_scan_not_ordered(n):
    base = [100 + i for i in range(n)]
    rows = {0, n - 1, n // 2}
    rows |= {r for r in (WG_ROWS - 1, WG_ROWS, 2 * WG_ROWS) if r < n}
    for r in sorted(rows):
        for delta in (1, -1, 2**32, -2**40):
            keys = list(base)
            keys[r] += delta
            assert not _check_scan(keys)
        if r + 1 < n:                        # an adjacent pair swapped
            keys = list(base)
            keys[r], keys[r + 1] = keys[r + 1], keys[r]
            assert not _check_scan(keys)
        if r:                                # one duplicate
            keys = list(base)
            keys[r] = keys[r - 1]
            assert not _check_scan(keys)
    assert not _check_scan([100 + 2 * i for i in range(n)])
    assert not _check_scan([100 - i for i in range(n)])
    assert not _check_scan([100 - i for i in range(n)], torch.int32)
    keys = list(base)
    keys[n // 2] += 3
    assert not _check_scan(keys, torch.int32)
    assert not _check_scan(keys, offset=1)


@pytest.mark.parametrize("n", [1, 2, 9, 64, 65, 2049, N_MANY])
def test_scan_nulls(n):
    keys = [100 + i for i in range(n)]
    assert _check_scan(keys, valid=[True] * n)
    for r in sorted({0, n // 2, n - 1, min(n - 1, WG_ROWS)}):
        valid = [True] * n
        valid[r] = False
        assert not _check_scan(keys, valid=valid)
        assert not _check_scan(keys, valid=valid, offset=1)
        assert not _check_scan(keys, torch.int32, valid=valid)


# ---------------------------------------------------------------------------
# routing
# ---------------------------------------------------------------------------
def test_routing_at_scan_threshold(monkeypatch):
    from spark_rapids_jni_amd import _native
    from spark_rapids_jni_amd.ops import join as J
    n = J.NARROW_SCAN_MIN_ROWS
    keys = torch.arange(n, dtype=torch.int64, device="cuda") + 100

    def col(k):
        return Column(DType.INT64, n, k)

    spy = _Spy(_native.gpu())
    monkeypatch.setattr(_native, "gpu", lambda: spy)
    tbl = J.HashJoinTable.build(col(keys))
    built = [c[0] for c in spy.calls]
    probe = _col([100, 99, 100 + n - 1, 100 + n, 100 + 2**32, 105])
    bi, pi = tbl.inner_join(probe)
    monkeypatch.undo()
    assert tbl.layout == "ordered" and tbl.i64_fast
    assert tbl.slots is None and tbl.capacity == n and tbl.kmin == 100
    assert built == ["join_scan_keys"]
    assert [c[0] for c in spy.calls[1:]] == ["join_probe_ord"] * 2
    assert sorted(zip(pi.tolist(), bi.tolist())) == [(0, 0), (2, n - 1),
                                                     (5, 5)]

    swapped = keys.clone()
    swapped[[7, n - 9]] = swapped[[n - 9, 7]]
    assert J.HashJoinTable.build(col(swapped)).layout == "dense"
    assert J.HashJoinTable.build(col(keys), ordered=False).layout == "dense"
    assert J.HashJoinTable.build(col(keys), dense=True).layout == "dense"
    # a null row: not ordered
    valid = torch.full(((n + 63) // 64 * 8,), 0xff, dtype=torch.uint8,
                       device="cuda")
    valid[3] = 0xfe
    nul = Column(DType.INT64, n, keys, valid, null_count=None)
    assert J.HashJoinTable.build(nul).layout == "dense"


def test_forced_ordered_raises():
    from spark_rapids_jni_amd.ops.join import HashJoinTable
    vals = list(range(5, 405))
    good = _col(vals)
    assert HashJoinTable.build(good, ordered=True).layout == "ordered"
    # below the scan threshold nothing is scanned unless forced
    assert HashJoinTable.build(good).layout == "wide"
    shuffled = list(vals)
    random.Random(3).shuffle(shuffled)
    with pytest.raises(ValueError):
        HashJoinTable.build(_col(shuffled), ordered=True)
    with pytest.raises(ValueError):
        HashJoinTable.build(_col(vals[:100] + [None] + vals[101:]),
                            ordered=True)
    for kw in ({"narrow": True}, {"narrow": False}, {"dense": True},
               {"force_generic": True}):
        with pytest.raises(ValueError):
            HashJoinTable.build(good, ordered=True, **kw)
    with pytest.raises(ValueError):
        HashJoinTable.build([good, good], ordered=True)


# ---------------------------------------------------------------------------
# the probe
# ---------------------------------------------------------------------------
KMIN = -7
NBUILD = 1500


def _tile():
    from spark_rapids_jni_amd import _native
    return _native.gpu().JOIN_PROBE_TILE["ordered"]


def _probe_vals(nprobe, kmin, n, nulls, i32=False, seed=0):
    rnd = random.Random(1000 * nprobe + seed)
    vals = [rnd.randint(kmin - 50, kmin + n + 50) for _ in range(nprobe)]
    special = [kmin - 1, kmin, kmin + n - 1, kmin + n]
    if not i32:
        special += [kmin + 2**32, kmin - 2**32, INT64_MIN, INT64_MAX,
                    kmin + 2**32 + 5, _wrap(kmin + 2**63 + 3)]
    else:
        special += [-2**31, 2**31 - 1]
    # at both ends of the probe column and of a tile where there is room
    for at in (0, nprobe - len(special)):
        if 0 <= at and at + len(special) <= nprobe:
            vals[at:at + len(special)] = special
    if nprobe and nprobe < len(special):
        vals = special[:nprobe]
    if nulls:
        vals = [None if rnd.random() < 0.05 else v for v in vals]
        if nprobe > 2:
            vals[1] = None
            vals[-1] = None
    return vals


def _oracle(bkeys, pvals):
    """Sorted inner (probe row, build row) pairs by a dict join."""
    rows = {k: i for i, k in enumerate(bkeys)}
    assert len(rows) == len(bkeys)
    return sorted((j, rows[v]) for j, v in enumerate(pvals)
                  if v is not None and v in rows)


def _pairs(bi, pi):
    return sorted(zip(pi.cpu().tolist(), bi.cpu().tolist()))


def _check_all_methods(tbl, bkeys, p, pvals):
    nb, nprobe = len(bkeys), len(pvals)
    ref = _oracle(bkeys, pvals)
    hit_p = {j for j, _ in ref}
    hit_b = {b for _, b in ref}
    matched_ref = [1 if b in hit_b else 0 for b in range(nb)]
    outer_ref = sorted(ref + [(j, -1) for j in range(nprobe)
                              if j not in hit_p])

    for hint in (None, len(ref), max(len(ref) // 3, 0)):
        bi, pi = tbl.inner_join(p, out_hint=hint)
        assert bi.dtype == torch.int32 and pi.dtype == torch.int64
        assert _pairs(bi, pi) == ref
    bi, pi, matched = tbl.inner_join(p, track_build_matches=True)
    assert _pairs(bi, pi) == ref and matched.tolist() == matched_ref

    for hint in (None, len(outer_ref), len(outer_ref) // 3):
        bi, pi = tbl.left_outer_join(p, out_hint=hint)
        assert _pairs(bi, pi) == outer_ref
    bi, pi, matched = tbl.left_outer_join(p, track_build_matches=True)
    assert _pairs(bi, pi) == outer_ref and matched.tolist() == matched_ref

    fb, fp = tbl.full_outer_join(p)
    full_ref = sorted(outer_ref + [(-1, b) for b in range(nb)
                                   if b not in hit_b])
    assert _pairs(fb, fp) == full_ref

    for anti in (False, True):
        want = [int((j in hit_p) != anti) for j in range(nprobe)]
        assert tbl.probe_matches(p, anti).tolist() == want
        sel = tbl.semi_select(p, anti)
        assert sel.dtype == torch.int64
        assert sel.tolist() == [j for j in range(nprobe) if want[j]]
    assert tbl.mark_matches(p).tolist() == matched_ref
    return ref


def _probe_sizes():
    t = _tile()
    return [0, 1, 63, t - 1, t, t + 1, 3 * t + 65]


@pytest.fixture(scope="module")
def build_1500():
    from spark_rapids_jni_amd.ops.join import HashJoinTable
    bkeys = [KMIN + i for i in range(NBUILD)]
    tbl = HashJoinTable.build(_col(bkeys), ordered=True)
    assert tbl.layout == "ordered" and tbl.slots is None
    assert tbl.kmin == KMIN and tbl.capacity == NBUILD
    return tbl, bkeys


@pytest.mark.parametrize("nulls", [False, True])
@pytest.mark.parametrize("size", range(7))
def test_probe_every_method(build_1500, size, nulls):
    tbl, bkeys = build_1500
    nprobe = _probe_sizes()[size]
    pvals = _probe_vals(nprobe, KMIN, NBUILD, nulls)
    ref = _check_all_methods(tbl, bkeys, _col(pvals), pvals)
    if nprobe >= 63:
        assert len(ref) > nprobe // 2
    if nprobe >= 63 and not nulls:
        # KMIN - 1 misses, both ends of the range hit, KMIN + n misses
        assert [j for j, _ in ref if j < 4] == [1, 2]


@pytest.mark.parametrize("nb", [0, 1])
def test_probe_tiny_builds(nb):
    from spark_rapids_jni_amd.ops.join import HashJoinTable
    kmin = 40
    bkeys = [kmin + i for i in range(nb)]
    tbl = HashJoinTable.build(_col(bkeys), ordered=True)
    assert tbl.layout == "ordered" and tbl.capacity == nb
    t = _tile()
    for nprobe in (0, 1, 63, t + 1):
        for nulls in (False, True):
            pvals = _probe_vals(nprobe, kmin, nb, nulls)
            if nprobe > 20:
                pvals[13] = kmin
                pvals[14] = 0          # kmin of the empty table
            ref = _check_all_methods(tbl, bkeys, _col(pvals), pvals)
            assert nb or not ref


@pytest.mark.parametrize("extreme", [INT64_MIN + 3, INT64_MAX - 149])
def test_probe_extreme_kmin(extreme):
    from spark_rapids_jni_amd.ops.join import HashJoinTable
    nb = 150
    bkeys = [extreme + i for i in range(nb)]
    tbl = HashJoinTable.build(_col(bkeys), ordered=True)
    assert tbl.kmin == extreme
    pvals = list(bkeys[::3]) + [INT64_MIN, INT64_MAX, INT64_MIN + 1,
                                INT64_MAX - 1, 0, -1, 1, None]
    for d in (1, 2, nb, 2**32, 2**62, 2**63):
        for v in (extreme - d, extreme + nb - 1 + d):
            pvals.append(_wrap(v))
    _check_all_methods(tbl, bkeys, _col(pvals), pvals)


@pytest.mark.parametrize("nulls", [False, True])
def test_probe_mixed_key_widths(build_1500, nulls):
    from spark_rapids_jni_amd.ops.join import HashJoinTable
    tbl, bkeys = build_1500
    nprobe = _tile() + 65
    pvals = _probe_vals(nprobe, KMIN, NBUILD, nulls, i32=True)
    # int32 probe keys against the int64 build
    _check_all_methods(tbl, bkeys, _col(pvals, DType.INT32), pvals)
    # int64 probe keys against an int32 build
    t32 = HashJoinTable.build(_col(bkeys, DType.INT32), ordered=True)
    assert t32.layout == "ordered" and t32.kmin == KMIN
    pvals = _probe_vals(nprobe, KMIN, NBUILD, nulls)
    _check_all_methods(t32, bkeys, _col(pvals), pvals)
