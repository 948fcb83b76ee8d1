"""Workgroup-level append of the fast-path probe kernels (the
range-partitioned dense probe measured with it was not merged, see
docs/PERF.md). The oracle is a dict join on the CPU; pairs are compared as
sorted (probe_idx, build_idx) lists."""
import random

import pytest
import torch

from spark_rapids_jni_amd.columnar import Column

pytestmark = pytest.mark.gpu

LAYOUTS = {"wide": dict(narrow=False), "narrow": dict(narrow=True),
           "dense": dict(dense=True)}


class _Spy:
    """Forwards to the native module and records (name, args) of each call;
    constants pass through."""

    def __init__(self, mod):
        self._mod = mod
        self.calls = []

    def __getattr__(self, name):
        fn = getattr(self._mod, name)
        if not callable(fn):
            return fn

        def wrapped(*args):
            self.calls.append((name, args))
            return fn(*args)
        return wrapped


def _gpu():
    from spark_rapids_jni_amd import _native
    return _native.gpu()


def _col(vals, valid=None, dtype=torch.int64):
    return Column.from_torch(torch.tensor(vals, dtype=dtype, device="cuda"),
                             valid)


def _oracle(bvals, bvalid, pvals, pvalid):
    rows = {}
    for i, k in enumerate(bvals):
        if bvalid is None or bvalid[i]:
            rows.setdefault(k, []).append(i)
    return sorted((j, i) for j, k in enumerate(pvals)
                  if pvalid is None or pvalid[j] for i in rows.get(k, ()))


def _pairs(bi, pi):
    return sorted(zip(pi.cpu().tolist(), bi.cpu().tolist()))


def _flags(ref, nbuild):
    f = [0] * nbuild
    for _, i in ref:
        f[i] = 1
    return f


def _nulls(rnd, n, share=0.1):
    return [rnd.random() >= share for _ in range(n)]


# ---------------------------------------------------------------------------
# workgroup append
# ---------------------------------------------------------------------------
def _build_rows(rnd, dup):
    """About 1,000 build rows, 10 % null: unique keys of [5, 1805), or about
    four rows per key of [0, 250)."""
    if dup:
        bvals = [rnd.randrange(0, 250) for _ in range(1000)]
    else:
        bvals = rnd.sample(range(5, 1805), 1000)
    return bvals, _nulls(rnd, 1000)


@pytest.mark.parametrize("layout,dup", [("wide", False), ("wide", True),
                                        ("narrow", False), ("narrow", True),
                                        ("dense", False)])
def test_workgroup_append(layout, dup):
    """Probe sizes at the edges of one workgroup tile (workgroup size times
    rows per lane) and past three tiles; probe keys reach past both ends of
    the build range; with duplicate build keys a row's several matches cross
    the workgroup scan."""
    from spark_rapids_jni_amd.ops.join import HashJoinTable
    rnd = random.Random(101 + 2 * len(layout) + dup)
    tile = _gpu().JOIN_PROBE_TILE[layout]
    assert tile % 512 == 0
    bvals, bvalid = _build_rows(rnd, dup)
    tbl = HashJoinTable.build(_col(bvals, bvalid), **LAYOUTS[layout])
    assert tbl.layout == layout
    lo, hi = (-60, 310) if dup else (-200, 2100)
    multi = False
    for n in (1, 63, tile - 1, tile, tile + 1, 3 * tile + 65):
        pvals = [rnd.randrange(lo, hi) for _ in range(n)]
        pvalid = _nulls(rnd, n)
        if n == 1:
            pvals, pvalid = [bvals[bvalid.index(True)]], [True]
        ref = _oracle(bvals, bvalid, pvals, pvalid)
        assert ref
        multi = multi or len(ref) > len({j for j, _ in ref})
        p = _col(pvals, pvalid)
        for hint in (None, len(ref), len(ref) // 3):
            assert _pairs(*tbl.inner_join(p, out_hint=hint)) == ref, (n, hint)
        bi, pi, matched = tbl.inner_join(p, track_build_matches=True)
        assert _pairs(bi, pi) == ref
        assert matched.cpu().tolist() == _flags(ref, len(bvals))
    assert multi == dup


# ---------------------------------------------------------------------------
# capacity guard at the native level
# ---------------------------------------------------------------------------
SENTINEL = -7


@pytest.fixture(scope="module")
def guard_case():
    """A dense table of 1,500 keys over a range of 2,800 and 20,000 probe
    rows, about half of which match."""
    from spark_rapids_jni_amd.ops.join import HashJoinTable
    rnd = random.Random(7)
    bvals = rnd.sample(range(-7, 2793), 1500)
    pvals = [rnd.randrange(-50, 2850) for _ in range(20000)]
    tbl = HashJoinTable.build(_col(bvals), dense=True)
    assert tbl.layout == "dense"
    ref = _oracle(bvals, None, pvals, None)
    assert 5000 < len(ref) < 15000
    return tbl, _col(pvals), ref


def _guarded_outputs(total):
    cap = total // 2
    ob = torch.full((total + 100,), SENTINEL, dtype=torch.int32, device="cuda")
    op = torch.full((total + 100,), SENTINEL, dtype=torch.int64, device="cuda")
    counter = torch.zeros(1, dtype=torch.int64, device="cuda")
    return cap, ob, op, counter


def _check_guard(cap, ob, op, counter, ref):
    assert int(counter.item()) == len(ref)
    assert bool((ob[cap:] == SENTINEL).all()) and bool((op[cap:] == SENTINEL).all())
    got = _pairs(ob[:cap], op[:cap])
    assert len(set(got)) == cap and set(got) <= set(ref)


def test_capacity_guard_direct(guard_case):
    from spark_rapids_jni_amd import _native
    tbl, p, ref = guard_case
    g = _gpu()
    cap, ob, op, counter = _guarded_outputs(len(ref))
    g.join_probe_d32(p.data.data_ptr(), 0, 0, p.size, tbl.slots.data_ptr(),
                     tbl.capacity, tbl.kmin, counter.data_ptr(),
                     ob.data_ptr(), op.data_ptr(), cap, 0, 1,
                     _native.current_stream())
    _check_guard(cap, ob, op, counter, ref)


# ---------------------------------------------------------------------------
# routing
# ---------------------------------------------------------------------------
def _spied_names(monkeypatch, tbl, p, **kw):
    from spark_rapids_jni_amd import _native
    spy = _Spy(_native.gpu())
    monkeypatch.setattr(_native, "gpu", lambda: spy)
    tbl.inner_join(p, **kw)
    monkeypatch.setattr(_native, "gpu", lambda: spy._mod)
    return [c[0] for c in spy.calls], spy.calls


def test_routing(monkeypatch, guard_case):
    """A dense probe is the one direct kernel call per pass that it was: count
    then fill without a hint, fill alone with one, fill with null outputs for
    a mark-only probe."""
    tbl, p, ref = guard_case
    names, calls = _spied_names(monkeypatch, tbl, p, out_hint=len(ref))
    assert names == ["join_probe_d32"]
    args = calls[0][1]
    assert args[:7] == (p.data.data_ptr(), 0, 0, p.size,
                        tbl.slots.data_ptr(), tbl.capacity, tbl.kmin)
    assert args[10] == len(ref) and args[12] == 1
    names, calls = _spied_names(monkeypatch, tbl, p)
    assert names == ["join_probe_d32", "join_probe_d32"]
    assert [c[1][12] for c in calls] == [0, 1]
    from spark_rapids_jni_amd import _native
    spy = _Spy(_native.gpu())
    monkeypatch.setattr(_native, "gpu", lambda: spy)
    tbl.mark_matches(p)
    monkeypatch.setattr(_native, "gpu", lambda: spy._mod)
    assert [c[0] for c in spy.calls] == ["join_probe_d32"]
    assert spy.calls[0][1][8:11] == (0, 0, 0)
