"""The NDS group-by route (nds/plan.py GpuBackend(groupby_mode=...),
Engine(deterministic=...)): the sort-based group-by of ops/segmented.py
against the CPU oracle backend, run-to-run equality without rounding, and
the per-path call counters.

Engine(deterministic=True) also puts the output of every join in a fixed row
order (GpuBackend(ordered_joins=True)): the probe kernels place matches at an
atomic cursor, and without that the rows of a group would reach the sums in
another order on every run.

CPU tier: the sorted route runs on CPU tensors through the op's torch twin
(aggregations only - joins of the GPU backend need the device), so the
plumbing of _agg_frame is checked without a GPU. GPU tier: queries at the
scale factor of tests/test_nds.py. Between them q3 (multi-key), q5 and q77
(rollup over unions, nullable keys), q7 (avg), q28 (global aggregates with
count distinct), q42, q67 (nine-level rollup), q70 (rollup and window) and
q97 (global sums) cover a global aggregate, a rollup, avg, count distinct and
multi-key aggregates with nullable keys; stddev_samp has no query in that
list and is covered by the synthetic frame below on both tiers.
"""
import functools

import pytest
import torch

from spark_rapids_jni_amd.nds import gen_catalog
from spark_rapids_jni_amd.nds import plan as P
from spark_rapids_jni_amd.nds.expr import Val, col
from spark_rapids_jni_amd.nds.plan import (Agg, CpuBackend, Distinct, Engine,
                                           Frame, GpuBackend, Scan)
from spark_rapids_jni_amd.nds.queries import QUERIES
from spark_rapids_jni_amd.nds.runner import compare_frames

SF = 0.01
NDS_QUERIES = [3, 5, 7, 28, 42, 67, 70, 77, 97]


@functools.lru_cache(maxsize=None)
def catalog():
    return gen_catalog(sf=SF)


@functools.lru_cache(maxsize=None)
def oracle(q):
    return QUERIES[q](Engine(catalog(), device="cpu", backend=CpuBackend()))


def _frame(dev, n, seed=7):
    g = torch.Generator().manual_seed(seed)
    k1 = torch.randint(0, 6, (n,), generator=g)
    v1 = torch.rand(n, generator=g) < 0.85
    k2 = torch.randint(0, 4, (n,), generator=g)
    k3 = torch.randint(-2, 3, (n,), generator=g).to(torch.int32)
    v3 = torch.rand(n, generator=g) < 0.9
    # quarter-integers: every sum below is exact in any order
    x = torch.randint(-40, 40, (n,), generator=g).to(torch.float64) / 4
    vx = torch.rand(n, generator=g) < 0.8
    qty = torch.randint(-3, 30, (n,), generator=g).to(torch.int32)
    return Frame({
        "k1": Val(k1.to(dev), v1.to(dev)),
        "code": Val(k2.to(dev), None, ["d%d" % i for i in range(4)]),
        "k3": Val(k3.to(dev), v3.to(dev)),
        "x": Val(x.to(dev), vx.to(dev)),
        "qty": Val(qty.to(dev)),
    }, n)


_AGGS = [("n", "count", None), ("nx", "count", col("x")),
         ("sx", "sum", col("x")), ("mn", "min", col("x")),
         ("mx", "max", col("qty")), ("av", "avg", col("x")),
         ("sd", "stddev_samp", col("x")), ("sq", "sum", col("qty"))]


def _plans(with_keyed_countd):
    plans = [
        Agg(Scan("t"), ["k1", "code", "k3"], _AGGS),          # nullable keys
        Agg(Scan("t"), [], _AGGS + [("cd", "countd", col("qty"))]),  # global
        Agg(Scan("t"), ["code", "k1"],
            [("sx", "sum", col("x")), ("n", "count", None),
             ("mx", "max", col("qty"))], rollup=True),
        Distinct(Scan("t", ["k1", "k3"])),
        Agg(Scan("empty"), [], [("n", "count", None),
                                ("sx", "sum", col("x"))]),
    ]
    if with_keyed_countd:  # merges by a join: the GPU backend's needs a GPU
        plans.append(Agg(Scan("t"), ["k1"], [("cd", "countd", col("qty")),
                                             ("sx", "sum", col("x"))]))
    return plans


def _run_synthetic(dev, n, backend, with_keyed_countd):
    e = Engine({}, device=dev, backend=backend)
    e.register("t", _frame(dev, n))
    e.register("empty", _frame(dev, 0))
    return e, [e.run(p) for p in _plans(with_keyed_countd)]


def _check_synthetic(dev, n):
    on_gpu = dev == "cuda"
    _e, want = _run_synthetic("cpu", n, CpuBackend(), on_gpu)
    e, got = _run_synthetic(dev, n, GpuBackend("sorted", dev,
                                               ordered_joins=on_gpu), on_gpu)
    for k, (g, w) in enumerate(zip(got, want)):
        compare_frames(g, w, k)
    st = e.groupby_stats
    assert st is e.backend.groupby_stats
    assert st.hash_calls == 0 and st.sorted_calls > 0
    # the global aggregate, its count distinct aside, is ONE call with no
    # key, however many aggregates it has; so are the one over no rows and
    # the top level of the rollup
    assert st.global_calls == 3
    return got


# ---------------------------------------------------------------------------
# CPU tier
# ---------------------------------------------------------------------------

def test_modes_and_engine_flag():
    assert P.GROUPBY_MODES == ("auto", "hash", "sorted")
    with pytest.raises(ValueError, match="groupby_mode"):
        GpuBackend("sort")
    assert GpuBackend().groupby_mode == "auto"
    # building an engine touches no device
    assert Engine({}, device="cuda").backend.groupby_mode == "auto"
    e = Engine({}, device="cuda", deterministic=True)
    assert e.backend.groupby_mode == "sorted" and e.backend.ordered_joins
    assert not GpuBackend("sorted").ordered_joins
    assert e.groupby_stats is e.backend.groupby_stats
    c = Engine({}, device="cpu", deterministic=True)
    assert isinstance(c.backend, CpuBackend)
    assert (c.groupby_stats.hash_calls, c.groupby_stats.sorted_calls) == (0, 0)


def test_auto_mode_obeys_the_constant(monkeypatch):
    b = GpuBackend("auto")
    lim = P.SORTED_GROUPBY_MAX_ROWS
    assert isinstance(lim, int) and lim >= 0
    assert not b.uses_sorted(0)
    assert b.uses_sorted(1) == (lim >= 1)
    assert b.uses_sorted(max(lim, 1)) == (lim >= 1)
    assert not b.uses_sorted(lim + 1)
    monkeypatch.setattr(P, "SORTED_GROUPBY_MAX_ROWS", 100)
    assert b.uses_sorted(100) and not b.uses_sorted(101)
    assert GpuBackend("sorted").uses_sorted(10 ** 9)
    assert not GpuBackend("hash").uses_sorted(1)


@pytest.mark.parametrize("n", [1, 300, 5000])
def test_cpu_sorted_route_matches_oracle_backend(n):
    _check_synthetic("cpu", n)


def test_cpu_sorted_route_groups_come_out_in_key_order():
    e = Engine({}, device="cpu", backend=GpuBackend("sorted", "cpu"))
    e.register("t", _frame("cpu", 300))
    rows = e.run(Agg(Scan("t"), ["k1", "k3"], [("n", "count", None)])) \
        .to_rows()
    keys = [tuple((0, 0) if x is None else (1, x) for x in r[:2])
            for r in rows]
    assert keys == sorted(keys) and len(set(keys)) == len(keys)


# ---------------------------------------------------------------------------
# GPU tier
# ---------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("n", [300, 5000])
def test_gpu_sorted_route_matches_oracle_backend(n):
    a = _check_synthetic("cuda", n)
    b = _check_synthetic("cuda", n)
    for fa, fb in zip(a, b):
        assert [repr(r) for r in fa.to_rows()] == \
            [repr(r) for r in fb.to_rows()]


@pytest.mark.gpu
@pytest.mark.parametrize("q", NDS_QUERIES)
def test_gpu_deterministic_engine_matches_cpu_oracle(q):
    e = Engine(catalog(), device="cuda", deterministic=True)
    got = QUERIES[q](e)
    compare_frames(got, oracle(q), q)
    st = e.groupby_stats
    assert st.sorted_calls > 0 and st.hash_calls == 0
    if q in (28, 97):  # global aggregates: no key, no sort
        assert st.global_calls > 0
    # a second fresh engine: the same rows, floats unrounded
    again = QUERIES[q](Engine(catalog(), device="cuda", deterministic=True))
    assert [repr(r) for r in again.to_rows()] == \
        [repr(r) for r in got.to_rows()]


@pytest.mark.gpu
def test_gpu_path_counters_follow_the_mode(monkeypatch):
    cat = catalog()
    h = Engine(cat, device="cuda", backend=GpuBackend("hash"))
    for q in (3, 28):
        compare_frames(QUERIES[q](h), oracle(q), q)
    assert h.groupby_stats.sorted_calls == 0
    assert h.groupby_stats.global_calls == 0
    assert h.groupby_stats.hash_calls > 0

    def auto_counts(limit):
        monkeypatch.setattr(P, "SORTED_GROUPBY_MAX_ROWS", limit)
        e = Engine({}, device="cuda")
        assert e.backend.groupby_mode == "auto"
        e.register("t", _frame("cuda", 300))
        e.register("big", _frame("cuda", 3000))
        for t in ("t", "big"):
            e.run(Agg(Scan(t), ["k1"], [("sx", "sum", col("x"))]))
            e.run(Agg(Scan(t), [], [("sx", "sum", col("x"))]))
        st = e.groupby_stats
        return st.sorted_calls, st.global_calls, st.hash_calls

    assert auto_counts(0) == (0, 0, 4)
    assert auto_counts(300) == (2, 1, 2)
    assert auto_counts(1 << 40) == (4, 2, 0)
