#!/usr/bin/env python3
"""Micro-benchmarks reproducing the reference's six nvbench shapes
(row transpose to/from rows, string->float, long->binary-string,
bloom build/probe, get_json_object 1-N paths, parse_uri) so per-op throughput
is comparable once numbers exist on both sides.

Run on an MI355X: python bench_micro.py [--rows N] [--iters K]
Prints one JSON line per shape: {"bench": ..., "value": ..., "unit": ...}.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch


def timeit(fn, iters, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


def emit(name, rows, secs, bytes_processed=None):
    rec = {"bench": name, "rows": rows, "ms": round(secs * 1e3, 3),
           "rows_per_sec": round(rows / secs, 1)}
    if bytes_processed:
        rec["GBps"] = round(bytes_processed / secs / 1e9, 2)
    print(json.dumps(rec), flush=True)


def ab_time(new_fn, old_fn, iters, repeats=5):
    """Time two equivalent paths in the same process, alternating them, so a
    drift of the machine's load hits both. Returns per-repeat seconds."""
    new_s, old_s = [], []
    for _ in range(repeats):
        new_s.append(timeit(new_fn, iters))
        old_s.append(timeit(old_fn, iters))
    return new_s, old_s


def emit_ab(name, rows, kept, new_s, old_s):
    def stats(xs):
        xs = sorted(xs)
        return {"ms": round(xs[len(xs) // 2] * 1e3, 4),
                "ms_min": round(xs[0] * 1e3, 4),
                "ms_max": round(xs[-1] * 1e3, 4)}
    for path, xs in (("hip", new_s), ("torch_parent", old_s)):
        rec = {"bench": name, "path": path, "rows": rows, "kept": kept,
               "repeats": len(xs)}
        rec.update(stats(xs))
        print(json.dumps(rec), flush=True)


def compact_bench(n, iters, dev, g):
    """Stream compaction and fused gather against the expressions they
    replaced (torch.nonzero + one t[idx] per tensor), at 1/50/99 % kept."""
    from spark_rapids_jni_amd.ops import compact
    ri = lambda dt: torch.randint(-2**31, 2**31, (n,), device=dev,
                                  generator=g).to(dt)
    frame = [ri(torch.int64), ri(torch.int64), ri(torch.int64),
             ri(torch.int32), ri(torch.int32),
             torch.rand(n, dtype=torch.float64, device=dev, generator=g),
             torch.rand(n, device=dev, generator=g) < 0.9,
             torch.rand(n, device=dev, generator=g) < 0.9]
    u = torch.rand(n, device=dev, generator=g)
    for kept in (0.01, 0.5, 0.99):
        m = u < kept

        def parent_nonzero():
            return torch.nonzero(m, as_tuple=False).view(-1)

        def parent_frame():
            idx = torch.nonzero(m, as_tuple=False).view(-1)
            return [t[idx] for t in frame]

        new_s, old_s = ab_time(lambda: compact.nonzero(m), parent_nonzero,
                               iters)
        emit_ab("compact_nonzero", n, kept, new_s, old_s)
        new_s, old_s = ab_time(lambda: compact.compact_tensors(frame, m),
                               parent_frame, iters)
        emit_ab("compact_frame_8col", n, kept, new_s, old_s)
    for kept in (0.01, 0.5, 0.99):
        idx = torch.nonzero(u < kept, as_tuple=False).view(-1)
        new_s, old_s = ab_time(lambda: compact.gather_tensors(frame, idx),
                               lambda: [t[idx] for t in frame], iters)
        emit_ab("gather_frame_8col", n, kept, new_s, old_s)


def parent_argsort(by, n, dev):
    """The expression NDS Sort/Window used before the native sort order:
    per key two gathers, a fill, a torch.argsort and a perm[o]. `by` is a
    list of (data, valid, ascending), first key primary."""
    perm = torch.arange(n, dtype=torch.int64, device=dev)
    for data, valid, asc in reversed(by):
        d = data[perm]
        if d.dtype == torch.bool:
            d = d.to(torch.int8)
        if valid is not None:
            vm = valid[perm]
            if d.dtype.is_floating_point:
                fill = float("-inf") if asc else float("inf")
            else:
                ii = torch.iinfo(d.dtype)
                fill = ii.min if asc else ii.max
            d = torch.where(vm, d, torch.full_like(d, fill))
        o = torch.argsort(d, stable=True, descending=not asc)
        perm = perm[o]
    return perm


def count_launches(fn):
    """GPU kernels launched by one call of fn (None without a profiler)."""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return sum(1 for e in prof.events()
                   if str(e.device_type).endswith("CUDA"))
    except Exception:  # the count is a report, not part of the timing
        return None


def sort_order_bench(n, iters, dev, g):
    """sort_order_tensors against the expression it replaced in NDS
    (parent_argsort) on four key sets. Median of `reps` timings."""
    from spark_rapids_jni_amd.ops.sort import sort_order_tensors
    ri = lambda lo, hi, dt: torch.randint(lo, hi, (n,), device=dev,
                                          generator=g).to(dt)
    valid = lambda: torch.rand(n, device=dev, generator=g) < 0.9
    # the extremes stay out: the old expression ties them with its null fill
    i32 = lambda: ri(-2**31 + 1, 2**31 - 1, torch.int32)
    code = lambda: ri(0, 1000, torch.int64)
    # (data, valid, ascending, key_bits)
    sets = {
        "int64_full": [(ri(-2**63, 2**63 - 1, torch.int64), None, True, None)],
        "int32": [(i32(), None, True, None)],
        "2x_int32_nullable": [(i32(), valid(), True, None),
                              (i32(), valid(), False, None)],
        "nds_6key": [(code(), None, True, 10), (code(), None, True, 10),
                     (code(), None, False, 10), (i32(), None, True, None),
                     (i32(), None, True, None),
                     (torch.rand(n, dtype=torch.float64, device=dev,
                                 generator=g), valid(), True, None)],
    }
    # what NDS Sort passes: the sort keys plus every other column of the
    # frame as a tie-breaker
    f64 = lambda: torch.rand(n, dtype=torch.float64, device=dev, generator=g)
    sets["nds_12key"] = sets["nds_6key"] + [
        (code(), None, True, 10), (code(), None, True, 10),
        (code(), valid(), True, 10), (f64(), None, True, None),
        (f64(), valid(), True, None), (i32(), valid(), True, None)]
    reps = 20
    inner = max(1, min(iters, 20)) if n <= 2**16 else 1
    for name, ks in sets.items():
        keys = [k[0] for k in ks]
        valids = [k[1] for k in ks]
        asc = [k[2] for k in ks]
        bits = [k[3] for k in ks]
        by = [(k[0], k[1], k[2]) for k in ks]
        # nulls first in either direction, as parent_argsort's fill does
        new = lambda: sort_order_tensors(keys, valids, asc, [True] * len(ks),
                                         bits)
        old = lambda: parent_argsort(by, n, dev)
        assert torch.equal(new(), old()), name
        new_s, old_s = ab_time(new, old, inner, repeats=reps)
        launches = {"hip": count_launches(new),
                    "torch_parent": count_launches(old)}

        def stats(xs):
            xs = sorted(xs)
            return {"ms": round(xs[len(xs) // 2] * 1e3, 4),
                    "ms_min": round(xs[0] * 1e3, 4),
                    "ms_max": round(xs[-1] * 1e3, 4)}
        for path, xs in (("hip", new_s), ("torch_parent", old_s)):
            rec = {"bench": "sort_order_" + name, "path": path, "rows": n,
                   "repeats": reps, "launches": launches[path]}
            rec.update(stats(xs))
            print(json.dumps(rec), flush=True)


def parent_window(fn, perm, bnd, change, vdata, vvalid):
    """The expression NDS Window ran per function before the native window
    op, from the sort order `perm` and the partition flags `bnd` on (`change`:
    the peer flags, for rank)."""
    n = perm.numel()
    dev = perm.device
    inv = torch.empty_like(perm)
    inv[perm] = torch.arange(n, dtype=torch.int64, device=dev)
    seg = torch.cumsum(bnd.to(torch.int64), 0) - 1
    nseg = int(seg[-1].item()) + 1
    seg_start = torch.zeros(nseg, dtype=torch.int64, device=dev)
    seg_start.scatter_(0, seg[bnd], torch.nonzero(
        bnd, as_tuple=False).view(-1))
    pos = torch.arange(n, dtype=torch.int64, device=dev) - \
        seg_start[seg]
    if fn == "sum":
        data = vdata[perm].to(torch.float64)
        vm = (vvalid[perm] if vvalid is not None
              else torch.ones(n, dtype=torch.bool, device=dev))
        acc = torch.zeros(nseg, dtype=torch.float64, device=dev)
        acc.index_add_(0, seg, torch.where(vm, data,
                                           torch.zeros_like(data)))
        res_sorted = acc[seg]
    elif fn == "cumsum":
        data = vdata[perm].to(torch.float64)
        vm = (vvalid[perm] if vvalid is not None
              else torch.ones(n, dtype=torch.bool, device=dev))
        data = torch.where(vm, data, torch.zeros_like(data))
        cs = torch.cumsum(data, 0)
        base = torch.zeros(nseg, dtype=torch.float64, device=dev)
        starts = torch.nonzero(bnd, as_tuple=False).view(-1)
        base[1:] = cs[starts[1:] - 1]
        res_sorted = cs - base[seg]
    else:  # rank (`pos`, above, is computed for every function)
        idx = torch.arange(n, dtype=torch.int64, device=dev)
        last_change = torch.cummax(
            torch.where(change, idx,
                        torch.full_like(idx, -1)), 0)[0]
        res_sorted = last_change - seg_start[seg] + 1
    return res_sorted[inv]


def window_bench(n, dev, g):
    """window_tensors against parent_window on rank over 2 partition keys
    plus 1 order key, a partition sum and a running sum. Both sides start
    from the same sort order and boundary flags; the sort is not timed."""
    from spark_rapids_jni_amd.ops.sort import (key_change_flags,
                                               sort_order_tensors)
    from spark_rapids_jni_amd.ops.window import window_tensors
    ri = lambda hi: torch.randint(0, hi, (n,), device=dev, generator=g)
    # about 8 rows per partition, ties in the order key
    side = max(2, int((n / 8) ** 0.5))
    k1, k2, ok = ri(side), ri(side), ri(4)
    vdata = torch.randint(-400, 400, (n,), device=dev,
                          generator=g).to(torch.float64) / 4
    vvalid = torch.rand(n, device=dev, generator=g) < 0.9
    perm = sort_order_tensors([k1, k2, ok])
    bnd = key_change_flags([k1, k2], perm)
    change = key_change_flags([k1, k2, ok], perm)
    cases = {
        "rank": ([("rank", None, None, "rows")], "rank"),
        "partition_sum": ([("sum", vdata, vvalid, "partition")], "sum"),
        "cumsum": ([("sum", vdata, vvalid, "rows")], "cumsum"),
    }
    reps = 20
    inner = 20 if n <= 2**16 else 1
    for name, (funcs, fn) in cases.items():
        new = lambda: window_tensors(perm, bnd, funcs, change)[0][0]
        old = lambda: parent_window(fn, perm, bnd, change, vdata, vvalid)
        # quarter-integers: every order of summation is exact
        assert torch.equal(new().to(torch.float64),
                           old().to(torch.float64)), name
        new_s, old_s = ab_time(new, old, inner, repeats=reps)
        launches = {"hip": count_launches(new),
                    "torch_parent": count_launches(old)}
        for path, xs in (("hip", new_s), ("torch_parent", old_s)):
            xs = sorted(xs)
            print(json.dumps({
                "bench": "window_" + name, "path": path, "rows": n,
                "repeats": reps, "launches": launches[path],
                "ms": round(xs[len(xs) // 2] * 1e3, 4),
                "ms_min": round(xs[0] * 1e3, 4),
                "ms_max": round(xs[-1] * 1e3, 4)}), flush=True)


def window_rolling_bench(n, part_rows, dev, g):
    """lag(1) and sum / max over bounded ROWS frames: window_tensors against
    the torch expression a caller can write today (the CPU twin of
    ops/window.py on CUDA tensors: one shifted, masked read per offset), and
    the kernel's staged path against its direct path at the same width. Both
    sides start from the same sort order and flags; the sort is not timed."""
    from spark_rapids_jni_amd.ops import window as W
    from spark_rapids_jni_amd.ops.sort import (key_change_flags,
                                               sort_order_tensors)
    H = W.ROLL_MAX_REACH
    env = "SRJ_WINDOW_ROLLING_DIRECT"
    os.environ.pop(env, None)
    pk = torch.randint(0, max(1, n // part_rows), (n,), device=dev,
                       generator=g)
    ok = torch.randint(0, 2**40, (n,), device=dev, generator=g)
    vdata = torch.randint(-400, 400, (n,), device=dev,
                          generator=g).to(torch.float64) / 4
    vvalid = torch.rand(n, device=dev, generator=g) < 0.9
    perm = sort_order_tensors([pk, ok])
    bnd = key_change_flags([pk], perm)
    head = bnd != 0
    head[0] = True

    def native(funcs):
        return W.window_tensors(perm, bnd, funcs)[0][0]

    def direct(funcs):
        os.environ[env] = "1"
        try:
            return native(funcs)
        finally:
            del os.environ[env]

    def twin(funcs):
        fs = W._check_funcs(funcs, n, perm.device, False)
        return W._rolling_cpu(perm, head, fs)[0][0]

    def record(name, width, a, b, fa, fb):
        # both have run once (the equality check): size the timed window,
        # and spend no warm-up calls on a case that takes seconds
        slow = max(timeit(fa, 1, warmup=0), timeit(fb, 1, warmup=0))
        reps = 7 if slow < 0.5 else 3
        inner = 10 if slow < 0.005 else 1
        a_s, b_s = [], []
        for _ in range(reps):  # alternating, as ab_time
            a_s.append(timeit(fa, inner, warmup=2 if slow < 0.5 else 0))
            b_s.append(timeit(fb, inner, warmup=2 if slow < 0.5 else 0))
        for path, xs in ((a, a_s), (b, b_s)):
            xs = sorted(xs)
            print(json.dumps({
                "bench": "window_rolling_" + name, "path": path, "rows": n,
                "partition_rows": part_rows, "width": width, "repeats": reps,
                "calls_per_repeat": inner,
                "ms": round(xs[len(xs) // 2] * 1e3, 4),
                "ms_min": round(xs[0] * 1e3, 4),
                "ms_max": round(xs[-1] * 1e3, 4)}), flush=True)

    def frame(width):
        return ("rows", -(width // 2), width // 2)

    cases = [("lag", 1, [("lag", vdata, vvalid, 1)])]
    for width in (3, 9, 33, 2 * H + 3):
        for fn in ("sum", "max"):
            cases.append((fn, width, [(fn, vdata, vvalid, frame(width))]))
    for name, width, funcs in cases:
        # the twin folds in the kernel's order: the same bits
        assert torch.equal(native(funcs), twin(funcs)), (name, width)
        record(name, width, "hip", "torch_twin", lambda: native(funcs),
               lambda: twin(funcs))
    for width in (3, 9, 33, 257, 2 * H + 1):
        for fn in ("sum", "max"):
            funcs = [(fn, vdata, vvalid, frame(width))]
            assert torch.equal(native(funcs), direct(funcs)), (fn, width)
            record(fn + "_paths", width, "staged", "direct",
                   lambda: native(funcs), lambda: direct(funcs))


def expr_bench(n, dev, g):
    """NDS eval_expr on the fused expression kernel against the same
    eval_expr forced to its torch evaluator, alternating in one process:
    a nullable filter predicate, a case_when product and a ratio with
    coalesce. The compiled program is memoised, as in a query run."""
    from spark_rapids_jni_amd.nds import expr as X
    from spark_rapids_jni_amd.nds.expr import Val, case_when, coalesce, col
    ri = lambda lo, hi: torch.randint(lo, hi, (n,), device=dev, generator=g,
                                      dtype=torch.int32)
    rf = lambda s: torch.rand(n, device=dev, generator=g,
                              dtype=torch.float64) * s
    rv = lambda p: torch.rand(n, device=dev, generator=g) < p
    env = {"qty": Val(ri(0, 100), rv(0.9)), "sk": Val(ri(1, 2000)),
           "year": Val(ri(1998, 2003), rv(0.95)),
           "price": Val(rf(200), rv(0.9)), "cost": Val(rf(100)),
           "disc": Val(rf(10), rv(0.5)), "zero": Val(ri(0, 3), rv(0.9))}
    c = col
    cases = {
        "filter": (c("qty").between(10, 60) & c("sk").isin([3, 5, 7, 11, 13])
                   | (c("year") == 2000) & (c("price") > 50.0)),
        "case_product": case_when((c("year") == 1999,
                                   c("qty") * c("price")), otherwise=0),
        "ratio_coalesce": coalesce((c("price") - c("cost")) / c("zero"),
                                   c("disc"), 0.0),
    }

    def run(e, force):
        def fn():
            X.FORCE_TORCH = force
            try:
                return X.eval_expr(e, env, n, dev)
            finally:
                X.FORCE_TORCH = False
        return fn

    reps = 20
    inner = 20 if n <= 2**16 else 1
    for name, e in cases.items():
        new, old = run(e, False), run(e, True)
        a, b = new(), old()
        assert a.data.dtype == b.data.dtype, name
        assert torch.equal(a.data, b.data), name  # no NaN in these shapes
        assert (a.valid is None) == (b.valid is None), name
        assert a.valid is None or torch.equal(a.valid, b.valid), name
        new_s, old_s = ab_time(new, old, inner, repeats=reps)
        launches = {"hip": count_launches(new), "torch": count_launches(old)}
        for path, xs in (("hip", new_s), ("torch", old_s)):
            xs = sorted(xs)
            print(json.dumps({
                "bench": "expr_" + name, "path": path, "rows": n,
                "repeats": reps, "launches": launches[path],
                "ms": round(xs[len(xs) // 2] * 1e3, 4),
                "ms_min": round(xs[0] * 1e3, 4),
                "ms_max": round(xs[-1] * 1e3, 4)}), flush=True)


def groupby_sorted_bench(n, dev, g):
    """ops.aggregate.groupby (hash table) against groupby_sorted (sort plus
    segmented reduce) on the whole call, sort and host syncs included: what
    the NDS engine pays per aggregate. A nullable float64 sum and a count
    over four key sets."""
    from spark_rapids_jni_amd.columnar import Column, DType, Table
    from spark_rapids_jni_amd.ops.aggregate import (Agg, _validity_from_bool,
                                                    groupby, groupby_sorted)
    ri = lambda hi: torch.randint(0, hi, (n,), device=dev, generator=g)
    icol = lambda t, valid=None: Column(
        DType.INT64, n, t, None if valid is None
        else _validity_from_bool(valid), null_count=None)
    # quarter-integers: every order of summation is exact
    vdata = torch.randint(-400, 400, (n,), device=dev,
                          generator=g).to(torch.float64) / 4
    vvalid = torch.rand(n, device=dev, generator=g) < 0.9
    vcol = Column(DType.FLOAT64, n, vdata, _validity_from_bool(vvalid),
                  null_count=None)
    aggs = [(Agg.SUM, vcol), (Agg.COUNT_ALL, None)]
    fkey = torch.randint(0, 1000, (n,), device=dev,
                         generator=g).to(torch.float64) / 8
    knull = torch.rand(n, device=dev, generator=g) < 0.9
    cases = {
        "i64_100_groups": ([icol(ri(100))], None),
        "i64_n4_groups": ([icol(ri(max(1, n // 4)))], None),
        "dict3_one_nullable": ([icol(ri(8)), icol(ri(16), knull),
                                icol(ri(4))], [10, 10, 10]),
        "f64_generic": ([Column(DType.FLOAT64, n, fkey)], None),
    }
    reps = 20
    inner = 20 if n <= 2**16 else 1
    for name, (kcols, bits) in cases.items():
        new = lambda: groupby_sorted(Table(kcols), aggs, key_bits=bits)
        old = lambda: groupby(Table(kcols), aggs)
        (nk, nr), (ok, orr) = new(), old()
        assert nk.num_rows == ok.num_rows, name
        for a, b in zip(nr, orr):
            assert torch.equal(a.data.sum(), b.data.sum()), name
        new_s, old_s = ab_time(new, old, inner, repeats=reps)
        launches = {"sorted": count_launches(new),
                    "hash": count_launches(old)}
        for path, xs in (("sorted", new_s), ("hash", old_s)):
            xs = sorted(xs)
            print(json.dumps({
                "bench": "groupby_sorted", "keys": name, "path": path,
                "rows": n, "groups": nk.num_rows, "repeats": reps,
                "launches": launches[path],
                "ms": round(xs[len(xs) // 2] * 1e3, 4),
                "ms_min": round(xs[0] * 1e3, 4),
                "ms_max": round(xs[-1] * 1e3, 4)}), flush=True)


def join_narrow_bench(nb, npr, iters, dev, g):
    """Narrow (8-byte slot) against wide (16-byte slot) join table on the same
    dense int64 keys, build and probe timed separately and alternating. The
    build time includes the zero fill of the table and, for the automatic
    narrow choice, the min/max scan with its read-back."""
    from spark_rapids_jni_amd.columnar import Column, DType
    from spark_rapids_jni_amd.ops.join import HashJoinTable
    bcol = Column(DType.INT64, nb, torch.randperm(nb, dtype=torch.int64,
                                                  device=dev, generator=g))
    pcol = Column(DType.INT64, npr, torch.randint(
        0, 2 * nb, (npr,), dtype=torch.int64, device=dev, generator=g))
    tables = {}

    def build(narrow):
        def run():
            tables[narrow] = None  # one table resident at a time
            tables[narrow] = HashJoinTable.build(bcol, narrow=narrow)
        return run

    def probe(narrow):
        return lambda: tables[narrow].inner_join(pcol, out_hint=npr)

    for phase, fn in (("build", build), ("probe", probe)):
        rows = nb if phase == "build" else npr
        if phase == "probe":
            tables[True] = HashJoinTable.build(bcol, narrow=True)
            tables[False] = HashJoinTable.build(bcol, narrow=False)
        nar, wide = ab_time(fn(True), fn(False), iters, repeats=3)
        for path, xs in (("narrow", nar), ("wide", wide)):
            xs = sorted(xs)
            print(json.dumps({
                "bench": f"join_narrow_{phase}", "path": path,
                "build_rows": nb, "probe_rows": npr,
                "ms": round(xs[1] * 1e3, 4), "ms_min": round(xs[0] * 1e3, 4),
                "ms_max": round(xs[2] * 1e3, 4),
                "rows_per_sec": round(rows / xs[1], 1)}), flush=True)
    tables.clear()


def join_dense_bench(nb, npr, iters, dev, g):
    """Dense (direct-address) against narrow (8-byte hashed slot) join table,
    both forced, on the same duplicate-free int64 keys, sorted and shuffled;
    build and probe timed separately and alternating. The build time includes
    the zero fill, the min/max scan with its read-back and, for dense, the
    read-back of the duplicate flag."""
    from spark_rapids_jni_amd.columnar import Column, DType
    from spark_rapids_jni_amd.ops.join import HashJoinTable
    keys = torch.arange(nb, dtype=torch.int64, device=dev)
    pcol = Column(DType.INT64, npr, torch.randint(
        0, 2 * nb, (npr,), dtype=torch.int64, device=dev, generator=g))
    kw = {"dense": {"dense": True}, "narrow": {"narrow": True}}
    for order in ("sorted", "shuffled"):
        if order == "shuffled":
            keys = keys[torch.randperm(nb, device=dev, generator=g)]
        bcol = Column(DType.INT64, nb, keys)
        tables = {}

        def build(path):
            def run():
                tables[path] = None  # one table resident at a time
                tables[path] = HashJoinTable.build(bcol, **kw[path])
            return run

        def probe(path):
            return lambda: tables[path].inner_join(pcol, out_hint=npr)

        for phase, fn in (("build", build), ("probe", probe)):
            rows = nb if phase == "build" else npr
            if phase == "probe":
                for path in kw:
                    tables[path] = HashJoinTable.build(bcol, **kw[path])
                assert tables["dense"].layout == "dense"
                assert tables["narrow"].layout == "narrow"
            den, nar = ab_time(fn("dense"), fn("narrow"), iters, repeats=3)
            for path, xs in (("dense", den), ("narrow", nar)):
                xs = sorted(xs)
                print(json.dumps({
                    "bench": f"join_dense_{phase}", "path": path,
                    "keys": order, "build_rows": nb, "probe_rows": npr,
                    "ms": round(xs[1] * 1e3, 4),
                    "ms_min": round(xs[0] * 1e3, 4),
                    "ms_max": round(xs[2] * 1e3, 4),
                    "rows_per_sec": round(rows / xs[1], 1)}), flush=True)
        tables.clear()


def join_ordered_bench(nb, npr, iters, dev, g):
    """Ordered (no table) against dense (direct-address table), both forced,
    on the same sorted int64 keys; build and probe timed separately and
    alternating. The ordered build is the key scan and its read-back; the
    dense build is the min/max scan with its read-back, the zero fill, the
    build kernel and the read-back of its duplicate flag."""
    from spark_rapids_jni_amd.columnar import Column, DType
    from spark_rapids_jni_amd.ops.join import HashJoinTable
    bcol = Column(DType.INT64, nb,
                  torch.arange(nb, dtype=torch.int64, device=dev) + 100)
    pcol = Column(DType.INT64, npr, torch.randint(
        0, 2 * nb, (npr,), dtype=torch.int64, device=dev, generator=g))
    kw = {"ordered": {"ordered": True}, "dense": {"dense": True}}
    tables = {}

    def build(path):
        def run():
            tables[path] = None  # one table resident at a time
            tables[path] = HashJoinTable.build(bcol, **kw[path])
        return run

    def probe(path):
        return lambda: tables[path].inner_join(pcol, out_hint=npr)

    for phase, fn in (("build", build), ("probe", probe)):
        rows = nb if phase == "build" else npr
        if phase == "probe":
            for path in kw:
                tables[path] = HashJoinTable.build(bcol, **kw[path])
                assert tables[path].layout == path
            a, b = probe("ordered")(), probe("dense")()
            assert a[0].numel() == b[0].numel()
            assert torch.equal((a[0] ^ a[1]).sum(), (b[0] ^ b[1]).sum())
            del a, b
        ordd, den = ab_time(fn("ordered"), fn("dense"), iters, repeats=3)
        for path, xs in (("ordered", ordd), ("dense", den)):
            xs = sorted(xs)
            print(json.dumps({
                "bench": f"join_ordered_{phase}", "path": path,
                "build_rows": nb, "probe_rows": npr,
                "ms": round(xs[1] * 1e3, 4),
                "ms_min": round(xs[0] * 1e3, 4),
                "ms_max": round(xs[2] * 1e3, 4),
                "rows_per_sec": round(rows / xs[1], 1)}), flush=True)
    tables.clear()


def join_modes_bench(nb, npr, iters, dev, g):
    """Semi, anti and left outer joins as emit modes of the fast-path probe
    (semi_select, left_outer_join) against the parent's expressions, copied
    here: HashJoinTable.semi_join, and inner_join plus make_left_outer. Forced
    wide, narrow and dense tables over the same duplicate-free int64 keys;
    probe keys uniform over nb / rate values, so `rate` of them match. The two
    paths alternate; results are compared before timing. The parent's semi
    join is timed as NDS pays it, on a table that was built for this join
    alone: its generic second table is dropped before every call."""
    from spark_rapids_jni_amd.columnar import Column, DType
    from spark_rapids_jni_amd.ops.join import HashJoinTable, make_left_outer
    bcol = Column(DType.INT64, nb, torch.randperm(nb, dtype=torch.int64,
                                                  device=dev, generator=g))
    kw = {"wide": {"narrow": False}, "narrow": {"narrow": True},
          "dense": {"dense": True}}

    def pair_key(bi, pi):
        return torch.sort(pi * (nb + 1) + (bi.long() + 1))[0]

    for rate in (0.1, 0.5, 1.0):
        pcol = Column(DType.INT64, npr, torch.randint(
            0, int(nb / rate), (npr,), dtype=torch.int64, device=dev,
            generator=g))
        for layout in kw:
            tbl = HashJoinTable.build(bcol, **kw[layout])
            assert tbl.layout == layout

            def parent_semi(anti):
                def run():
                    if hasattr(tbl, "_generic"):
                        del tbl._generic
                    return tbl.semi_join(pcol, anti=anti)
                return run

            def parent_left():
                bi, pi = tbl.inner_join(pcol)
                return make_left_outer(npr, bi, pi)

            cells = {
                "semi": (lambda: tbl.semi_select(pcol), parent_semi(False)),
                "anti": (lambda: tbl.semi_select(pcol, anti=True),
                         parent_semi(True)),
                "left": (lambda: tbl.left_outer_join(pcol), parent_left),
            }
            for kind, (new_fn, old_fn) in cells.items():
                a, b = new_fn(), old_fn()
                if kind == "left":
                    assert torch.equal(pair_key(*a), pair_key(*b))
                    out_rows = a[0].numel()
                else:
                    assert torch.equal(a, torch.sort(b)[0])
                    out_rows = a.numel()
                del a, b
                new_s, old_s = ab_time(new_fn, old_fn, iters, repeats=3)
                for path, xs in (("native", new_s), ("parent", old_s)):
                    xs = sorted(xs)
                    print(json.dumps({
                        "bench": "join_modes", "layout": layout, "kind": kind,
                        "match_rate": rate, "path": path, "build_rows": nb,
                        "probe_rows": npr, "out_rows": out_rows,
                        "ms": round(xs[1] * 1e3, 4),
                        "ms_min": round(xs[0] * 1e3, 4),
                        "ms_max": round(xs[2] * 1e3, 4),
                        "rows_per_sec": round(npr / xs[1], 1)}), flush=True)
            tbl = None


def plumbing_bench():
    """BASELINE config[0]: murmur3 + row<->columnar on a 1k-row int64 batch
    via the HOST path (no GPU) — measures binding/plumbing overhead like the
    reference's Java/JNI host path."""
    import io
    import numpy as np
    from spark_rapids_jni_amd import _native, kudo
    from spark_rapids_jni_amd.columnar import Column, DType
    host = _native.host()
    n = 1000
    keys = torch.arange(n, dtype=torch.int64)
    out = torch.empty(n, dtype=torch.int32)
    col = Column.from_torch(keys)
    iters = 2000
    t0 = time.perf_counter()
    for _ in range(iters):
        host.murmur3_long_host(keys.data_ptr(), n, 42, out.data_ptr())
        b = io.BytesIO()
        kudo.write_partition([col], 0, n, b)
        kudo.merge_on_host([b.getvalue()], [col])
    dt = (time.perf_counter() - t0) / iters
    print(json.dumps({"bench": "host_plumbing_murmur3_rowcol_1k",
                      "rows": n, "us_per_batch": round(dt * 1e6, 1),
                      "rows_per_sec": round(n / dt, 1)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=2**24)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--only", choices=["sort_order", "join_narrow",
                                      "join_dense", "join_ordered",
                                      "join_modes", "window",
                                      "window_rolling", "expr",
                                      "groupby_sorted"],
                    default=None,
                    help="run just this group")
    args = ap.parse_args()
    if args.only == "window_rolling":
        g = torch.Generator(device="cuda")
        g.manual_seed(7)
        # 2^20 and 2^24 rows; --rows N measures N rows alone
        for wn in ((2**20, 2**24) if args.rows == 2**24 else (args.rows,)):
            for part_rows in (1024, 16):
                window_rolling_bench(wn, part_rows, "cuda", g)
        return
    if args.only == "groupby_sorted":
        g = torch.Generator(device="cuda")
        g.manual_seed(7)
        for gn in (256, 2048, 2**16, 2**20, 2**24):
            groupby_sorted_bench(gn, "cuda", g)
        return
    if args.only == "window":
        g = torch.Generator(device="cuda")
        g.manual_seed(7)
        for wn in (2**11, 2**16, 2**20, 2**24):
            window_bench(wn, "cuda", g)
        return
    if args.only == "expr":
        g = torch.Generator(device="cuda")
        g.manual_seed(7)
        for en in (2**11, 2**16, 2**20, 2**24):
            expr_bench(en, "cuda", g)
        return
    if args.only == "sort_order":
        g = torch.Generator(device="cuda")
        g.manual_seed(7)
        for sn in (256, 2048, 2**16, args.rows):
            sort_order_bench(sn, 20, "cuda", g)
        return
    if args.only == "join_narrow":
        g = torch.Generator(device="cuda")
        g.manual_seed(7)
        # beyond the Infinity Cache, then cache resident
        for nb, npr in ((2**26, 2**26), (2**20, 2**24)):
            join_narrow_bench(nb, npr, args.iters, "cuda", g)
        return
    if args.only == "join_dense":
        g = torch.Generator(device="cuda")
        g.manual_seed(7)
        # beyond the Infinity Cache, then cache resident
        for nb, npr in ((2**26, 2**26), (2**20, 2**24)):
            join_dense_bench(nb, npr, args.iters, "cuda", g)
        return
    if args.only == "join_ordered":
        g = torch.Generator(device="cuda")
        g.manual_seed(7)
        # beyond the Infinity Cache, then cache resident
        for nb, npr in ((2**26, 2**26), (2**20, 2**24)):
            join_ordered_bench(nb, npr, args.iters, "cuda", g)
        return
    if args.only == "join_modes":
        g = torch.Generator(device="cuda")
        g.manual_seed(7)
        # cache resident, then beyond the Infinity Cache
        for nb, npr in ((2**20, 2**24), (2**26, 2**26)):
            join_modes_bench(nb, npr, args.iters, "cuda", g)
        return
    plumbing_bench()  # CPU shape (BASELINE config[0]) first
    n = args.rows
    dev = "cuda"

    from spark_rapids_jni_amd.columnar import Column, DType, Table
    from spark_rapids_jni_amd.ops import cast, hashing, misc
    from spark_rapids_jni_amd.ops.row_conversion import (convert_from_rows,
                                                         convert_to_rows)
    from spark_rapids_jni_amd.ops.json import (get_json_object,
                                               get_json_object_multiple_paths)
    from spark_rapids_jni_amd.ops.sketch import parse_uri, UriPart

    g = torch.Generator(device=dev)
    g.manual_seed(7)

    # 1. row transpose: mixed fixed-width table (reference: 212 mixed columns
    #    at 2^10..2^26 rows; here 24 columns x 8 type-pattern, scaled rows)
    cols = []
    dtypes = [DType.INT64, DType.INT32, DType.FLOAT64, DType.FLOAT32,
              DType.INT16, DType.INT8, DType.BOOL8, DType.TIMESTAMP_US] * 3
    for dt in dtypes:
        from spark_rapids_jni_amd.columnar import TORCH_DTYPE
        t = torch.randint(0, 100, (n // 16,), dtype=torch.int64,
                          device=dev, generator=g).to(TORCH_DTYPE[dt])
        cols.append(Column(dt, n // 16, t))
    tbl = Table(cols)
    batches = None

    def to_rows():
        nonlocal batches
        batches = convert_to_rows(tbl)

    secs = timeit(to_rows, args.iters)
    row_size = batches[0][0].numel() // batches[0][1]
    emit("row_conversion_to_rows", n // 16, secs,
         (n // 16) * row_size)
    secs = timeit(lambda: convert_from_rows(batches, dtypes), args.iters)
    emit("row_conversion_from_rows", n // 16, secs, (n // 16) * row_size)

    # 2. string -> float
    fvals = torch.rand(n // 4, dtype=torch.float64, device=dev,
                       generator=g) * 1e6 - 5e5
    fstr = cast.from_floats(Column(DType.FLOAT64, n // 4, fvals))
    secs = timeit(lambda: cast.to_float(fstr), args.iters)
    emit("string_to_float", n // 4, secs,
         int(fstr.offsets[-1].item()))

    # 3. long -> "binary" (base-2) string via conv, plus hex
    lvals = torch.randint(0, 2**62, (n // 4,), dtype=torch.int64, device=dev,
                          generator=g)
    lstr = cast.from_integer(Column(DType.INT64, n // 4, lvals))
    from spark_rapids_jni_amd.ops.sketch import convert_base
    secs = timeit(lambda: convert_base(lstr, 10, 2), args.iters)
    emit("long_to_binary_string", n // 4, secs)

    # 4. bloom filter build + probe
    keys = torch.randint(0, 2**40, (n,), dtype=torch.int64, device=dev,
                         generator=g)
    kc = Column(DType.INT64, n, keys)
    bf = misc.BloomFilter(2, 3, 1 << 20, seed=42)
    secs = timeit(lambda: bf.put(kc), args.iters)
    emit("bloom_filter_build", n, secs)
    secs = timeit(lambda: bf.might_contain(kc), args.iters)
    emit("bloom_filter_probe", n, secs)

    # 5. get_json_object, 1..4 paths over the same docs
    docs = ['{"a":%d,"b":{"c":"x%d"},"d":[%d,%d],"e":"v"}' %
            (i, i % 97, i, i + 1) for i in range(200_000)]
    jc = Column.from_pylist(docs, DType.STRING, dev)
    paths = ["$.a", "$.b.c", "$.d[1]", "$.e"]
    for k in (1, 2, 4):
        def run_paths(k=k):
            if k == 1:
                get_json_object(jc, paths[0])
            else:
                get_json_object_multiple_paths(jc, paths[:k])
        secs = timeit(run_paths, args.iters)
        emit(f"get_json_object_{k}path", jc.size * k, secs,
             int(jc.offsets[-1].item()) * k)

    # 5b. generic (multi-column) hash join probe — the non-int64 join path
    from spark_rapids_jni_amd.ops.join import HashJoinTable
    nb = n // 2
    npr = n
    k1 = torch.randint(0, nb, (nb,), dtype=torch.int32, device=dev, generator=g)
    k2 = torch.randint(0, 8, (nb,), dtype=torch.int32, device=dev, generator=g)
    btbl = Table([Column.from_torch(k1), Column.from_torch(k2)])
    p1 = torch.randint(0, nb, (npr,), dtype=torch.int32, device=dev,
                       generator=g)
    p2 = torch.randint(0, 8, (npr,), dtype=torch.int32, device=dev,
                       generator=g)
    ptbl = Table([Column.from_torch(p1), Column.from_torch(p2)])
    tbl = HashJoinTable.build(btbl)
    secs = timeit(lambda: tbl.inner_join(ptbl, out_hint=npr // 4), args.iters)
    emit("generic_join_probe_2col", npr, secs)

    # 5c. radix sort (north-star hot op; reference delegates to cub/cudf)
    from spark_rapids_jni_amd.ops.sort import sort_pairs_i64
    skeys = torch.randint(-2**62, 2**62, (n,), dtype=torch.int64, device=dev,
                          generator=g)
    secs = timeit(lambda: sort_pairs_i64(skeys), args.iters)
    emit("radix_sort_int64", n, secs, n * 8)

    # 6. parse_uri
    uris = ["https://host%d.example.com:80/p/%d?k=%d&z=9" % (i % 50, i, i)
            for i in range(200_000)]
    uc = Column.from_pylist(uris, DType.STRING, dev)
    secs = timeit(lambda: parse_uri(uc, UriPart.HOST), args.iters)
    emit("parse_uri_host", uc.size, secs, int(uc.offsets[-1].item()))
    secs = timeit(lambda: parse_uri(uc, UriPart.QUERY_KEY, "k"), args.iters)
    emit("parse_uri_query_key", uc.size, secs)

    # 7. stream compaction / fused multi-column gather vs the torch
    #    expressions they replaced
    compact_bench(n, args.iters, dev, g)

    # 8. multi-key sort order vs the per-key torch.argsort expression
    for sn in (256, 2048, 2**16, n):
        sort_order_bench(sn, args.iters, dev, g)


if __name__ == "__main__":
    main()
