"""Window functions over a sorted order (Spark WindowExec's GPU half; cudf
grouped scans and rolling aggregations over unbounded frames).

`window_tensors` takes the permutation that sorts the rows by (partition keys,
order keys) and the partition / peer boundary flags of the sorted rows - what
`sort_order_tensors` and `key_change_flags` give - and evaluates any number of
window functions in one call of the segmented-scan kernels of
src/gpu/window.hip. Values are read in place through the permutation and
results land in original row order. `window_columns` is the same on Tables.

Functions: row_number, rank, dense_rank, count, sum, min, max, avg. Frames of
the five aggregates: "partition" (the whole partition), "rows" (unbounded
preceding to the current row) and "range" (unbounded preceding through the
current row's last peer: Spark's default frame under an ORDER BY). Ranking
functions ignore the frame.

Rolling functions (src/gpu/window_rolling.hip, cudf's rolling aggregations):
the five aggregates also take the bounded frame `("rows", lo, hi)`, ROWS
BETWEEN -lo PRECEDING AND hi FOLLOWING clipped to the partition, with signed
ints lo <= hi: `("rows", -2, 0)` is "2 preceding to the current row",
`("rows", -3, -1)` leaves the current row out. `("lag" | "lead", values,
valid, k)` is the value k rows before / after the row in its partition (a
negative k swaps the direction), null where that row does not exist or is
null; there is no ignore-nulls and no default value, callers coalesce. Every
output row folds its own frame in ascending position, so results are exact
and the same bits on every run, float sums included; the cost is O(m * frame
width) and there is no cap on the width. Frames unbounded on one side and
bounded on the other (an offset of None) are not implemented.

Semantics (Spark, non-ANSI): aggregates skip nulls; count is int64 and never
null; sum is int64 (wrapping) for integer and bool input and float64 for float
input; min and max keep the input dtype, with NaN greater than every value;
avg accumulates and divides in float64; sum, min, max and avg are null (data
zero) where the frame holds no valid value. Ranking results are int64.

CPU tensors take an equivalent torch expression; CUDA tensors always take the
native kernels: no host sync (the op runs under stream capture), no atomics,
and the same input gives bit-identical output on every run.
"""
from typing import List, Optional, Sequence, Tuple

import torch

from .. import _native
from ..columnar import Column, DType, Table, validity_to_bool
from ._segscan import (CARRY_CHUNK, ROLL_MAX_OFFSET,  # noqa: F401
                       ROLL_MAX_REACH, ROLL_TILE_ROWS, SMALL_ROWS, TILE_ROWS,
                       _BYTE_DTYPES, _FRAMES, _FUNCS, _RANKING, _SHIFTS,
                       _Func, _RollFunc, _check_values, _descriptor,
                       _outputs, _roll_descriptor, _work_buffer)
from ._segscan import MAX_FUNCS as WINDOW_MAX_FUNCS


def window_work_bytes(m: int, nfuncs: int) -> int:
    """Bytes of scratch one kernel call over m rows and nfuncs functions
    takes (zero on the one-workgroup path)."""
    return _native.gpu().window_work_bytes(m, nfuncs)


def _check_flags(t, what, m, dev):
    if not isinstance(t, torch.Tensor) or t.dtype not in _BYTE_DTYPES:
        raise TypeError(f"{what} must be a bool, uint8 or int8 tensor")
    if t.dim() != 1 or t.numel() != m:
        raise ValueError(f"{what} must be 1-D with {m} rows")
    if t.device != dev:
        raise ValueError(f"{what} and perm are on different devices")
    return t.contiguous()


def _check_funcs(funcs, m, dev, have_peer) -> List[_Func]:
    out = []
    for i, spec in enumerate(funcs):
        if len(spec) != 4:
            raise ValueError(f"funcs[{i}] must be (fn, values, valid, frame)")
        fn, values, valid, frame = spec
        if fn in _SHIFTS:
            if isinstance(frame, (str, tuple, list)):
                raise ValueError(f"funcs[{i}]: {fn} takes a row offset k, "
                                 f"not the frame {frame!r}")
            k = _check_offset(i, "k", frame)
            if values is None:
                raise ValueError(f"funcs[{i}]: {fn} needs values")
            valid = _check_values(i, fn, values, valid, m, dev, "perm")
            shift = -k if fn == "lag" else k
            out.append(_RollFunc(fn, values, valid, shift, shift, shift))
            continue
        if fn not in _FUNCS:
            raise ValueError(f"funcs[{i}]: unknown function {fn!r}")
        if fn in _RANKING:
            if not have_peer:
                raise ValueError(f"funcs[{i}]: {fn} needs peer_flags")
            if values is not None or valid is not None:
                raise ValueError(f"funcs[{i}]: {fn} takes no values")
            out.append(_Func(fn, None, None, "rows"))
            continue
        if isinstance(frame, (tuple, list)):
            if len(frame) != 3 or frame[0] != "rows":
                raise ValueError(f"funcs[{i}]: unknown frame {frame!r}")
            if frame[1] is None or frame[2] is None:
                raise NotImplementedError(
                    f"funcs[{i}]: the frame {frame!r} is unbounded on one "
                    "side; only bounded ROWS frames and the string frames "
                    "'partition', 'rows' and 'range' are implemented")
            lo = _check_offset(i, "lo", frame[1])
            hi = _check_offset(i, "hi", frame[2])
            if lo > hi:
                raise ValueError(f"funcs[{i}]: frame {frame!r} has lo > hi")
            valid = _check_values(i, fn, values, valid, m, dev, "perm")
            out.append(_RollFunc(fn, values, valid, lo, hi))
            continue
        if not isinstance(frame, str) or frame not in _FRAMES:
            raise ValueError(f"funcs[{i}]: unknown frame {frame!r}")
        valid = _check_values(i, fn, values, valid, m, dev, "perm")
        out.append(_Func(fn, values, valid, frame))
    return out


def _check_offset(i, what, x):
    if isinstance(x, bool) or not isinstance(x, int):
        raise TypeError(f"funcs[{i}]: {what} must be an int, got {x!r}")
    if abs(x) > ROLL_MAX_OFFSET:
        raise ValueError(f"funcs[{i}]: {what} = {x} is beyond "
                         "+-(2**31 - 1) rows")
    return x


# ---------------------------------------------------------------------------
# CPU twin
# ---------------------------------------------------------------------------

def _merge(op, ca, aa, cb, ab):
    """Accumulator of `a` (left) combined with `b`; counts decide validity
    for min and max, sums hold zero under nulls."""
    if op == "sum":
        return aa + ab
    if op == "none":
        return ab
    if op == "maxidx":
        return torch.maximum(aa, ab)
    if aa.dtype.is_floating_point:
        # NaN greatest: maximum propagates NaN, fmin drops it
        both = torch.maximum(aa, ab) if op == "max" else torch.fmin(aa, ab)
    else:
        both = torch.maximum(aa, ab) if op == "max" else torch.minimum(aa, ab)
    return torch.where(ca == 0, ab, torch.where(cb == 0, aa, both))


def _seg_scan_cpu(head, cnt, acc, op):
    """Inclusive segmented scan by doubling: the torch twin of the kernels'
    scan (same operator, another association)."""
    m = head.numel()
    flag = head.clone()
    d = 1
    while d < m:
        take = ~flag[d:]
        zero = torch.zeros_like(cnt[:-d])
        merged = _merge(op, cnt[:-d], acc[:-d], cnt[d:], acc[d:])
        acc = torch.cat([acc[:d], torch.where(take, merged, acc[d:])])
        cnt = torch.cat([cnt[:d], cnt[d:] + torch.where(take, cnt[:-d],
                                                        zero)])
        flag = torch.cat([flag[:d], flag[d:] | flag[:-d]])
        d *= 2
    return cnt, acc


def _frame_last(head):
    """Last sorted position of the segment each position lies in."""
    m = head.numel()
    idx = torch.arange(m, dtype=torch.int64, device=head.device)
    nxt = torch.where(head, idx, torch.full_like(idx, m))
    nxt = torch.flip(torch.cummin(torch.flip(nxt, [0]), 0)[0], [0])
    return torch.cat([nxt[1:], nxt.new_full((1,), m)]) - 1


def _window_cpu(perm, part, peer, fs: List[_Func]):
    m = perm.numel()
    dev = perm.device
    idx = torch.arange(m, dtype=torch.int64, device=dev)
    ends = {"rows": idx, "partition": _frame_last(part),
            "range": _frame_last(peer)}
    ones = torch.ones(m, dtype=torch.int64, device=dev)
    results = []
    for f in fs:
        if f.fn in _RANKING:
            if f.fn == "dense_rank":
                cnt, _ = _seg_scan_cpu(part, peer.to(torch.int64), ones,
                                       "none")
                res = cnt
            else:
                cnt, last_peer = _seg_scan_cpu(
                    part, ones, torch.where(peer, idx, -ones), "maxidx")
                res = cnt if f.fn == "row_number" else cnt - idx + last_peer
            data = torch.empty_like(res)
            data[perm] = res
            results.append((data, None))
            continue
        valid = (f.valid[perm] != 0 if f.valid is not None
                 else torch.ones(m, dtype=torch.bool, device=dev))
        cnt = valid.to(torch.int64)
        if f.fn == "count":
            acc, op = ones, "none"
        else:
            v = f.values[perm]
            if f.fn == "avg" or v.dtype.is_floating_point:
                acc = v.to(torch.float64)
            else:
                acc = v.to(torch.int64)
            op = "sum" if f.fn in ("sum", "avg") else f.fn
            acc = torch.where(valid, acc, torch.zeros_like(acc))
        cnt, acc = _seg_scan_cpu(part, cnt, acc, op)
        e = ends[f.frame]
        cnt, acc = cnt[e], acc[e]
        has = cnt > 0
        if f.fn == "count":
            res = cnt
        elif f.fn == "avg":
            res = acc / cnt.clamp(min=1).to(torch.float64)
        else:
            res = acc
            res = torch.where(has, res, torch.zeros_like(res))
        res = res.to(f.out_dtype())
        data = torch.empty_like(res)
        data[perm] = res
        ov = None
        if f.nullable():
            ov = torch.empty(m, dtype=torch.bool, device=dev)
            ov[perm] = has
        results.append((data, ov))
    return results


def _roll_merge(op, ca, aa, cb, ab):
    """_merge with the kernel's choice among equals spelled out, so that the
    bits agree: seg_max_f / seg_min_f keep the left side only where it is
    strictly greater / less, so of -0.0 and 0.0 the later one wins."""
    if op == "sum":
        return aa + ab
    if aa.dtype.is_floating_point:
        an, bn = aa != aa, ab != ab
        if op == "max":
            left = an | (~bn & (aa > ab))
        else:
            left = ~an & (bn | (aa < ab))
        both = torch.where(left, aa, ab)
    else:
        both = torch.maximum(aa, ab) if op == "max" else torch.minimum(aa, ab)
    return torch.where(ca == 0, ab, torch.where(cb == 0, aa, both))


def _rolling_cpu(perm, part, fs: List[_RollFunc]):
    """The torch twin of the rolling kernel: one shifted, masked read per
    offset lo..hi in ascending order, accumulated from the empty state with
    the kernel's operator. Both add in the same order from +0.0, so the twin
    equals the kernel bit for bit, float sums included."""
    m = perm.numel()
    dev = perm.device
    idx = torch.arange(m, dtype=torch.int64, device=dev)
    ps = torch.cummax(torch.where(part, idx, torch.zeros_like(idx)), 0)[0]
    pe = _frame_last(part)
    results = []
    for f in fs:
        valid = (f.valid[perm] != 0 if f.valid is not None
                 else torch.ones(m, dtype=torch.bool, device=dev))
        if f.fn in _SHIFTS:
            j = idx + f.shift
            has = (j >= ps) & (j <= pe)
            j = j.clamp(0, m - 1)
            has = has & valid[j]
            v = f.values[perm][j]
            res = torch.where(has, v, torch.zeros_like(v))
        else:
            item_cnt = valid.to(torch.int64)
            if f.fn == "count":
                item_acc, op = torch.zeros_like(item_cnt), "sum"
            else:
                v = f.values[perm]
                if f.fn == "avg" or v.dtype.is_floating_point:
                    item_acc = v.to(torch.float64)
                else:
                    item_acc = v.to(torch.int64)
                item_acc = torch.where(valid, item_acc,
                                       torch.zeros_like(item_acc))
                op = "sum" if f.fn in ("sum", "avg") else f.fn
            cnt = torch.zeros_like(item_cnt)
            acc = torch.zeros_like(item_acc)
            # offsets past the longest possible partition touch nothing
            for d in range(max(f.lo, -m), min(f.hi, m) + 1):
                j = idx + d
                inside = (j >= ps) & (j <= pe)
                j = j.clamp(0, m - 1)
                cb = torch.where(inside, item_cnt[j],
                                 torch.zeros_like(item_cnt))
                ab = torch.where(inside, item_acc[j],
                                 torch.zeros_like(item_acc))
                acc = _roll_merge(op, cnt, acc, cb, ab)
                cnt = cnt + cb
            has = cnt > 0
            if f.fn == "count":
                res = cnt
            elif f.fn == "avg":
                res = acc / cnt.clamp(min=1).to(torch.float64)
            else:
                res = torch.where(has, acc, torch.zeros_like(acc))
            res = res.to(f.out_dtype())
        data = torch.empty_like(res)
        data[perm] = res
        ov = None
        if f.nullable():
            ov = torch.empty(m, dtype=torch.bool, device=dev)
            ov[perm] = has
        results.append((data, ov))
    return results


# ---------------------------------------------------------------------------
# native path
# ---------------------------------------------------------------------------

def _rolling_gpu(perm, part, fs: List[_RollFunc]):
    """The rolling functions: the partition bounds of every sorted position
    once (row_number and count(*) over the partition, by the scan kernels
    over the identity permutation), then one launch of the rolling kernel per
    WINDOW_MAX_FUNCS functions."""
    g = _native.gpu()
    m = perm.numel()
    dev = perm.device
    stream = _native.current_stream()
    identity = torch.arange(m, dtype=torch.int64, device=dev)
    rn = torch.empty(m, dtype=torch.int64, device=dev)
    pcnt = torch.empty(m, dtype=torch.int64, device=dev)
    work = _work_buffer(g.window_work_bytes(m, 2), dev)
    g.window([(_FUNCS["row_number"], _FRAMES["rows"], 0, 1, 1, 0, 0,
               rn.data_ptr(), 0),
              (_FUNCS["count"], _FRAMES["partition"], 0, 1, 1, 0, 0,
               pcnt.data_ptr(), 0)],
             identity.data_ptr(), part.data_ptr(), 0, m,
             work.data_ptr() if work is not None else 0, stream)
    results = []
    for lo in range(0, len(fs), WINDOW_MAX_FUNCS):
        chunk = fs[lo:lo + WINDOW_MAX_FUNCS]
        descs = []
        for f in chunk:
            data, ov = _outputs(f, m, dev)
            descs.append(_roll_descriptor(f, m, data, ov))
            results.append((data, ov))
        g.window_rolling(descs, perm.data_ptr(), rn.data_ptr(),
                         pcnt.data_ptr(), m, stream)
    return results


def _window_gpu(perm, part, peer, fs: List[_Func], have_peer):
    g = _native.gpu()
    m = perm.numel()
    dev = perm.device
    stream = _native.current_stream()
    results = []
    for lo in range(0, len(fs), WINDOW_MAX_FUNCS):
        chunk = fs[lo:lo + WINDOW_MAX_FUNCS]
        descs = []
        for f in chunk:
            data, ov = _outputs(f, m, dev)
            descs.append(_descriptor(f, m, data, ov))
            results.append((data, ov))
        work = _work_buffer(g.window_work_bytes(m, len(chunk)), dev)
        g.window(descs, perm.data_ptr(), part.data_ptr(),
                 peer.data_ptr() if have_peer else 0, m,
                 work.data_ptr() if work is not None else 0, stream)
    return results


def window_tensors(perm: torch.Tensor, part_flags: torch.Tensor,
                   funcs: Sequence[Tuple],
                   peer_flags: Optional[torch.Tensor] = None
                   ) -> List[Tuple[torch.Tensor, Optional[torch.Tensor]]]:
    """Window functions over the sorted order `perm`.

    `part_flags[i]` / `peer_flags[i]` are nonzero where sorted position i
    starts a partition / a peer group (position 0 always does, and a
    partition head is a peer head, whatever the flags say). Without
    `peer_flags` every row is its own peer group. `funcs` is a list of
    `(fn, values, valid, frame)`: `values` and `valid` (a byte per row, zero
    = null) are indexed by original row and are None for the ranking
    functions and count(*). Returns one `(data, valid)` per function in
    original row order; `valid` is a bool tensor, or None for count, the
    ranking functions and inputs without validity.

    The rolling forms mix freely with these: `(fn, values, valid, ("rows",
    lo, hi))` for the five aggregates over the bounded frame of sorted
    positions [i + lo, i + hi] within the partition, and `("lag" | "lead",
    values, valid, k)`. lag and lead keep the input dtype and always return
    a `valid`; a bounded sum, min, max or avg returns one when the input has
    validity or the frame can leave the current row out (lo > 0 or hi < 0).
    Offsets are ints of at most 2**31 - 1 in magnitude; the cost is O(rows *
    (hi - lo + 1)) with no cap on the width. A frame with None for an offset
    (unbounded on one side) raises NotImplementedError.
    """
    if not isinstance(perm, torch.Tensor) or perm.dtype != torch.int64:
        raise TypeError("perm must be an int64 tensor")
    if perm.dim() != 1:
        raise ValueError(f"perm must be 1-D, got shape {tuple(perm.shape)}")
    m = perm.numel()
    dev = perm.device
    part = _check_flags(part_flags, "part_flags", m, dev)
    have_peer = peer_flags is not None
    peer = _check_flags(peer_flags, "peer_flags", m, dev) if have_peer \
        else None
    fs = _check_funcs(list(funcs), m, dev, have_peer)
    if m == 0:
        return [_outputs(f, 0, dev) for f in fs]
    if not fs:
        return []
    perm = perm.contiguous()
    # the scan group and the rolling group, each in the caller's order
    rolling = [isinstance(f, _RollFunc) for f in fs]
    scan_fs = [f for f, r in zip(fs, rolling) if not r]
    roll_fs = [f for f, r in zip(fs, rolling) if r]
    if dev.type == "cuda":
        scan = (_window_gpu(perm, part, peer, scan_fs, have_peer)
                if scan_fs else [])
        roll = _rolling_gpu(perm, part, roll_fs) if roll_fs else []
    else:
        part = part != 0
        part[0] = True
        peer = (peer != 0) | part if have_peer else torch.ones_like(part)
        scan = _window_cpu(perm, part, peer, scan_fs) if scan_fs else []
        roll = _rolling_cpu(perm, part, roll_fs) if roll_fs else []
    scan, roll = iter(scan), iter(roll)
    return [next(roll) if r else next(scan) for r in rolling]


_VALUE_COLUMNS = (DType.BOOL8, DType.INT8, DType.INT16, DType.INT32,
                  DType.INT64, DType.FLOAT32, DType.FLOAT64, DType.DATE32,
                  DType.TIMESTAMP_US)
_OUT_DTYPE = {torch.int8: DType.INT8, torch.int16: DType.INT16,
              torch.int32: DType.INT32, torch.int64: DType.INT64,
              torch.float32: DType.FLOAT32, torch.float64: DType.FLOAT64}


def window_columns(partition_by: Optional[Table], order_by: Optional[Table],
                   funcs, ascending: Optional[Sequence[bool]] = None,
                   nulls_first: Optional[Sequence] = None) -> List[Column]:
    """Window functions `funcs` = [(fn, Column or None, frame)] over the
    partitions of `partition_by` (None, a Table cannot be empty: one
    partition) ordered by
    `order_by` (`ascending` / `nulls_first` as in `sort_order`). Partition
    and order keys compare as the sort does: nulls equal each other, NaNs
    equal, -0.0 == 0.0. `frame` may be the bounded `("rows", lo, hi)`, and
    `("lag" | "lead", Column, k)` is accepted, as in `window_tensors`.
    Results are Columns in input row order."""
    from .aggregate import _validity_from_bool
    from .sort import _key_change_keys, _sort_order_keys, _table_keys
    funcs = list(funcs)
    pkeys = (_table_keys(partition_by, None, None)
             if partition_by is not None else [])
    okeys = (_table_keys(order_by, ascending, nulls_first)
             if order_by is not None else [])
    n = None
    for t in (partition_by, order_by):
        if t is not None:
            if n is not None and t.num_rows != n:
                raise ValueError(f"order_by has {t.num_rows} rows but "
                                 f"partition_by has {n}")
            n, dev = t.num_rows, t.device
    for i, spec in enumerate(funcs):
        if len(spec) != 3:
            raise ValueError(f"funcs[{i}] must be (fn, column, frame)")
        c = spec[1]
        if c is not None:
            if c.dtype not in _VALUE_COLUMNS:
                raise NotImplementedError(
                    f"window: {c.dtype.name} values are not supported")
            if n is None:
                n, dev = c.size, c.device
            if c.size != n:
                raise ValueError(f"funcs[{i}]: column has {c.size} rows but "
                                 f"the keys have {n}")
    if n is None:
        raise ValueError("window_columns needs a key or a value column")
    perm = _sort_order_keys(pkeys + okeys, n, torch.device(dev))
    if pkeys and n:
        part = _key_change_keys(pkeys, perm, n)
    else:
        part = torch.zeros(n, dtype=torch.bool, device=dev)
    # no order: the rows of a partition are all peers
    peer = _key_change_keys(pkeys + okeys, perm, n) if okeys and n else part
    specs = []
    for fn, c, frame in funcs:
        if c is None:
            specs.append((fn, None, None, frame))
        else:
            valid = (validity_to_bool(c.validity, c.size)
                     if c.validity is not None else None)
            specs.append((fn, c.data, valid, frame))
    out = []
    for (fn, c, _frame), (data, valid) in zip(
            funcs, window_tensors(perm, part, specs, peer)):
        if fn in ("min", "max") or fn in _SHIFTS:
            dt, scale = c.dtype, c.scale
        else:
            dt, scale = _OUT_DTYPE[data.dtype], 0
        mask = _validity_from_bool(valid) if valid is not None else None
        out.append(Column(dt, n, data, mask, scale=scale))
    return out
