"""Segmented reduce over a sorted order, and the sort-based group-by on top of
it (Spark's sort aggregate; cudf sort-based groupby and segmented reductions).

`segmented_reduce_tensors` takes the boundary flags of the sorted rows - what
`key_change_flags` gives - and optionally the permutation that sorts them, and
evaluates any number of aggregates in one call of the kernels of
src/gpu/seg_reduce.hip: one output row per segment. Values are read in place
through the permutation. `groupby_tensors` is sort, flags, reduce in one call;
`ops.aggregate.groupby_sorted` is the same on Tables.

Functions: count, sum, min, max, avg.

Semantics (Spark, non-ANSI; those of ops/window.py): aggregates skip nulls;
count is int64 and never null; sum is int64 (wrapping) for integer and bool
input and float64 for float input; min and max keep the input dtype, with NaN
greater than every value; avg accumulates and divides in float64; sum, min,
max and avg are null (data zero) where the segment holds no valid value.

CPU tensors take an equivalent torch expression (another association for
sums); CUDA tensors always take the native kernels: no host sync in
`segmented_reduce_tensors` (it runs under stream capture), no atomics, and the
same input gives bit-identical output on every run. Within a segment values
combine in sorted-position order, which after the stable sort of
`groupby_tensors` is input row order.
"""
from typing import List, Optional, Sequence, Tuple

import torch

from .. import _native
from ._segscan import (CARRY_CHUNK, SMALL_ROWS, TILE_ROWS,  # noqa: F401
                       _AGGREGATES, _BYTE_DTYPES, _Func,
                       _check_values, _descriptor, _outputs, _work_buffer)
from ._segscan import MAX_FUNCS as SEG_MAX_FUNCS


def seg_reduce_work_bytes(m: int, nfuncs: int) -> int:
    """Bytes of scratch one kernel call over m rows and nfuncs functions
    takes (zero on the one-workgroup path)."""
    return _native.gpu().seg_reduce_work_bytes(m, nfuncs)


def _check_funcs(funcs, m, dev) -> List[_Func]:
    out = []
    for i, spec in enumerate(funcs):
        if len(spec) != 3:
            raise ValueError(f"funcs[{i}] must be (fn, values, valid)")
        fn, values, valid = spec
        if fn not in _AGGREGATES:  # the ranking functions are the window's
            raise ValueError(f"funcs[{i}]: unknown function {fn!r}")
        valid = _check_values(i, fn, values, valid, m, dev, "head_flags")
        out.append(_Func(fn, values, valid))
    return out


# ---------------------------------------------------------------------------
# CPU twin
# ---------------------------------------------------------------------------

def _reduce_cpu(head, perm, fs: List[_Func], k):
    """head: normalised bool flags. Outputs of k rows: the first k segments,
    zero rows beyond the number of segments."""
    m = head.numel()
    dev = head.device
    seg = torch.cumsum(head.to(torch.int64), 0) - 1
    ng = int(seg[-1]) + 1
    pos = torch.nonzero(head).view(-1)

    def fit(t):
        if k <= ng:
            return t[:k].clone()
        return torch.cat([t, t.new_zeros(k - ng)])

    first = fit(perm[pos] if perm is not None else pos)
    results = []
    for f in fs:
        if f.valid is not None:
            valid = f.valid != 0
            if perm is not None:
                valid = valid[perm]
        else:
            valid = torch.ones(m, dtype=torch.bool, device=dev)
        cnt = torch.zeros(ng, dtype=torch.int64, device=dev)
        cnt.index_add_(0, seg, valid.to(torch.int64))
        has = cnt > 0
        if f.fn == "count":
            results.append((fit(cnt), None))
            continue
        v = f.values[perm] if perm is not None else f.values
        is_float = v.dtype.is_floating_point
        if f.fn in ("sum", "avg"):
            wide = torch.float64 if (is_float or f.fn == "avg") \
                else torch.int64
            x = torch.where(valid, v.to(wide), torch.zeros((), dtype=wide))
            res = torch.zeros(ng, dtype=wide, device=dev).index_add_(0, seg, x)
            if f.fn == "avg":
                res = res / cnt.clamp(min=1).to(torch.float64)
        elif is_float:
            x = v.to(torch.float64)
            nan = torch.isnan(x) & valid
            nnan = torch.zeros(ng, dtype=torch.int64, device=dev)
            nnan.index_add_(0, seg, nan.to(torch.int64))
            inf = float("inf") if f.fn == "min" else float("-inf")
            x = torch.where(valid & ~nan, x, torch.full_like(x, inf))
            res = torch.full((ng,), inf, dtype=torch.float64, device=dev)
            res.scatter_reduce_(0, seg, x, "amin" if f.fn == "min" else "amax")
            # NaN greatest: max takes any NaN, min only a segment of NaNs
            to_nan = nnan > 0 if f.fn == "max" else nnan == cnt
            res = torch.where(to_nan, torch.full_like(res, float("nan")), res)
        else:
            x = v.to(torch.int64)
            ii = torch.iinfo(torch.int64)
            fill = ii.max if f.fn == "min" else ii.min
            x = torch.where(valid, x, torch.full_like(x, fill))
            res = torch.full((ng,), fill, dtype=torch.int64, device=dev)
            res.scatter_reduce_(0, seg, x, "amin" if f.fn == "min" else "amax")
        res = torch.where(has, res, torch.zeros_like(res)).to(f.out_dtype())
        results.append((fit(res), fit(has) if f.nullable() else None))
    count = torch.full((1,), ng, dtype=torch.int64, device=dev)
    return first, results, count


# ---------------------------------------------------------------------------
# native path
# ---------------------------------------------------------------------------

def _reduce_gpu(head, perm, fs: List[_Func], k):
    g = _native.gpu()
    m = head.numel()
    dev = head.device
    stream = _native.current_stream()
    first = torch.empty(k, dtype=torch.int64, device=dev)
    count = torch.empty(1, dtype=torch.int64, device=dev)
    results = [_outputs(f, k, dev) for f in fs]
    # without output rows only the count is wanted
    todo = list(zip(fs, results)) if k > 0 else []
    for lo in range(0, max(len(todo), 1), SEG_MAX_FUNCS):
        chunk = todo[lo:lo + SEG_MAX_FUNCS]
        descs = [_descriptor(f, m, data, ov) for f, (data, ov) in chunk]
        work = _work_buffer(g.seg_reduce_work_bytes(m, len(chunk)), dev)
        g.seg_reduce(descs, perm.data_ptr() if perm is not None else 0,
                     head.data_ptr(), m, m, k, first.data_ptr() if k else 0,
                     count.data_ptr(),
                     work.data_ptr() if work is not None else 0, stream)
    return first, results, count


def segmented_reduce_tensors(head_flags: torch.Tensor, funcs: Sequence[Tuple],
                             perm: Optional[torch.Tensor] = None,
                             num_segments: Optional[int] = None):
    """Aggregates per segment of the sorted order `perm`.

    `head_flags[i]` is nonzero where sorted position i starts a segment
    (position 0 always does, whatever the flag says). Without `perm` the
    order is the identity: the rows are grouped already. `funcs` is a list of
    `(fn, values, valid)`: `values` and `valid` (a byte per row, zero = null)
    are indexed by original row; `values` is None for count(*).

    Returns `(first_rows, results, count)`. Segment g is the g-th in sorted
    order; `first_rows[g]` is `perm[position of its head]`, after a stable
    sort the smallest original row of the group. `results` holds one
    `(data, valid)` per function; `valid` is a bool tensor, or None for count
    and inputs without validity. `count` is an int64[1] tensor on the device
    of the input: the number of segments.

    `num_segments=None` gives outputs of one row per input row, the upper
    bound: no host sync, and rows at and beyond `count` are unspecified.
    `num_segments=k` gives outputs of k rows: the first k segments if there
    are more, and `count` still reports the total.
    """
    if not isinstance(head_flags, torch.Tensor) or \
            head_flags.dtype not in _BYTE_DTYPES:
        raise TypeError("head_flags must be a bool, uint8 or int8 tensor")
    if head_flags.dim() != 1:
        raise ValueError("head_flags must be 1-D, got shape "
                         f"{tuple(head_flags.shape)}")
    m = head_flags.numel()
    dev = head_flags.device
    if perm is not None:
        if not isinstance(perm, torch.Tensor) or perm.dtype != torch.int64:
            raise TypeError("perm must be an int64 tensor")
        if perm.dim() != 1 or perm.numel() != m:
            raise ValueError(f"perm must be 1-D with {m} rows")
        if perm.device != dev:
            raise ValueError("perm and head_flags are on different devices")
        perm = perm.contiguous()
    if num_segments is not None:
        if isinstance(num_segments, bool) or not isinstance(num_segments, int):
            raise TypeError("num_segments must be an int or None")
        if not 0 <= num_segments <= m:
            raise ValueError(f"num_segments = {num_segments} is outside "
                             f"0..{m}")
    fs = _check_funcs(list(funcs), m, dev)
    k = m if num_segments is None else num_segments
    if m == 0:
        return (torch.empty(0, dtype=torch.int64, device=dev),
                [_outputs(f, 0, dev) for f in fs],
                torch.zeros(1, dtype=torch.int64, device=dev))
    head = head_flags.contiguous()
    if dev.type == "cuda":
        return _reduce_gpu(head, perm, fs, k)
    head = head != 0
    head[0] = True
    return _reduce_cpu(head, perm, fs, k)


def groupby_tensors(keys: Sequence[torch.Tensor], aggs: Sequence[Tuple],
                    valids: Optional[Sequence] = None,
                    key_bits: Optional[Sequence] = None):
    """Sort-based group-by: `sort_order_tensors`, `key_change_flags`, a read
    of the group count (the op's one host sync) and
    `segmented_reduce_tensors` with the exact size.

    `keys`, `valids` and `key_bits` are those of `sort_order_tensors`; `aggs`
    is the `funcs` list of `segmented_reduce_tensors`. Returns
    `(first_rows, results, ngroups)`: gather the key columns by `first_rows`
    for the group keys.

    Contract: groups come out in ascending key order, nulls first. Key
    equality is the sort's: nulls equal each other, all NaNs are equal and
    -0.0 == 0.0. Within a group values combine in input row order. An empty
    key list is one global group (no sort, no sync); no rows give no groups.
    """
    from .sort import _check_keys, _key_change_keys, _sort_order_keys
    ks = _check_keys(keys, valids, None, None, key_bits)
    aggs = list(aggs)
    if ks:
        m, dev = ks[0].data.numel(), ks[0].data.device
    else:
        cols = [spec[1] for spec in aggs if len(spec) == 3
                and isinstance(spec[1], torch.Tensor)]
        if not cols:
            raise ValueError("groupby_tensors needs a key or a value column")
        m, dev = cols[0].numel(), cols[0].device
    if not ks or m == 0:
        head = torch.zeros(m, dtype=torch.bool, device=dev)
        ngroups = 1 if m else 0
        first, results, _count = segmented_reduce_tensors(
            head, aggs, None, num_segments=ngroups)
        return first, results, ngroups
    perm = _sort_order_keys(ks, m, dev)
    head = _key_change_keys(ks, perm, m)
    ngroups = int(head.sum().item())
    first, results, _count = segmented_reduce_tensors(
        head, aggs, perm, num_segments=ngroups)
    return first, results, ngroups
