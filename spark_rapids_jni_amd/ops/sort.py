"""Sort order and sort-merge join (Java API parity:
JoinPrimitives.sortMergeInnerJoin, join_primitives.hpp:64-72).

Sort order (cudf sorted_order / sort_by_key): `sort_order_tensors`,
`key_change_flags`, `sort_order` and `sort_by_key` give the stable,
multi-column, null-aware permutation on the packed-key radix sort of
src/gpu/sort_order.hip. Every key becomes a bit field whose unsigned order is
the wanted order; the fields are packed least-significant key first into
64-bit words and each word costs ceil(used_bits / 8) radix passes. Equality
is the same everywhere: nulls equal each other, all NaNs are equal (and sort
above +inf), -0.0 == 0.0. CPU tensors take an equivalent torch expression;
CUDA tensors always take the native kernels, with no host sync, so the ops
run under stream capture.

`sort_pairs_i64` is that sort with one ascending 64-bit signed key;
`sort_merge_inner_join` sorts the build keys with it and probes them with the
binary-search kernel of src/gpu/sort.hip.
"""
from typing import List, Optional, Sequence, Tuple

import torch

from .. import _native
from ..columnar import Column, DType, Table, validity_to_bool
from .compact import nonzero


def sort_pairs_i64(keys: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """Stable ascending sort; returns (sorted_keys, order) where
    sorted_keys[i] = keys[order[i]]."""
    n = keys.numel()
    if n == 0:
        return keys.clone(), torch.empty(0, dtype=torch.int64,
                                         device=keys.device)
    key = _Key(keys, None, _SK_SINT, 64, desc=False, nulls_first=False)
    order = _sort_order_keys([key], n, keys.device)
    return keys[order], order


def sort_merge_inner_join(build: Column, probe: Column):
    """reference join_primitives.hpp:64 sort_merge_inner_join: sort the build
    side, binary-search probes, emit gather maps."""
    g = _native.gpu()
    stream = _native.current_stream()
    assert build.dtype == DType.INT64 and probe.dtype == DType.INT64
    dev = build.device
    bkeys = build.data
    orig_rows = None
    if build.validity is not None:
        # null build keys never match: sort the valid rows only
        orig_rows = nonzero(validity_to_bool(build.validity, build.size))
        bkeys = build.data[orig_rows]
    sorted_k, order = sort_pairs_i64(bkeys)
    build_rows = order if orig_rows is None else orig_rows[order]
    n = probe.size
    counter = torch.zeros(1, dtype=torch.int64, device=dev)
    g.merge_join(sorted_k.data_ptr(), build_rows.data_ptr(), sorted_k.numel(),
                 probe.data.data_ptr(),
                 probe.validity.data_ptr() if probe.validity is not None else 0,
                 n, counter.data_ptr(), 0, 0, 0, 0, stream)
    total = int(counter.item())
    counter.zero_()
    out_build = torch.empty(max(total, 1), dtype=torch.int32, device=dev)
    out_probe = torch.empty(max(total, 1), dtype=torch.int64, device=dev)
    g.merge_join(sorted_k.data_ptr(), build_rows.data_ptr(), sorted_k.numel(),
                 probe.data.data_ptr(),
                 probe.validity.data_ptr() if probe.validity is not None else 0,
                 n, counter.data_ptr(), out_build.data_ptr(),
                 out_probe.data_ptr(), total, 1, stream)
    return out_build[:total], out_probe[:total]


# ---------------------------------------------------------------------------
# sort order
# ---------------------------------------------------------------------------

# field kinds and flags of src/gpu/sort_order.hpp
_SK_UINT, _SK_SINT, _SK_BOOL, _SK_F32, _SK_F64, _SK_NULL = range(6)
_SF_DESC, _SF_NULLS_FIRST, _SF_NULL_BIT = 1, 2, 4

_BYTE_DTYPES = (torch.bool, torch.uint8, torch.int8)
_KEY_KINDS = {
    torch.bool: _SK_BOOL, torch.uint8: _SK_UINT,
    torch.int8: _SK_SINT, torch.int16: _SK_SINT, torch.int32: _SK_SINT,
    torch.int64: _SK_SINT, torch.float32: _SK_F32, torch.float64: _SK_F64,
}


class _Key:
    """One sort key: a 1-D tensor (any stride), optional byte validity, the
    field kind and width, direction and null order. `null_bit=False` keeps
    the validity (null rows encode as zero) but emits no null field: the low
    half of a DECIMAL128 rides on the null field of the high half."""
    __slots__ = ("data", "valid", "kind", "bits", "desc", "nulls_first",
                 "null_bit")

    def __init__(self, data, valid, kind, bits, desc, nulls_first,
                 null_bit=True):
        self.data, self.valid, self.kind, self.bits = data, valid, kind, bits
        self.desc, self.nulls_first = desc, nulls_first
        self.null_bit = null_bit and valid is not None

    def flags(self, null_bit):
        return ((_SF_DESC if self.desc else 0)
                | (_SF_NULLS_FIRST if self.nulls_first else 0)
                | (_SF_NULL_BIT if null_bit else 0))

    def field(self, kind, shift, null_bit):
        """Descriptor tuple of bind_sort_order.cpp."""
        return (self.data.data_ptr(),
                self.valid.data_ptr() if self.valid is not None else 0,
                self.data.stride(0) if self.data.numel() > 1 else 1,
                kind, self.data.element_size(), self.bits, shift,
                self.flags(null_bit))


def _check_keys(keys, valids, ascending, nulls_first, key_bits) -> List[_Key]:
    keys = list(keys)
    nk = len(keys)

    def per_key(x, what, default):
        if x is None:
            return [default] * nk
        x = list(x)
        if len(x) != nk:
            raise ValueError(f"{what} has {len(x)} entries for {nk} keys")
        return x

    valids = per_key(valids, "valids", None)
    ascending = [bool(a) for a in per_key(ascending, "ascending", True)]
    nulls_first = [a if nf is None else bool(nf) for a, nf in
                   zip(ascending, per_key(nulls_first, "nulls_first", None))]
    key_bits = per_key(key_bits, "key_bits", None)
    out = []
    for i, t in enumerate(keys):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"keys[{i}] must be a torch.Tensor")
        if t.dtype not in _KEY_KINDS:
            raise TypeError(f"keys[{i}] has unsupported dtype {t.dtype}")
        if t.dim() != 1:
            raise ValueError(f"keys[{i}] must be 1-D, got shape "
                             f"{tuple(t.shape)}")
        if t.numel() != keys[0].numel():
            raise ValueError(f"keys[{i}] has {t.numel()} rows but keys[0] "
                             f"has {keys[0].numel()}")
        if t.device != keys[0].device:
            raise ValueError(f"keys[{i}] and keys[0] are on different devices")
        v = valids[i]
        if v is not None:
            if not isinstance(v, torch.Tensor) or v.dtype not in _BYTE_DTYPES:
                raise TypeError(f"valids[{i}] must be a bool, uint8 or int8 "
                                "tensor")
            if v.dim() != 1 or v.numel() != t.numel():
                raise ValueError(f"valids[{i}] must be 1-D with "
                                 f"{t.numel()} rows")
            if v.device != t.device:
                raise ValueError(f"valids[{i}] and keys[{i}] are on different "
                                 "devices")
            v = v.contiguous()
        kind = _KEY_KINDS[t.dtype]
        bits = 1 if kind == _SK_BOOL else 8 * t.element_size()
        b = key_bits[i]
        if b is not None:
            if t.dtype.is_floating_point:
                raise ValueError(f"key_bits given for float keys[{i}]")
            if not 1 <= int(b) <= 64:
                raise ValueError(f"key_bits[{i}] = {b} is outside 1..64")
            if kind != _SK_BOOL:
                # low b bits as unsigned; a hint wider than the dtype keeps
                # the dtype's own order
                if int(b) < bits:
                    kind, bits = _SK_UINT, int(b)
        out.append(_Key(t.contiguous(), v, kind, bits, not ascending[i],
                        nulls_first[i]))
    return out


def _cpu_code(k: _Key) -> torch.Tensor:
    """int64 codes whose signed order is the key's wanted order (null rows
    zero): the torch twin of encode_field in sort_order.hip."""
    d = k.data
    if k.kind == _SK_BOOL:
        c = (d != 0).to(torch.int64)
    elif k.kind in (_SK_F32, _SK_F64):
        d = torch.where(torch.isnan(d), torch.full_like(d, float("nan")), d)
        d = d + 0.0  # -0.0 -> +0.0
        iv = torch.int32 if k.kind == _SK_F32 else torch.int64
        b = d.contiguous().view(iv).to(torch.int64)
        c = torch.where(b < 0, b ^ torch.iinfo(torch.int64).max, b)
    elif k.kind == _SK_UINT:
        c = d.to(torch.int64)
        if k.bits < 64:
            c = c & ((1 << k.bits) - 1)
        elif d.dtype == torch.int64:  # full unsigned word (DECIMAL128 low)
            c = c ^ torch.iinfo(torch.int64).min
    else:
        c = d.to(torch.int64)
    if k.desc:
        c = ~c
    if k.valid is not None:
        c = torch.where(k.valid != 0, c, torch.zeros_like(c))
    return c


def _null_rank(k: _Key) -> torch.Tensor:
    valid = k.valid != 0
    return (valid if k.nulls_first else ~valid).to(torch.int8)


def _sort_order_cpu(ks: List[_Key], n: int, dev) -> torch.Tensor:
    perm = torch.arange(n, dtype=torch.int64, device=dev)
    for k in reversed(ks):
        perm = perm[torch.argsort(_cpu_code(k)[perm], stable=True)]
        if k.null_bit:  # nulls by a pass of their own, never a fill value
            perm = perm[torch.argsort(_null_rank(k)[perm], stable=True)]
    return perm


def _layout(ks: List[_Key]):
    """Fields least-significant key first into 64-bit words; a field that
    does not fit starts the next word."""
    words, cur, used = [], [], 0

    def put(k, kind, width, null_bit):
        nonlocal cur, used
        if used + width > 64:
            words.append(cur)
            cur, used = [], 0
        cur.append(k.field(kind, used, null_bit))
        used += width

    for k in reversed(ks):
        if k.null_bit and k.bits < 64:
            put(k, k.kind, k.bits + 1, True)
        else:
            put(k, k.kind, k.bits, False)
            if k.null_bit:  # a 64-bit value leaves its null field no room
                put(k, _SK_NULL, 1, False)
    words.append(cur)
    return words


def _sort_order_keys(ks: List[_Key], n: int, dev) -> torch.Tensor:
    if n == 0 or not ks:
        return torch.arange(n, dtype=torch.int64, device=dev)
    if dev.type != "cuda":
        return _sort_order_cpu(ks, n, dev)
    g = _native.gpu()
    out = torch.empty(n, dtype=torch.int64, device=dev)
    work = torch.empty(g.sort_order_work_words(n), dtype=torch.int64,
                       device=dev)
    g.sort_order(_layout(ks), n, work.data_ptr(), out.data_ptr(),
                 _native.current_stream())
    return out


def sort_order_tensors(keys: Sequence[torch.Tensor],
                       valids: Optional[Sequence] = None,
                       ascending: Optional[Sequence[bool]] = None,
                       nulls_first: Optional[Sequence] = None,
                       key_bits: Optional[Sequence] = None) -> torch.Tensor:
    """The stable permutation that sorts rows by `keys` (first key primary):
    rows equal under all keys keep input order.

    `valids[i]` is None or a byte-per-row tensor (zero = null). `ascending`
    defaults to all True; `nulls_first[i]` defaults to `ascending[i]` (the
    Spark default). Nulls order strictly before or after every valid value.
    `key_bits[i] = b` promises `0 <= keys[i] < 2**b` for an integer key
    (dictionary codes): only b bits are sorted; values outside the promise
    give an unspecified order.
    """
    ks = _check_keys(keys, valids, ascending, nulls_first, key_bits)
    if not ks:
        raise ValueError("sort_order_tensors needs at least one key")
    return _sort_order_keys(ks, ks[0].data.numel(), ks[0].data.device)


def _key_change_keys(ks: List[_Key], perm: torch.Tensor,
                     nrows: int) -> torch.Tensor:
    m = perm.numel()
    dev = perm.device
    if m == 0:
        return torch.empty(0, dtype=torch.bool, device=dev)
    if dev.type != "cuda":
        out = torch.zeros(m, dtype=torch.bool, device=dev)
        out[0] = True
        for k in ks:
            c = _cpu_code(k)[perm]
            out[1:] |= c[1:] != c[:-1]
            if k.null_bit:
                v = (k.valid != 0)[perm]
                out[1:] |= v[1:] != v[:-1]
        return out
    g = _native.gpu()
    out = torch.empty(m, dtype=torch.bool, device=dev)
    fields = []
    for k in ks:
        fits = k.null_bit and k.bits < 64
        fields.append(k.field(k.kind, 0, fits))
        if k.null_bit and not fits:
            fields.append(k.field(_SK_NULL, 0, False))
    g.key_change_flags(fields, perm.data_ptr(), m, nrows, out.data_ptr(),
                       _native.current_stream())
    return out


def key_change_flags(keys: Sequence[torch.Tensor], perm: torch.Tensor,
                     valids: Optional[Sequence] = None) -> torch.Tensor:
    """`out[i]` is True when `i == 0` or rows `perm[i]` and `perm[i-1]`
    differ in any key, under the sort's equality (nulls equal each other,
    all NaNs equal, -0.0 == 0.0). Precondition: `0 <= perm < len(keys[0])`.
    """
    ks = _check_keys(keys, valids, None, None, None)
    if not isinstance(perm, torch.Tensor) or perm.dtype != torch.int64:
        raise TypeError("perm must be an int64 tensor")
    if perm.dim() != 1:
        raise ValueError(f"perm must be 1-D, got shape {tuple(perm.shape)}")
    if not ks:
        raise ValueError("key_change_flags needs at least one key")
    if perm.device != ks[0].data.device:
        raise ValueError("perm and keys are on different devices")
    nrows = ks[0].data.numel()
    if nrows == 0 and perm.numel():
        raise ValueError("perm indexes empty keys")
    return _key_change_keys(ks, perm.contiguous(), nrows)


_COLUMN_KEYS = (DType.BOOL8, DType.INT8, DType.INT16, DType.INT32,
                DType.INT64, DType.FLOAT32, DType.FLOAT64, DType.DATE32,
                DType.TIMESTAMP_US, DType.DECIMAL32, DType.DECIMAL64)


def _table_keys(table: Table, ascending, nulls_first) -> List[_Key]:
    nc = table.num_columns
    asc = [True] * nc if ascending is None else [bool(a) for a in ascending]
    nf = [None] * nc if nulls_first is None else list(nulls_first)
    if len(asc) != nc or len(nf) != nc:
        raise ValueError(f"ascending/nulls_first must have {nc} entries")
    ks = []
    for i, c in enumerate(table.columns):
        first = asc[i] if nf[i] is None else bool(nf[i])
        valid = (validity_to_bool(c.validity, c.size)
                 if c.validity is not None else None)
        if c.dtype == DType.DECIMAL128:
            # little-endian pair: element 0 low (unsigned), element 1 high
            pair = c.data.view(c.size, 2)
            ks.append(_Key(pair[:, 1], valid, _SK_SINT, 64, not asc[i],
                           first))
            ks.append(_Key(pair[:, 0], valid, _SK_UINT, 64, not asc[i],
                           first, null_bit=False))
        elif c.dtype in _COLUMN_KEYS:
            kind = _SK_F32 if c.dtype == DType.FLOAT32 else \
                _SK_F64 if c.dtype == DType.FLOAT64 else _SK_SINT
            ks.append(_Key(c.data, valid, kind, 8 * c.data.element_size(),
                           not asc[i], first))
        else:
            raise NotImplementedError(
                f"sort_order: {c.dtype.name} keys are not supported")
    return ks


def sort_order(table: Table, ascending: Optional[Sequence[bool]] = None,
               nulls_first: Optional[Sequence] = None) -> torch.Tensor:
    """cudf sorted_order: the stable permutation that sorts `table`'s rows
    by its columns (first column primary). Fixed-width columns only."""
    ks = _table_keys(table, ascending, nulls_first)
    return _sort_order_keys(ks, table.num_rows, table.device)


def sort_by_key(values: Table, keys: Table,
                ascending: Optional[Sequence[bool]] = None,
                nulls_first: Optional[Sequence] = None) -> Table:
    """cudf sort_by_key: `values` reordered by the sort order of `keys`."""
    from .copying import gather
    if values.num_rows != keys.num_rows:
        raise ValueError(f"values has {values.num_rows} rows but keys has "
                         f"{keys.num_rows}")
    return gather(values, sort_order(keys, ascending, nulls_first))
