"""Composable join building blocks.

Java API parity: com.nvidia.spark.rapids.jni.JoinPrimitives
(reference join_primitives.hpp:64-237 / JoinPrimitives.java:80-302):
hash_inner_join producing gather maps, plus gather-map algebra
(make_left_outer / make_full_outer / semi / anti).

MI355X design: a multimap of packed (fingerprint32|row+1) u64 slots at 50%
load, linear probing (src/gpu/hashtable.hip). Build side is capped at 2^31-1
rows (the reference has the same per-column row cap); probe side is int64.

Which to prefer. Semi, anti, left and full outer joins are first-class probes
of a HashJoinTable: `semi_select` / `probe_matches`, `left_outer_join` and
`full_outer_join`. On the fast-path tables they are emit modes of the one
probe kernel (src/gpu/join_probe.hpp); on the generic table they fall back to
the compositions below. `semi_join` and the gather-map algebra
`make_left_outer` / `make_full_outer` over `inner_join` remain, unchanged,
for callers that hold an inner-join result already or need the generic
kernels.
"""
from typing import List, Optional, Sequence, Tuple, Union

import torch

from .. import _native
from ..columnar import Column, Table, pack_descriptors


def _keys(x) -> List[Column]:
    if isinstance(x, Table):
        return x.columns
    if isinstance(x, Column):
        return [x]
    return list(x)


def _next_pow2(n: int) -> int:
    p = 1
    while p < n:
        p <<= 1
    return p


_FAST_KEY_DTYPES = None


def _is_i64_fast(cols: List[Column]) -> bool:
    """Single integer-typed key -> the specialized fast-path tables: the
    narrow one reads 4-byte-or-less columns in place (real NDS surrogate
    keys are INT32); the wide one upcasts them to int64 once, where sign
    extension preserves equality."""
    global _FAST_KEY_DTYPES
    from ..columnar import DType
    if _FAST_KEY_DTYPES is None:
        _FAST_KEY_DTYPES = {DType.INT64, DType.INT32, DType.INT16, DType.INT8,
                            DType.DATE32, DType.TIMESTAMP_US}
    return len(cols) == 1 and cols[0].dtype in _FAST_KEY_DTYPES


def _as_i64_keys(c: Column) -> Column:
    """int64 view/upcast of an integer key column (validity shared)."""
    if c.data.dtype == torch.int64:
        return c
    return Column(c.dtype, c.size, c.data.to(torch.int64), c.validity,
                  null_count=None)


# int64 / timestamp keys are range-scanned for the narrow table only from this
# build size on: from here the wide table, next_pow2(4n) x 16 B, no longer
# fits the 256 MiB Infinity Cache, and below it the scan's host read-back is
# not worth paying in host-bound plans.
NARROW_SCAN_MIN_ROWS = 1 << 22
# slots per build row before rounding up to a power of two (25% max load)
NARROW_SLOTS_PER_ROW = 4
_I32_KMIN = -(1 << 31)
# a key range of at most this many slots per build row takes the direct-
# address table: at most 8 B per build row, a quarter of the narrow table
DENSE_MAX_SLOTS_PER_ROW = 2
# `mode` of the join_probe_mode_* entry points: ProbeEmit in join_probe.hpp
# (its INNER = 0 is what join_probe_i64 / _n32 / _d32 run)
PROBE_OUTER, PROBE_FLAG = 1, 2


def _is_dense(lo: int, hi: int, n: int) -> bool:
    """True when the key range [lo, hi] of n build rows is small enough for
    one direct-address slot per key of the range."""
    return hi - lo + 1 <= max(DENSE_MAX_SLOTS_PER_ROW * n, 64)


def _fits_narrow(lo: int, hi: int) -> bool:
    """True when every key of [lo, hi] has a 32-bit offset from lo."""
    return hi - lo < (1 << 32)


def _key_range(data: torch.Tensor) -> Tuple[int, int]:
    """(min, max) of a key tensor as Python ints: one pass, one read-back.
    Only the forced dense build still scans with torch: its native calls are
    exactly one build and the probes (tests/test_join_dense.py pins them)."""
    lo, hi = torch.aminmax(data)
    lo, hi = torch.stack([lo, hi]).cpu().tolist()
    return int(lo), int(hi)


def _scan_keys(data: torch.Tensor, key_i32: int,
               valid: Optional[torch.Tensor], n: int) -> Tuple[int, int, bool]:
    """(min, max, ordered) of the first n >= 1 keys of an int32 / int64
    tensor: one pass of join_scan_keys (src/gpu/join_fast.hip), one read-back.
    `ordered`: row i holds key min + i for every i and, where a mask is
    given, no row is null. The kernel's flag says key[i] - key[0] == i in
    unsigned arithmetic; max - min == n - 1 rejects the one sequence that
    passes it without being ascending, one that wraps past INT64_MAX."""
    out = torch.empty(3, dtype=torch.int64, device=data.device)
    _native.gpu().join_scan_keys(
        data.data_ptr(), key_i32, valid.data_ptr() if valid is not None else 0,
        n, out.data_ptr(), _native.current_stream())
    lo, hi, flag = out.cpu().tolist()
    return lo, hi, bool(flag) and hi - lo == n - 1


def _narrow_keys(c: Column) -> Tuple[torch.Tensor, int]:
    """(key tensor the narrow kernels read in place, key_i32 flag): 4-byte
    columns as they are, 1- and 2-byte ones widened to int32."""
    d = c.data
    if d.dtype == torch.int64:
        return d, 0
    if d.dtype != torch.int32:
        d = d.to(torch.int32)
    return d, 1


def _int_packable(cols: List[Column]) -> bool:
    from ..columnar import DType
    return (len(cols) > 1 and all(
        c.data is not None
        and c.data.dtype in (torch.int64, torch.int32, torch.int16,
                             torch.int8)
        and c.dtype not in (DType.FLOAT64, DType.FLOAT32) for c in cols))


def _pack_ranges(cols: List[Column]):
    """(mins, widths) for folding an int-key tuple into one int64, or None
    if the range product overflows."""
    if cols[0].size == 0:
        return None  # nothing to scan; generic path handles empties
    pairs = [torch.aminmax(c.data) for c in cols]
    flat = torch.stack([t for lo_hi in pairs for t in lo_hi]).cpu().tolist()
    mins, widths = [], []
    total = 1
    for k in range(len(cols)):  # ONE device sync for all columns
        lo, hi = int(flat[2 * k]), int(flat[2 * k + 1])
        span = hi - lo + 1
        if span <= 0:
            return None
        mins.append(lo)
        widths.append(span)
        total *= span
        if total >= 2**62:
            return None
    return mins, widths


def _pack_keys(cols: List[Column], mins, widths, drop_all_valid=True):
    """Fold key columns into (packed int64, validity bitmask|None) using the
    given ranges. Rows with a null key or an out-of-range value (probe side
    of a join: can never match) get their validity bit cleared — join
    semantics, where nulls never match. An all-valid mask is dropped, which
    costs one read-back; drop_all_valid=False keeps the mask whatever it
    holds and reads nothing back."""
    from ..columnar import validity_to_bool
    n = cols[0].size
    dev = cols[0].device
    packed = torch.zeros(n, dtype=torch.int64, device=dev)
    ok = torch.ones(n, dtype=torch.bool, device=dev)
    for c, lo, w in zip(cols, mins, widths):
        v = c.data.to(torch.int64) - lo
        in_range = (v >= 0) & (v < w)
        if c.validity is not None:
            in_range &= validity_to_bool(c.validity, n)
        ok &= in_range
        packed = packed * w + torch.where(in_range, v, torch.zeros_like(v))
    if drop_all_valid and bool(ok.all().item()):
        return packed, None
    from ..ops.aggregate import _validity_from_bool
    return packed, _validity_from_bool(ok)


class HashJoinTable:
    """Build-side hash table reusable across probes (reference: the build/probe
    split of hash_inner_join).

    Five layouts (`layout`): "generic", a (fingerprint32|row+1) single-word
    table for any key schema; "wide", the specialized 16-byte {key,row} table
    for single integer keys that need 64 bits; "narrow", one 8-byte word
    (key - kmin | row+1 | chain) per slot for keys whose range fits 32 bits —
    INT32/DATE32 columns, packed tuples, int64 surrogate keys; "dense",
    a direct-address table of one 4-byte word (row+1) per key of
    [kmin, kmin + capacity) with no hashing at all, for a single integer key
    column that is duplicate-free and whose range is at most
    DENSE_MAX_SLOTS_PER_ROW slots per row; and "ordered", no table at all
    (`slots` is None), for a single integer key column without nulls whose
    row i holds key kmin + i: a dimension table written in surrogate-key
    order, or a contiguous range of one. The word the dense table would hold
    for a key is then key - kmin + 1, and the probe computes it. Wide,
    narrow, dense and ordered are the software-pipelined fast path
    (`i64_fast`), see src/gpu/join_fast.hip and its one probe kernel,
    src/gpu/join_probe.hpp. `capacity` is the slot count in every layout; it
    is a power of two except for dense, where it is the key range, and
    ordered, where it is the build row count.

    Probes: `inner_join`, `left_outer_join`, `full_outer_join` give gather
    maps; `semi_select` gives the ascending probe rows of a semi or anti
    join, `probe_matches` their per-probe-row flags and `mark_matches` the
    per-build-row ones. All of them run on every layout and probe the table
    that was built. `semi_join` is the older form of `semi_select`: on a
    fast-path table it builds and probes a second, generic table and its row
    order is unspecified; prefer `semi_select`.
    """

    def __init__(self, build_keys: List[Column], slots: torch.Tensor,
                 capacity: int, keep, i64_fast: bool,
                 layout: Optional[str] = None, kmin: int = 0):
        self.build_keys = build_keys
        self.slots = slots
        self.capacity = capacity
        self._keep = keep
        self.i64_fast = i64_fast
        self.layout = layout or ("wide" if i64_fast else "generic")
        self.kmin = kmin
        self.num_build_rows = build_keys[0].size

    @staticmethod
    def build(keys: Union[Column, Table, Sequence[Column]],
              force_generic: bool = False,
              narrow: Optional[bool] = None,
              dense: Optional[bool] = None,
              ordered: Optional[bool] = None) -> "HashJoinTable":
        """narrow: True forces the 8-byte-slot table (raises if the key range
        does not fit 32 bits), False forbids it (wide), None decides:
        4-byte-or-less key columns and packed tuples of width product <= 2^32
        always, int64 columns from NARROW_SCAN_MIN_ROWS rows when a min/max
        scan fits. Neither True nor False ever gives the dense table.

        dense: True forces the direct-address table for a single integer key
        column of any width and row count (scans the range; raises if it is
        not dense or a key repeats), False forbids it. None applies only where
        narrow is None and an int64 column is range-scanned anyway: a dense
        range builds the direct table and reads back its duplicate flag (one
        more read-back; the probe cannot start before the build ends); if a
        key repeats the table is dropped and the narrow build goes ahead with
        the range already known. dense=True gives "dense" whatever the key
        order.

        ordered: True forces the table-free layout for a single integer key
        column of any width and row count, zero included (scans the keys;
        raises if a row is null or row i does not hold key[0] + i, or if
        another layout is forced with it), False forbids it. None applies
        where dense=None does: the scan that finds the range of an int64
        column finds the order in the same pass, and an ordered column
        returns right after the scan's read-back, with no slots, no zero
        fill, no build kernel and no second read-back. The scan runs again
        on every build; nothing is cached between calls."""
        cols = _keys(keys)
        n = cols[0].size
        assert n < 2**31, "build side capped at 2^31-1 rows (chunk the build)"
        g = _native.gpu()
        dev = cols[0].device
        stream = _native.current_stream()
        # int64 fast path runs at 25% max load: random-probe scans touch
        # ~1.3 slots instead of ~2.5 at 50% load (measured faster than
        # double-slot prefetching); generic path stays at 50%.
        capacity = max(_next_pow2(n * 2), 64)

        def build_narrow(data, key_i32, valid, kmin, keep, pack=None):
            cap = max(_next_pow2(n * NARROW_SLOTS_PER_ROW), 64)
            slots = torch.zeros(cap, dtype=torch.int64, device=dev)
            g.join_build_n32(data.data_ptr(), key_i32,
                             valid.data_ptr() if valid is not None else 0,
                             n, slots.data_ptr(), cap, kmin, stream)
            tbl = HashJoinTable(cols, slots, cap, keep, True, "narrow", kmin)
            if pack is not None:
                tbl._pack = pack
            return tbl

        def build_dense(data, key_i32, valid, lo, hi):
            """The direct-address table over [lo, hi], or None when a build
            key repeats (the table cannot hold it)."""
            span = hi - lo + 1
            slots = torch.zeros(span, dtype=torch.int32, device=dev)
            flag = torch.zeros(1, dtype=torch.int32, device=dev)
            g.join_build_d32(data.data_ptr(), key_i32,
                             valid.data_ptr() if valid is not None else 0,
                             n, slots.data_ptr(), span, lo, flag.data_ptr(),
                             stream)
            bad = int(flag.item())
            assert not bad & 2, "build key outside its scanned range"
            if bad:
                return None
            return HashJoinTable(cols, slots, span, None, True, "dense", lo)

        def ordered_table(lo):
            return HashJoinTable(cols, None, n, None, True, "ordered", lo)

        if ordered:
            if (force_generic or narrow is not None or dense
                    or not _is_i64_fast(cols)):
                raise ValueError("ordered=True needs a single integer key "
                                 "column and no other layout forced")
            if n == 0:
                return ordered_table(0)
            data, key_i32 = _narrow_keys(cols[0])
            lo, hi, is_ord = _scan_keys(data, key_i32, cols[0].validity, n)
            if not is_ord:
                raise ValueError("ordered=True: a build row is null or row i "
                                 "does not hold key[0] + i")
            return ordered_table(lo)

        if dense:
            if force_generic or narrow is not None or not _is_i64_fast(cols):
                raise ValueError("dense=True needs a single integer key "
                                 "column and no other layout forced")
            data, key_i32 = _narrow_keys(cols[0])
            lo, hi = _key_range(data) if n else (0, 0)
            if not _is_dense(lo, hi, n):
                raise ValueError(f"dense=True: key range [{lo}, {hi}] is not "
                                 f"dense for {n} rows")
            tbl = build_dense(data, key_i32, cols[0].validity, lo, hi)
            if tbl is None:
                raise ValueError("dense=True: duplicate build key")
            return tbl

        pack = None
        if not force_generic and _int_packable(cols):
            pack = _pack_ranges(cols)
        if pack is not None:
            packed, pvalid = _pack_keys(cols, *pack)
            total = 1
            for w in pack[1]:
                total *= w
            fits = total <= (1 << 32)
            if narrow and not fits:
                raise ValueError("narrow=True: packed key range needs more "
                                 "than 32 bits")
            if fits and narrow is not False:
                return build_narrow(packed, 0, pvalid, 0, (packed, pvalid),
                                    pack)
            capacity = max(_next_pow2(n * 4), 64)
            slots = torch.zeros(capacity * 2, dtype=torch.int64, device=dev)
            g.join_build_i64(packed.data_ptr(),
                             pvalid.data_ptr() if pvalid is not None else 0,
                             n, slots.data_ptr(), capacity, stream)
            tbl = HashJoinTable(cols, slots, capacity, (packed, pvalid), True)
            tbl._pack = pack
            return tbl
        if _is_i64_fast(cols) and not force_generic:
            c0 = cols[0]
            if narrow is not False:
                if c0.data.dtype != torch.int64:
                    # range known from the type: no scan, no sync
                    data, key_i32 = _narrow_keys(c0)
                    return build_narrow(data, key_i32, c0.validity, _I32_KMIN,
                                        data)
                if narrow or n >= NARROW_SCAN_MIN_ROWS:
                    auto = narrow is None and dense is None
                    try_ord = auto and ordered is None
                    lo, hi, is_ord = (
                        _scan_keys(c0.data, 0,
                                   c0.validity if try_ord else None, n)
                        if n else (0, 0, False))
                    if try_ord and is_ord:
                        return ordered_table(lo)
                    if auto and _is_dense(lo, hi, n):
                        tbl = build_dense(c0.data, 0, c0.validity, lo, hi)
                        if tbl is not None:
                            return tbl
                    if _fits_narrow(lo, hi):
                        return build_narrow(c0.data, 0, c0.validity, lo, None)
                    if narrow:
                        raise ValueError(
                            f"narrow=True: key range [{lo}, {hi}] needs more "
                            "than 32 bits")
            capacity = max(_next_pow2(n * 4), 64)
            c = _as_i64_keys(c0)
            slots = torch.zeros(capacity * 2, dtype=torch.int64, device=dev)
            g.join_build_i64(c.data.data_ptr(),
                             c.validity.data_ptr() if c.validity is not None else 0,
                             n, slots.data_ptr(), capacity, stream)
            return HashJoinTable(cols, slots, capacity, None, True)
        if narrow:
            raise ValueError("narrow=True needs integer keys on the fast path")
        slots = torch.zeros(capacity, dtype=torch.int64, device=dev)
        desc, top, keep = pack_descriptors(cols)
        g.join_build(desc.data_ptr(), top.data_ptr(), len(cols), n,
                     slots.data_ptr(), capacity, _native.current_stream())
        return HashJoinTable(cols, slots, capacity, (desc, top, keep), False)

    def _descs(self, probe_cols):
        bdesc, btop, bkeep = pack_descriptors(self.build_keys)
        pdesc, ptop, pkeep = pack_descriptors(probe_cols)
        return bdesc, btop, pdesc, ptop, (bkeep, pkeep, bdesc, btop, pdesc, ptop)

    def _fast_probe_col(self, pcols: List[Column],
                        sync: bool = True) -> Optional[Column]:
        """The single key column the fast-path probe kernels read, or None
        when this probe has to take the generic kernels. `sync=False` packs
        a multi-key probe without the read-back that drops an all-valid
        mask (see _pack_keys)."""
        pack = getattr(self, "_pack", None)
        if not self.i64_fast:
            return None
        if pack is not None:
            if len(pcols) != len(self.build_keys):
                return None
            packed, pvalid = _pack_keys(pcols, *pack, drop_all_valid=sync)
            return Column(pcols[0].dtype, pcols[0].size, packed, pvalid,
                          null_count=None)
        if not _is_i64_fast(pcols):
            return None
        if self.layout in ("narrow", "dense", "ordered"):
            return pcols[0]  # read in place, whatever its integer width
        return _as_i64_keys(pcols[0])

    def _probe_fast(self, p: Column, counter, out_build, out_probe,
                    out_capacity, matched, fill, stream):
        g = _native.gpu()
        pvalid = p.validity.data_ptr() if p.validity is not None else 0
        if self.layout == "ordered":
            data, key_i32 = _narrow_keys(p)
            g.join_probe_ord(data.data_ptr(), key_i32, pvalid, p.size,
                             self.capacity, self.kmin, counter.data_ptr(),
                             out_build, out_probe, out_capacity, matched,
                             fill, stream)
        elif self.layout == "dense":
            data, key_i32 = _narrow_keys(p)
            g.join_probe_d32(data.data_ptr(), key_i32, pvalid, p.size,
                             self.slots.data_ptr(), self.capacity, self.kmin,
                             counter.data_ptr(), out_build, out_probe,
                             out_capacity, matched, fill, stream)
        elif self.layout == "narrow":
            data, key_i32 = _narrow_keys(p)
            g.join_probe_n32(data.data_ptr(), key_i32, pvalid, p.size,
                             self.slots.data_ptr(), self.capacity, self.kmin,
                             counter.data_ptr(), out_build, out_probe,
                             out_capacity, matched, fill, 0, stream)
        else:
            g.join_probe_i64(p.data.data_ptr(), pvalid, p.size,
                             self.slots.data_ptr(), self.capacity,
                             counter.data_ptr(), out_build, out_probe,
                             out_capacity, matched, fill, 0, stream)

    def _probe_mode(self, p: Column, mode: int, counter, out_build, out_probe,
                    out_capacity, matched, fill, probe_hit, anti, stream):
        """One probe in an emit mode of join_probe.hpp (PROBE_*)."""
        g = _native.gpu()
        pvalid = p.validity.data_ptr() if p.validity is not None else 0
        if self.layout == "wide":
            g.join_probe_mode_i64(p.data.data_ptr(), pvalid, p.size,
                                  self.slots.data_ptr(), self.capacity,
                                  counter, out_build, out_probe, out_capacity,
                                  matched, fill, mode, probe_hit, anti, stream)
            return
        data, key_i32 = _narrow_keys(p)
        if self.layout == "ordered":
            g.join_probe_mode_ord(data.data_ptr(), key_i32, pvalid, p.size,
                                  self.capacity, self.kmin, counter,
                                  out_build, out_probe, out_capacity, matched,
                                  fill, mode, probe_hit, anti, stream)
            return
        fn = (g.join_probe_mode_d32 if self.layout == "dense"
              else g.join_probe_mode_n32)
        fn(data.data_ptr(), key_i32, pvalid, p.size, self.slots.data_ptr(),
           self.capacity, self.kmin, counter, out_build, out_probe,
           out_capacity, matched, fill, mode, probe_hit, anti, stream)

    def probe_matches(self, probe, anti: bool = False) -> torch.Tensor:
        """Per-PROBE-row flags (uint8): 1 where the row has a match, or, with
        `anti`, where it has none. The mirror of `mark_matches`. A null key
        never matches, so `anti` flags it. No pair is materialized and nothing
        is counted: on the fast-path tables this is one pass of the probe
        kernel in its flag mode, with no atomic and no read-back. The result
        is the [:nprobe] view of a buffer padded to 16 bytes."""
        pcols = _keys(probe)
        # a packed probe keeps its validity mask unchecked: no read-back
        p = self._fast_probe_col(pcols, sync=False)
        if p is None:
            flags = torch.zeros(pcols[0].size, dtype=torch.uint8,
                                device=pcols[0].device)
            flags[self.semi_join(pcols, anti)] = 1
            return flags
        return self._probe_flags(p, anti)

    def _probe_flags(self, p: Column, anti: bool) -> torch.Tensor:
        """`probe_matches` over an already resolved fast-path key column."""
        nprobe = p.size
        buf = torch.empty((nprobe + 15) // 16 * 16, dtype=torch.uint8,
                          device=p.data.device)
        if nprobe:
            self._probe_mode(p, PROBE_FLAG, 0, 0, 0, 0, 0,
                             0, buf.data_ptr(), 1 if anti else 0,
                             _native.current_stream())
        return buf[:nprobe]

    def semi_select(self, probe, anti: bool = False) -> torch.Tensor:
        """Left semi/anti join: the probe rows with a match (without one for
        `anti`), int64, in ASCENDING order: the flags of `probe_matches` and
        one stable compaction, whose kept-row count is the one read-back, on
        packed multi-key tables too. Prefer this to `semi_join`, which builds
        a second, generic table over a fast-path table's keys and returns the
        rows in no fixed order."""
        from .compact import nonzero
        pcols = _keys(probe)
        p = self._fast_probe_col(pcols, sync=False)
        if p is None:
            return torch.sort(self.semi_join(pcols, anti))[0]
        return nonzero(self._probe_flags(p, anti))

    def left_outer_join(self, probe, out_hint: Optional[int] = None,
                        track_build_matches: bool = False):
        """LEFT OUTER join with the probe side as left. Returns (build_idx
        int32, probe_idx int64[, build_matched uint8]): every matching pair,
        and one pair with build index -1 for every probe row without a match
        (null keys included). Count, `out_hint` and the rerun on a hint that
        is too small work as in `inner_join`; the size is matching pairs plus
        unmatched probe rows. Pair order is unspecified. On the fast-path
        tables the probe kernel emits the -1 pairs itself; prefer this to
        `make_left_outer(inner_join(...))`."""
        pcols = _keys(probe)
        nprobe = pcols[0].size
        dev = pcols[0].device
        p = self._fast_probe_col(pcols)
        if p is None:
            res = self.inner_join(pcols, out_hint, track_build_matches)
            lb, lp = make_left_outer(nprobe, res[0], res[1])
            return (lb.to(torch.int32), lp) + tuple(res[2:])
        stream = _native.current_stream()

        def launch(counter, out_build, out_probe, capacity, matched, fill):
            self._probe_mode(p, PROBE_OUTER, counter.data_ptr(), out_build,
                             out_probe, capacity, matched, fill, 0, 0, stream)
        return self._gather_maps(launch, dev, out_hint, track_build_matches)

    def _gather_maps(self, launch, dev, out_hint: Optional[int],
                     track_build_matches: bool):
        """The count / hint / rerun protocol of every probe that returns
        gather maps. `launch(counter, out_build, out_probe, capacity,
        matched, fill)` runs one probe: fill = 0 counts only (null outputs),
        fill = 1 writes up to `capacity` pairs and counts them all. Without
        a hint a count pass sizes the outputs; a hint that proves too small
        costs a second fill pass with the exact size."""
        counter = torch.zeros(1, dtype=torch.int64, device=dev)
        if out_hint is None:
            launch(counter, 0, 0, 0, 0, 0)
            total = int(counter.item())
            counter.zero_()
        else:
            total = out_hint
        out_build = torch.empty(max(total, 1), dtype=torch.int32, device=dev)
        out_probe = torch.empty(max(total, 1), dtype=torch.int64, device=dev)
        matched = (torch.zeros(self.num_build_rows, dtype=torch.uint8,
                               device=dev)
                   if track_build_matches else None)
        launch(counter, out_build.data_ptr(), out_probe.data_ptr(), total,
               matched.data_ptr() if matched is not None else 0, 1)
        actual = int(counter.item())
        if actual > total:
            # hint was too small: rerun with the exact size
            return self._gather_maps(launch, dev, actual,
                                     track_build_matches)
        out_build = out_build[:actual]
        out_probe = out_probe[:actual]
        if track_build_matches:
            return out_build, out_probe, matched
        return out_build, out_probe

    def full_outer_join(self, probe, out_hint: Optional[int] = None):
        """FULL OUTER join. Returns (build_idx int64, probe_idx int64) with
        -1 on either side: the `left_outer_join` pairs (`out_hint` is theirs),
        then the build rows nothing matched, ascending, with probe index
        -1."""
        lb, lp, matched = self.left_outer_join(probe, out_hint,
                                               track_build_matches=True)
        return append_unmatched_build(matched, lb, lp)

    def inner_join(self, probe: Union[Column, Table, Sequence[Column]],
                   out_hint: Optional[int] = None,
                   track_build_matches: bool = False):
        """Returns (build_idx int32, probe_idx int64[, build_matched uint8])."""
        pcols = _keys(probe)
        nprobe = pcols[0].size
        g = _native.gpu()
        stream = _native.current_stream()
        dev = pcols[0].device
        p = self._fast_probe_col(pcols)
        fast = p is not None
        if not fast:
            bdesc, btop, pdesc, ptop, keep = self._descs(pcols)
        # Where the probe's time goes is the random fetch of a table word per
        # row: ~25 ms per 1B-row chunk against the dense table, the rate of
        # 64 B requests past an XCD's L2 (~3.2 TB/s, the same from the
        # Infinity Cache as from HBM). The "ordered" layout has no such fetch
        # and streams (docs/PERF.md, "ordered"). For every layout that has a
        # table, measured and rejected, twice: grouping the probe rows by
        # table window before the probe. By hash prefix into a 64 GiB hashed table
        # (part_hist/part_scatter + idxmap probe) each 64 B line is touched
        # only ~1.4x per 1B chunk and the scatter cost 29 ms per chunk
        # (profiles/r01_bench_join_22.1B.json). By key range into the 3.7 GiB
        # dense table, with a 5 ms histogram + scatter, the probe over the
        # grouped rows still took 20 ms per chunk against 25.5 direct: windows
        # of 32 - 128 MiB hit the Infinity Cache, not the 4 MiB L2s, and random
        # 64 B lines come from either at the same ~3 TB/s (docs/PERF.md,
        # "workgroup append"). The probe stays direct; part_hist/part_scatter
        # and the idxmap probe stay exposed for schema-partitioned shuffle use.
        def launch(counter, out_build, out_probe, capacity, matched, fill):
            if fast:
                self._probe_fast(p, counter, out_build, out_probe, capacity,
                                 matched, fill, stream)
            elif not fill:
                g.join_probe_count(bdesc.data_ptr(), btop.data_ptr(), pdesc.data_ptr(),
                                   ptop.data_ptr(), len(pcols), nprobe,
                                   self.slots.data_ptr(), self.capacity,
                                   counter.data_ptr(), stream)
            else:
                g.join_probe_fill(bdesc.data_ptr(), btop.data_ptr(), pdesc.data_ptr(),
                                  ptop.data_ptr(), len(pcols), nprobe,
                                  self.slots.data_ptr(), self.capacity, counter.data_ptr(),
                                  out_build, out_probe, capacity, matched, stream)
        return self._gather_maps(launch, dev, out_hint, track_build_matches)

    def mark_matches(self, probe) -> torch.Tensor:
        """Stream the probe rows and return per-BUILD-row matched flags
        (uint8) without materializing join pairs. This is the right-semi
        building block: to semi/anti-filter a small table against a huge
        one, build on the small side and mark while probing the huge side
        (reference get_matched_rows, join_primitives.hpp:237)."""
        pcols = _keys(probe)
        nprobe = pcols[0].size
        g = _native.gpu()
        stream = _native.current_stream()
        dev = pcols[0].device
        matched = torch.zeros(self.num_build_rows, dtype=torch.uint8,
                              device=dev)
        counter = torch.zeros(1, dtype=torch.int64, device=dev)
        p = self._fast_probe_col(pcols)
        if p is not None:
            self._probe_fast(p, counter, 0, 0, 0, matched.data_ptr(), 1,
                             stream)
        else:
            bdesc, btop, pdesc, ptop, keep = self._descs(pcols)
            g.join_probe_fill(bdesc.data_ptr(), btop.data_ptr(),
                              pdesc.data_ptr(), ptop.data_ptr(),
                              len(pcols), nprobe, self.slots.data_ptr(),
                              self.capacity, counter.data_ptr(), 0, 0, 0,
                              matched.data_ptr(), stream)
        return matched

    def semi_join(self, probe, anti: bool = False) -> torch.Tensor:
        """Left semi/anti join: probe-side row indices with (no) match."""
        if self.i64_fast:
            # semi/anti runs on the generic slot layout
            if not hasattr(self, "_generic"):
                g = _native.gpu()
                n = self.num_build_rows
                # the generic table's own size (50% max load), not
                # self.capacity: a dense table's is no power of two
                capacity = max(_next_pow2(2 * n), 64)
                slots = torch.zeros(capacity, dtype=torch.int64,
                                    device=self.build_keys[0].device)
                desc, top, keep = pack_descriptors(self.build_keys)
                # hash over ALL key columns — a single-column hash here
                # silently misses every multi-key match (r2 fix)
                g.join_build(desc.data_ptr(), top.data_ptr(),
                             len(self.build_keys), n,
                             slots.data_ptr(), capacity,
                             _native.current_stream())
                self._generic = HashJoinTable(self.build_keys, slots,
                                              capacity, (desc, top, keep),
                                              False)
            return self._generic.semi_join(probe, anti)
        pcols = _keys(probe)
        nprobe = pcols[0].size
        g = _native.gpu()
        stream = _native.current_stream()
        dev = pcols[0].device
        bdesc, btop, pdesc, ptop, keep = self._descs(pcols)
        counter = torch.zeros(1, dtype=torch.int64, device=dev)
        out = torch.empty(nprobe, dtype=torch.int64, device=dev)
        g.join_semi(bdesc.data_ptr(), btop.data_ptr(), pdesc.data_ptr(),
                    ptop.data_ptr(), len(pcols), nprobe, self.slots.data_ptr(),
                    self.capacity, counter.data_ptr(), out.data_ptr(), nprobe,
                    1 if anti else 0, stream)
        return out[:int(counter.item())]


def hash_inner_join(build, probe) -> Tuple[torch.Tensor, torch.Tensor]:
    """reference join_primitives.hpp:87 hash_inner_join"""
    return HashJoinTable.build(build).inner_join(probe)


def make_left_outer(probe_size: int, build_idx: torch.Tensor,
                    probe_idx: torch.Tensor):
    """Extend an inner-join gather map pair to LEFT OUTER (probe side = left):
    unmatched probe rows appear with build index -1 (null gather).
    reference join_primitives.hpp:130 make_left_outer."""
    dev = probe_idx.device
    matched = torch.zeros(probe_size, dtype=torch.bool, device=dev)
    matched[probe_idx] = True
    unmatched = torch.nonzero(~matched, as_tuple=False).view(-1)
    lo_build = torch.cat([build_idx.long(),
                          torch.full((unmatched.numel(),), -1, dtype=torch.int64,
                                     device=dev)])
    lo_probe = torch.cat([probe_idx, unmatched])
    return lo_build, lo_probe


def append_unmatched_build(build_matched: torch.Tensor,
                           build_idx: torch.Tensor, probe_idx: torch.Tensor):
    """Left-outer pairs to FULL OUTER: the build rows whose `build_matched`
    flag is 0 follow the pairs, ascending, with probe index -1. Both results
    are int64."""
    from .compact import nonzero
    unmatched_b = nonzero(build_matched == 0)
    fo_build = torch.cat([build_idx.long(), unmatched_b])
    fo_probe = torch.cat([probe_idx,
                          torch.full((unmatched_b.numel(),), -1,
                                     dtype=torch.int64,
                                     device=probe_idx.device)])
    return fo_build, fo_probe


def make_full_outer(build_matched: torch.Tensor, build_idx: torch.Tensor,
                    probe_idx: torch.Tensor, probe_size: int):
    """FULL OUTER: left-outer plus unmatched build rows with probe index -1.
    reference join_primitives.hpp:150 make_full_outer."""
    lo_build, lo_probe = make_left_outer(probe_size, build_idx, probe_idx)
    unmatched_b = torch.nonzero(build_matched == 0, as_tuple=False).view(-1)
    fo_build = torch.cat([lo_build, unmatched_b])
    fo_probe = torch.cat([lo_probe,
                          torch.full((unmatched_b.numel(),), -1,
                                     dtype=torch.int64, device=lo_probe.device)])
    return fo_build, fo_probe
