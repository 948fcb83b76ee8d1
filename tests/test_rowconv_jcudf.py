"""JCUDF row format: an independent layout oracle and byte-exact device tests.

The row format is a wire contract with the JVM side, so nothing here trusts
`row_layout`: the rule is restated below from the contract
(RowConversion.java's class comment and the reference's column-information
pass) and the expected bytes are built on the host by a numpy packer.

The rule:
  * a fixed-width column is aligned to its own size (DECIMAL128 to 16);
  * a string column is an 8-byte (offset-in-row, length) int32 pair aligned
    to 4;
  * validity is one bit per column, bit c % 8 of byte c / 8, set = valid,
    directly after the last column, no padding in front of it;
  * a fixed-width row is padded to 8 bytes;
  * a variable-width row puts the chars, in column order, at the UNPADDED end
    of the validity bytes and takes round_up(that + string bytes, 8) bytes;
  * padding and the slots of null columns are zero.

Where the contract is silent (the slot of a null string) the packer writes
what the kernels write: the current char position and length 0.

Inputs are random full-range bit patterns (floats through integer views, so
NaN payloads and -0.0 travel; everything is compared as bytes), with random
garbage under nulls and a mix of no-mask / all-null / all-valid / random
masks in one table.
"""
import struct

import numpy as np
import pytest
import torch

from spark_rapids_jni_amd import _native
from spark_rapids_jni_amd.columnar import (Column, DType, TORCH_DTYPE, Table,
                                           validity_nbytes)
from spark_rapids_jni_amd.ops import row_conversion as rc

S = DType.STRING
# sizes written out here on purpose: the oracle shares no table with the code
SIZE = {DType.BOOL8: 1, DType.INT8: 1, DType.INT16: 2, DType.INT32: 4,
        DType.INT64: 8, DType.FLOAT32: 4, DType.FLOAT64: 8, DType.DATE32: 4,
        DType.TIMESTAMP_US: 8, DType.DECIMAL32: 4, DType.DECIMAL64: 8,
        DType.DECIMAL128: 16}
FIXED = list(SIZE)
assert len(FIXED) == 12

# all 12 dtypes, ordered so that padding is needed in front of a 2-, a 4-,
# an 8- and a 16-byte column
MIXED = [DType.INT8, DType.INT16, DType.BOOL8, DType.INT32, DType.INT64,
         DType.DECIMAL128, DType.DECIMAL32, DType.FLOAT32, DType.FLOAT64,
         DType.DATE32, DType.TIMESTAMP_US, DType.DECIMAL64]
MIXED_OFFS = [0, 2, 4, 8, 16, 32, 48, 52, 56, 64, 72, 80]


def _up(x, a):
    return (x + a - 1) // a * a


def oracle_layout(dtypes):
    """(column offsets, validity offset, unpadded end of the validity)."""
    off = 0
    offs = []
    for dt in dtypes:
        size, align = (8, 4) if dt == S else (SIZE[dt], SIZE[dt])
        off = _up(off, align)
        offs.append(off)
        off += size
    return offs, off, off + (len(dtypes) + 7) // 8


def cycle(k, start=0):
    return [FIXED[(start + i) % 12] for i in range(k)]


# ---------------------------------------------------------------------------
# CPU: row_layout / var_row_layout against the oracle
# ---------------------------------------------------------------------------

def _check_layout(dtypes):
    offs, voff, end = oracle_layout(dtypes)
    assert rc.var_row_layout(dtypes) == (offs, voff, end), dtypes
    if S not in dtypes:
        assert rc.row_layout(dtypes) == (offs, voff, _up(end, 8)), dtypes


def test_layout_every_dtype_alone_and_every_ordered_pair():
    for a in FIXED:
        _check_layout([a])
        # alone: offset 0, one validity byte right behind, row padded to 8
        assert rc.row_layout([a]) == ([0], SIZE[a], _up(SIZE[a] + 1, 8))
        for b in FIXED:
            _check_layout([a, b])
            assert rc.row_layout([a, b])[0] == [0, _up(SIZE[a], SIZE[b])]


def test_layout_contract_examples():
    # the two examples of RowConversion.java's class comment (its 32-bit
    # column is a duration; any 4-byte type has the same layout)
    ex1 = [DType.BOOL8, DType.INT16, DType.INT32]
    assert oracle_layout(ex1) == ([0, 2, 4], 8, 9)
    assert rc.row_layout(ex1) == ([0, 2, 4], 8, 16)
    ex2 = [DType.INT32, DType.INT16, DType.BOOL8]
    assert oracle_layout(ex2) == ([0, 4, 6], 7, 8)
    assert rc.row_layout(ex2) == ([0, 4, 6], 7, 8)
    # a 16-byte column is aligned to 16, not 8
    assert rc.row_layout([DType.INT32, DType.DECIMAL128]) == ([0, 16], 32, 40)
    assert rc.var_row_layout([DType.INT32, DType.DECIMAL128, S]) == \
        ([0, 16, 32], 40, 41)
    # chars start at the unpadded validity end
    assert rc.var_row_layout([DType.INT32, S]) == ([0, 4], 12, 13)
    assert rc.var_row_layout([DType.INT64, S, DType.INT8]) == \
        ([0, 8, 16], 17, 18)
    assert oracle_layout(MIXED) == (MIXED_OFFS, 88, 90)
    assert rc.row_layout(MIXED) == (MIXED_OFFS, 88, 96)


@pytest.mark.parametrize("k", [1, 7, 8, 9, 16, 17, 65])
def test_layout_column_counts(k):
    for start in range(12):
        dtypes = cycle(k, start)
        _check_layout(dtypes)
        offs, voff, rs = rc.row_layout(dtypes)
        # ceil(k/8) validity bytes, then only padding up to the next 8
        assert rs == _up(voff + (k + 7) // 8, 8)
    _check_layout([DType.INT8] * k)
    _check_layout([DType.DECIMAL128] * k)


def test_layout_strings_first_middle_last():
    for a in FIXED:
        for b in FIXED:
            for dtypes in ([S, a, b], [a, S, b], [a, b, S], [S, a, S, b, S],
                           [S], [S, S]):
                _check_layout(dtypes)
    _check_layout(cycle(9) + [S] + cycle(7, 3) + [S])


# k x INT64: (row size, from-rows tile height, to-rows tiled) on each side of
# every dispatch boundary
WIDE = {30: (248, 256, True), 31: (256, 128, True), 62: (504, 128, True),
        63: (512, 64, True), 125: (1016, 64, True), 126: (1024, 0, False)}


def lds_pitch(row_size):
    return row_size if (row_size >> 2) & 1 else row_size + 4


def from_rows_tile(row_size):
    """Tile height the from-rows dispatch picks: the largest of 256/128/64
    rows whose pitched tile fits 64 KB of LDS, else 0 (one thread per row)."""
    for tr in (256, 128, 64):
        if tr * lds_pitch(row_size) <= 64 * 1024:
            return tr
    return 0


def to_rows_tiled(row_size):
    return 64 * lds_pitch(row_size) <= 64 * 1024


@pytest.mark.parametrize("k", sorted(WIDE))
def test_wide_row_sizes_sit_on_the_dispatch_boundaries(k):
    rs, tile, tiled = WIDE[k]
    assert rc.row_layout([DType.INT64] * k)[2] == rs
    assert from_rows_tile(rs) == tile
    assert to_rows_tiled(rs) == tiled


# ---------------------------------------------------------------------------
# host data and the byte packers
# ---------------------------------------------------------------------------
NULL_MODES = ["mask", "none", "all_null", "all_valid"]


def gen_valid(rng, n, mode):
    if mode == "none":
        return None
    if mode == "all_null":
        return np.zeros(n, dtype=bool)
    if mode == "all_valid":
        return np.ones(n, dtype=bool)
    return rng.random(n) < 0.7


def gen_fixed(rng, dtypes, n):
    """Per column: (n, size) random bytes (garbage under nulls included) and
    a bool mask or None."""
    raws = [rng.integers(0, 256, size=(n, SIZE[dt]), dtype=np.uint8)
            for dt in dtypes]
    valids = [gen_valid(rng, n, NULL_MODES[i % 4]) for i in range(len(dtypes))]
    return raws, valids


def mask_bytes(valid):
    out = np.zeros(validity_nbytes(len(valid)), dtype=np.uint8)
    bits = np.packbits(valid, bitorder="little")
    out[:len(bits)] = bits
    return out


def mask_tensor(valid, dev="cuda"):
    return None if valid is None else torch.from_numpy(mask_bytes(valid)).to(dev)


def fixed_column(dt, raw, valid, dev="cuda"):
    if raw.shape[0] == 0:  # torch cannot reinterpret an empty tensor's dtype
        data = torch.empty(0, dtype=TORCH_DTYPE[dt])
    else:
        data = torch.from_numpy(raw.reshape(-1).copy()).view(TORCH_DTYPE[dt])
    return Column(dt, raw.shape[0], data.to(dev), mask_tensor(valid, dev),
                  null_count=None)


def string_column(strs, valid, dev="cuda"):
    offs = np.zeros(len(strs) + 1, dtype=np.int32)
    np.cumsum([len(s) for s in strs], out=offs[1:])
    chars = np.frombuffer(b"".join(strs), dtype=np.uint8).copy()
    return Column(S, len(strs), torch.from_numpy(chars).to(dev),
                  mask_tensor(valid, dev),
                  offsets=torch.from_numpy(offs).to(dev), null_count=None)


def valid_matrix(valids, n):
    return np.stack([np.ones(n, dtype=bool) if v is None else v
                     for v in valids])


def validity_byte(vm, j):
    b = np.zeros(vm.shape[1], dtype=np.uint8)
    for c in range(8 * j, min(8 * j + 8, vm.shape[0])):
        b |= vm[c].astype(np.uint8) << (c % 8)
    return b


def pack_fixed(dtypes, raws, valids):
    """Expected fixed-width row buffer as a flat uint8 array."""
    offs, voff, end = oracle_layout(dtypes)
    rs = _up(end, 8)
    n = raws[0].shape[0]
    nvb = (len(dtypes) + 7) // 8
    buf = np.zeros(n * rs, dtype=np.uint8)
    if n == 0:
        return buf
    row = np.dtype({
        "names": [f"c{i}" for i in range(len(dtypes))] +
                 [f"v{j}" for j in range(nvb)],
        "formats": [(np.uint8, (SIZE[dt],)) for dt in dtypes] +
                   [np.uint8] * nvb,
        "offsets": offs + [voff + j for j in range(nvb)],
        "itemsize": rs})
    rows = buf.view(row)
    vm = valid_matrix(valids, n)
    for i in range(len(dtypes)):
        rows[f"c{i}"] = np.where(vm[i][:, None], raws[i], 0)
    for j in range(nvb):
        rows[f"v{j}"] = validity_byte(vm, j)
    return buf


def pack_var(dtypes, cols, valids):
    """Expected variable-width buffer and row offsets, one row at a time.
    cols[i] is an (n, size) byte array, or a list of bytes for a string."""
    offs, voff, end = oracle_layout(dtypes)
    n = len(cols[0])
    vm = valid_matrix(valids, n)
    out = bytearray()
    row_offsets = [0]
    for r in range(n):
        nbytes = sum(len(cols[i][r]) for i, dt in enumerate(dtypes)
                     if dt == S and vm[i][r])
        row = bytearray(_up(end + nbytes, 8))
        pos = end
        for i, dt in enumerate(dtypes):
            if dt == S:
                s = cols[i][r] if vm[i][r] else b""
                struct.pack_into("<ii", row, offs[i], pos, len(s))
                row[pos:pos + len(s)] = s
                pos += len(s)
            elif vm[i][r]:
                row[offs[i]:offs[i] + SIZE[dt]] = cols[i][r].tobytes()
            if vm[i][r]:
                row[voff + i // 8] |= 1 << (i % 8)
        out += row
        row_offsets.append(len(out))
    return (np.frombuffer(bytes(out), dtype=np.uint8),
            np.array(row_offsets, dtype=np.int32))


def same_bytes(got, want, what):
    got = np.asarray(got).reshape(-1)
    want = np.asarray(want).reshape(-1)
    assert got.shape == want.shape, f"{what}: {got.shape} vs {want.shape}"
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got != want)
        pytest.fail(f"{what}: {bad.size} bytes differ, first at {bad[0]}: "
                    f"got {got[bad[0]]:#x}, want {want[bad[0]]:#x}")


def host_bytes(t, nbytes=None):
    h = t.detach().cpu().contiguous().view(torch.uint8).numpy().reshape(-1)
    return h if nbytes is None else h[:nbytes]


def unpack_mask(mask_u8, n):
    return np.unpackbits(np.asarray(mask_u8), bitorder="little")[:n] \
        .astype(bool)


def check_fixed_column(col, dt, raw, valid, what):
    n = raw.shape[0]
    assert col.dtype == dt and col.size == n, what
    want_v = np.ones(n, dtype=bool) if valid is None else valid
    assert col.validity is not None, what
    got_v = unpack_mask(host_bytes(col.validity), n)
    same_bytes(got_v, want_v, f"{what} validity")
    got = host_bytes(col.data, n * SIZE[dt]).reshape(n, SIZE[dt])
    same_bytes(got[want_v], raw[want_v], f"{what} data")


def check_fixed_table(table, dtypes, raws, valids, what):
    assert len(table.columns) == len(dtypes)
    for i, dt in enumerate(dtypes):
        check_fixed_column(table.columns[i], dt, raws[i], valids[i],
                           f"{what} col {i} {dt.name}")


def roundtrip_fixed(dtypes, n, rng, what):
    """to-rows equals the packer, from-rows equals the input. Returns the
    batches and the host data."""
    raws, valids = gen_fixed(rng, dtypes, n)
    table = Table([fixed_column(dt, r, v)
                   for dt, r, v in zip(dtypes, raws, valids)])
    want = pack_fixed(dtypes, raws, valids)
    batches = rc.convert_to_rows(table)
    rs = _up(oracle_layout(dtypes)[2], 8)
    for buf, m in batches:
        assert buf.numel() == m * rs, what
    got = np.concatenate([host_bytes(buf) for buf, _ in batches])
    same_bytes(got, want, f"{what} to-rows")
    assert sum(m for _, m in batches) == n
    back = rc.convert_from_rows(batches, dtypes)
    check_fixed_table(back, dtypes, raws, valids, f"{what} from-rows")
    return batches, raws, valids


# ---------------------------------------------------------------------------
# device: fixed width
# ---------------------------------------------------------------------------
NARROW = {"mixed12": MIXED, "v1": cycle(1, 3), "v7": cycle(7), "v8": cycle(8),
          "v9": cycle(9, 2), "v16": cycle(16), "v17": cycle(17, 5)}
# 300: the last 256-row tile has 44 rows, so three of its four 64-row
# validity sub-tiles lie past the end
NARROW_N = [0, 1, 63, 64, 65, 255, 256, 257, 300, 1000]


@pytest.fixture
def no_tile_override(monkeypatch):
    monkeypatch.delenv("SRJ_FROM_ROWS_TILE", raising=False)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(NARROW))
def test_fixed_narrow_schemas(name, no_tile_override):
    dtypes = NARROW[name]
    rs = _up(oracle_layout(dtypes)[2], 8)
    assert from_rows_tile(rs) == 256 and to_rows_tiled(rs)
    rng = np.random.default_rng(1000 + len(dtypes))
    for n in NARROW_N:
        roundtrip_fixed(dtypes, n, rng, f"{name} n={n}")


@pytest.mark.gpu
@pytest.mark.parametrize("k", sorted(WIDE))
def test_fixed_wide_rows_each_kernel(k, no_tile_override):
    """k x INT64 rows on both sides of every dispatch boundary: from-rows
    tiles of 256/128/64 rows and untiled, to-rows tiled and untiled."""
    dtypes = [DType.INT64] * k
    rs, tile, tiled = WIDE[k]
    assert rc.row_layout(dtypes)[2] == rs
    assert from_rows_tile(rs) == tile and to_rows_tiled(rs) == tiled
    rng = np.random.default_rng(2000 + k)
    for n in (65, 300):
        roundtrip_fixed(dtypes, n, rng, f"{k} x INT64 n={n}")


@pytest.mark.gpu
@pytest.mark.parametrize("n", [2048 * 64 + 65, 2048 * 256 + 300],
                         ids=["to_rows_lap", "from_rows_lap"])
def test_fixed_grid_stride_second_lap(n, no_tile_override):
    """8-byte rows, more tiles than the 2048-block grid: 64-row to-rows tiles
    and 256-row from-rows tiles both start a second lap."""
    dtypes = [DType.INT8]
    assert rc.row_layout(dtypes) == ([0], 1, 8)
    assert from_rows_tile(8) == 256 and to_rows_tiled(8)
    roundtrip_fixed(dtypes, n, np.random.default_rng(n), f"INT8 n={n}")


def same_table_bytes(a, b, what):
    for i, (x, y) in enumerate(zip(a.columns, b.columns)):
        same_bytes(host_bytes(x.data), host_bytes(y.data), f"{what} data {i}")
        same_bytes(host_bytes(x.validity), host_bytes(y.validity),
                   f"{what} validity {i}")


@pytest.mark.gpu
def test_from_rows_tile_override(monkeypatch):
    """SRJ_FROM_ROWS_TILE picks the tile height per call; a value that fits
    no tile, or a tile that does not fit LDS, takes the untiled kernel."""
    rng = np.random.default_rng(31)
    n = 300
    raws, valids = gen_fixed(rng, MIXED, n)
    rows = torch.from_numpy(pack_fixed(MIXED, raws, valids)).cuda()
    assert all(tr * lds_pitch(96) <= 64 * 1024 for tr in (256, 128, 64))
    first = None
    for tile in ("256", "128", "64", "1"):
        monkeypatch.setenv("SRJ_FROM_ROWS_TILE", tile)
        back = rc.convert_from_rows([(rows, n)], MIXED)
        check_fixed_table(back, MIXED, raws, valids, f"tile {tile}")
        if first is None:
            first = back
        same_table_bytes(first, back, f"tile {tile} vs 256")
    # 512-byte rows: a 256-row tile needs 129 KB, so the request falls through
    wide = [DType.INT64] * 63
    assert rc.row_layout(wide)[2] == 512
    assert 256 * lds_pitch(512) > 64 * 1024
    raws, valids = gen_fixed(rng, wide, n)
    rows = torch.from_numpy(pack_fixed(wide, raws, valids)).cuda()
    monkeypatch.setenv("SRJ_FROM_ROWS_TILE", "256")
    back = rc.convert_from_rows([(rows, n)], wide)
    check_fixed_table(back, wide, raws, valids, "tile 256 on 512-byte rows")


@pytest.mark.gpu
@pytest.mark.parametrize("rows_per_batch,counts",
                         [(64, [64] * 7 + [52]), (192, [192, 192, 116])])
def test_batching_seams(monkeypatch, no_tile_override, rows_per_batch, counts):
    rs = rc.row_layout(MIXED)[2]
    assert rs == 96
    monkeypatch.setattr(rc, "MAX_BATCH_BYTES", rows_per_batch * rs + rs - 1)
    batches, _, _ = roundtrip_fixed(MIXED, 500, np.random.default_rng(77),
                                    f"batches of {rows_per_batch}")
    assert [m for _, m in batches] == counts


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["mixed12", "v9", "v17"])
def test_from_rows_of_hand_made_rows(name, no_tile_override):
    """Rows as another writer may produce them: random bytes in the padding,
    in the slots of null columns and in the unused validity bits. Validity
    follows the column bits alone and valid data is exact."""
    dtypes = NARROW[name]
    rng = np.random.default_rng(len(dtypes))
    n = 300
    raws, valids = gen_fixed(rng, dtypes, n)
    offs, voff, end = oracle_layout(dtypes)
    rs = _up(end, 8)
    rows = pack_fixed(dtypes, raws, valids).reshape(n, rs).copy()
    noise = rng.integers(0, 256, size=(n, rs), dtype=np.uint8)
    free = np.ones((n, rs), dtype=bool)
    vm = valid_matrix(valids, n)
    for i, dt in enumerate(dtypes):
        free[:, offs[i]:offs[i] + SIZE[dt]] = ~vm[i][:, None]
    free[:, voff:end] = False
    rows[free] = noise[free]
    spare = len(dtypes) % 8
    if spare:
        rows[:, end - 1] |= noise[:, end - 1] & np.uint8(0xFF << spare & 0xFF)
    assert free[:, end:].all()
    back = rc.convert_from_rows([(torch.from_numpy(rows.reshape(-1)).cuda(),
                                  n)], dtypes)
    check_fixed_table(back, dtypes, raws, valids, name)


# ---------------------------------------------------------------------------
# device: variable width
# ---------------------------------------------------------------------------
WORDS = [b"", b"a", b"abc", "héllo".encode(), "日本語".encode(),
         "\U0001f600x".encode(), b"0123456789abcdef!", b"xy" * 20]

VAR_SCHEMAS = {
    "int32_str": [DType.INT32, S],
    "str_dec128": [S, DType.DECIMAL128, DType.INT32, S],
    "ten_cols": [DType.INT8, S, DType.INT64, DType.INT16, S, DType.DECIMAL128,
                 DType.FLOAT32, DType.BOOL8, S, DType.DATE32],
    "four_strings": [S, S, DType.INT16, S, S],
}


def gen_var(rng, dtypes, n):
    """String columns take turns: random mask, no mask, all empty, all null;
    fixed columns as in gen_fixed."""
    cols, valids = [], []
    ns = 0
    for i, dt in enumerate(dtypes):
        if dt == S:
            mode = ["mask", "none", "all_valid", "all_null"][ns % 4]
            pick = rng.integers(0, len(WORDS), size=n)
            empty = ns % 4 == 2
            cols.append([b"" if empty else WORDS[p] for p in pick])
            valids.append(gen_valid(rng, n, mode))
            ns += 1
        else:
            cols.append(rng.integers(0, 256, size=(n, SIZE[dt]),
                                     dtype=np.uint8))
            valids.append(gen_valid(rng, n, NULL_MODES[i % 4]))
    return cols, valids


def null_strings_empty(dtypes, cols, valids):
    """Arrow-style string columns: a null string spans no chars."""
    return [[s if valids[i] is None or valids[i][r] else b""
             for r, s in enumerate(c)] if dt == S else c
            for i, (dt, c) in enumerate(zip(dtypes, cols))]


def var_table(dtypes, cols, valids):
    return Table([string_column(c, v) if dt == S else fixed_column(dt, c, v)
                  for dt, c, v in zip(dtypes, cols, valids)])


def check_var_table(table, dtypes, cols, valids, what):
    n = len(cols[0])
    for i, dt in enumerate(dtypes):
        col = table.columns[i]
        w = f"{what} col {i} {dt.name}"
        if dt != S:
            check_fixed_column(col, dt, cols[i], valids[i], w)
            continue
        assert col.dtype == S and col.size == n
        want_v = np.ones(n, dtype=bool) if valids[i] is None else valids[i]
        same_bytes(unpack_mask(host_bytes(col.validity), n), want_v,
                   f"{w} validity")
        strs = [s if v else b"" for s, v in zip(cols[i], want_v)]
        want_offs = np.zeros(n + 1, dtype=np.int32)
        np.cumsum([len(s) for s in strs], out=want_offs[1:])
        assert col.offsets.dtype == torch.int32
        assert np.array_equal(col.offsets.cpu().numpy(), want_offs), w
        same_bytes(host_bytes(col.data, int(want_offs[-1])),
                   np.frombuffer(b"".join(strs), dtype=np.uint8),
                   f"{w} chars")


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(VAR_SCHEMAS))
def test_var_width_schemas(name):
    dtypes = VAR_SCHEMAS[name]
    rng = np.random.default_rng(len(name))
    for n in (1, 63, 65, 777):
        what = f"{name} n={n}"
        cols, valids = gen_var(rng, dtypes, n)
        cols = null_strings_empty(dtypes, cols, valids)
        want, want_offs = pack_var(dtypes, cols, valids)
        buf, row_offs = rc.convert_to_rows_varwidth(
            var_table(dtypes, cols, valids))
        assert row_offs.dtype == torch.int32
        assert np.array_equal(row_offs.cpu().numpy(), want_offs), what
        same_bytes(host_bytes(buf), want, f"{what} to-rows")
        back = rc.convert_from_rows_varwidth(buf, row_offs, dtypes)
        check_var_table(back, dtypes, cols, valids, f"{what} from-rows")


@pytest.mark.gpu
def test_var_width_grid_stride_second_lap():
    """[INT8, STRING] with 0-3 byte strings: every row is 16 bytes, chars at
    13, and 2048 * 256 + 65 rows send each thread round its loop again."""
    dtypes = [DType.INT8, S]
    assert oracle_layout(dtypes) == ([0, 4], 12, 13)
    n = 2048 * 256 + 65
    rng = np.random.default_rng(5)
    raw = rng.integers(0, 256, size=(n, 1), dtype=np.uint8)
    v0 = rng.random(n) < 0.7
    v1 = rng.random(n) < 0.8
    lens = np.where(v1, rng.integers(0, 4, size=n), 0).astype(np.int32)
    offs = np.zeros(n + 1, dtype=np.int32)
    np.cumsum(lens, out=offs[1:])
    chars = rng.integers(1, 256, size=int(offs[-1]), dtype=np.uint8)
    want = np.zeros((n, 16), dtype=np.uint8)
    want[:, 0] = np.where(v0, raw[:, 0], 0)
    want[:, 4:8] = np.full(n, 13, dtype="<i4").view(np.uint8).reshape(n, 4)
    want[:, 8:12] = lens.astype("<i4").view(np.uint8).reshape(n, 4)
    want[:, 12] = v0.astype(np.uint8) | (v1.astype(np.uint8) << 1)
    for k in range(3):
        has = lens > k
        want[has, 13 + k] = chars[offs[:-1][has] + k]
    scol = Column(S, n, torch.from_numpy(chars).cuda(), mask_tensor(v1),
                  offsets=torch.from_numpy(offs).cuda(), null_count=None)
    table = Table([fixed_column(DType.INT8, raw, v0), scol])
    buf, row_offs = rc.convert_to_rows_varwidth(table)
    assert np.array_equal(row_offs.cpu().numpy(),
                          np.arange(n + 1, dtype=np.int32) * 16)
    same_bytes(host_bytes(buf), want, "to-rows")
    back = rc.convert_from_rows_varwidth(buf, row_offs, dtypes)
    check_fixed_column(back.columns[0], DType.INT8, raw, v0, "INT8")
    got = back.columns[1]
    same_bytes(unpack_mask(host_bytes(got.validity), n), v1, "str validity")
    assert np.array_equal(got.offsets.cpu().numpy(), offs)
    same_bytes(host_bytes(got.data, int(offs[-1])), chars, "chars")


# ---------------------------------------------------------------------------
# device: guard bands round every output of the raw kernels
# ---------------------------------------------------------------------------
GUARD = 64
DESC_FMT = "<QQii"  # RowColDesc: data, valid, width, row_off


class Guarded:
    """nbytes of device memory in the middle of a tensor of 0xA5, with 64
    guard bytes on each side; the region starts 8-byte (in fact 64-byte)
    aligned and the guard behind it starts at its very first byte past."""

    def __init__(self, nbytes, fill=None):
        self.nbytes = nbytes
        self.big = torch.full((GUARD + _up(nbytes, 8) + GUARD,), 0xA5,
                              dtype=torch.uint8, device="cuda")
        self.mid = self.big[GUARD:GUARD + nbytes]
        assert self.mid.data_ptr() % 64 == 0
        if fill is not None:
            self.mid.fill_(fill)

    @property
    def ptr(self):
        return self.mid.data_ptr()

    def host(self):
        return self.mid.cpu().numpy()

    def check(self, what):
        h = self.big.cpu().numpy()
        lo = np.flatnonzero(h[:GUARD] != 0xA5)
        hi = np.flatnonzero(h[GUARD + self.nbytes:] != 0xA5)
        assert lo.size == 0, f"{what}: wrote {GUARD - lo[0]} bytes in front"
        assert hi.size == 0, \
            f"{what}: wrote up to {hi[-1] + 1} bytes past the end"


def dev_i64(vals):
    return torch.tensor(vals, dtype=torch.int64).cuda()


def pack_descs(entries):
    raw = b"".join(struct.pack(DESC_FMT, *e) for e in entries)
    return torch.frombuffer(bytearray(raw), dtype=torch.uint8).cuda()


GUARD_SCHEMAS = {256: MIXED, 128: [DType.INT64] * 31}


@pytest.mark.gpu
@pytest.mark.parametrize("n", [300, 100])
@pytest.mark.parametrize("tile", [256, 128])
def test_guard_bands_from_rows(tile, n, no_tile_override):
    """Column data and validity are written inside their buffers only. The
    whole 64-bit validity word that holds the tail is in bounds; the first
    byte after validity_nbytes(n) is not. At n = 300 the last 256-row tile
    holds 44 rows and the last 128-row tile 44 too, so each has sub-tiles
    that start past the end."""
    dtypes = GUARD_SCHEMAS[tile]
    offs, voff, end = oracle_layout(dtypes)
    rs = _up(end, 8)
    assert from_rows_tile(rs) == tile
    rng = np.random.default_rng(tile + n)
    raws, valids = gen_fixed(rng, dtypes, n)
    rows = torch.from_numpy(pack_fixed(dtypes, raws, valids)).cuda()
    data = [Guarded(n * SIZE[dt]) for dt in dtypes]
    masks = [Guarded(validity_nbytes(n)) for _ in dtypes]
    desc = pack_descs([(d.ptr, m.ptr, SIZE[dt], o)
                       for d, m, dt, o in zip(data, masks, dtypes, offs)])
    _native.gpu().from_rows(desc.data_ptr(), len(dtypes), n, rs, voff,
                            rows.data_ptr(), _native.current_stream())
    for i, dt in enumerate(dtypes):
        what = f"col {i} {dt.name}"
        data[i].check(f"{what} data")
        masks[i].check(f"{what} validity")
        v = valid_matrix(valids, n)[i]
        same_bytes(unpack_mask(masks[i].host(), n), v, f"{what} validity")
        same_bytes(data[i].host().reshape(n, SIZE[dt])[v], raws[i][v],
                   f"{what} data")


@pytest.mark.gpu
@pytest.mark.parametrize("n", [300, 100])
@pytest.mark.parametrize("tile", [256, 128])
def test_guard_bands_to_rows(tile, n):
    dtypes = GUARD_SCHEMAS[tile]
    offs, voff, end = oracle_layout(dtypes)
    rs = _up(end, 8)
    assert to_rows_tiled(rs)
    rng = np.random.default_rng(tile + n + 1)
    raws, valids = gen_fixed(rng, dtypes, n)
    cols = [fixed_column(dt, r, v) for dt, r, v in zip(dtypes, raws, valids)]
    desc = pack_descs([(c.data.data_ptr(),
                        0 if c.validity is None else c.validity.data_ptr(),
                        SIZE[dt], o)
                       for c, dt, o in zip(cols, dtypes, offs)])
    out = Guarded(n * rs, fill=0)  # callers hand the kernel a zeroed buffer
    _native.gpu().to_rows(desc.data_ptr(), len(dtypes), n, rs, voff, out.ptr,
                          _native.current_stream())
    out.check("row buffer")
    same_bytes(out.host(), pack_fixed(dtypes, raws, valids), "rows")


GUARD_VAR = [DType.INT8, S, DType.DECIMAL128, S]


@pytest.mark.gpu
@pytest.mark.parametrize("n", [300, 100])
def test_guard_bands_to_rows_var(n):
    dtypes = GUARD_VAR
    offs, voff, end = oracle_layout(dtypes)
    rng = np.random.default_rng(n)
    cols, valids = gen_var(rng, dtypes, n)
    cols = null_strings_empty(dtypes, cols, valids)
    want, want_offs = pack_var(dtypes, cols, valids)
    tcols = var_table(dtypes, cols, valids).columns
    desc = pack_descs([
        (c.offsets.data_ptr() if dt == S else c.data.data_ptr(),
         0 if c.validity is None else c.validity.data_ptr(),
         0 if dt == S else SIZE[dt], o)
        for c, dt, o in zip(tcols, dtypes, offs)])
    cptr = dev_i64([c.data.data_ptr() if dt == S else 0
                    for c, dt in zip(tcols, dtypes)])
    g = _native.gpu()
    stream = _native.current_stream()
    sizes = Guarded(n * 4)
    g.var_row_sizes(desc.data_ptr(), len(dtypes), n, end, sizes.ptr, stream)
    sizes.check("row sizes")
    got_sizes = sizes.host().view(np.int32)
    assert np.array_equal(got_sizes, np.diff(want_offs))
    row_offs = torch.from_numpy(want_offs).cuda()
    out = Guarded(int(want_offs[-1]), fill=0)
    g.to_rows_var(desc.data_ptr(), cptr.data_ptr(), len(dtypes), n, end, voff,
                  row_offs.data_ptr(), out.ptr, stream)
    out.check("row buffer")
    same_bytes(out.host(), want, "rows")


@pytest.mark.gpu
@pytest.mark.parametrize("n", [300, 100])
def test_guard_bands_from_rows_var(n):
    dtypes = GUARD_VAR
    offs, voff, end = oracle_layout(dtypes)
    rng = np.random.default_rng(n + 1)
    cols, valids = gen_var(rng, dtypes, n)
    cols = null_strings_empty(dtypes, cols, valids)
    rows, row_offs = pack_var(dtypes, cols, valids)
    rows = torch.from_numpy(rows.copy()).cuda()
    row_offs = torch.from_numpy(row_offs).cuda()
    g = _native.gpu()
    stream = _native.current_stream()
    strs = [i for i, dt in enumerate(dtypes) if dt == S]
    data = {i: Guarded(n * SIZE[dt]) for i, dt in enumerate(dtypes) if dt != S}
    masks = [Guarded(validity_nbytes(n)) for _ in dtypes]
    lens = {i: Guarded(n * 4) for i in strs}
    desc = pack_descs([(data[i].ptr if i in data else 0, masks[i].ptr,
                        0 if dt == S else SIZE[dt], offs[i])
                       for i, dt in enumerate(dtypes)])
    zero = dev_i64([0] * len(dtypes))
    lptr = dev_i64([lens[i].ptr if i in lens else 0
                    for i in range(len(dtypes))])
    # phase 0: string lengths per row
    g.from_rows_var(desc.data_ptr(), zero.data_ptr(), lptr.data_ptr(),
                    len(dtypes), n, voff, row_offs.data_ptr(),
                    rows.data_ptr(), 0, stream)
    vm = valid_matrix(valids, n)
    ooffs, chars = {}, {}
    for i in strs:
        lens[i].check(f"col {i} lengths")
        want_len = np.array([len(s) for s in cols[i]], dtype=np.int32)
        assert np.array_equal(lens[i].host().view(np.int32), want_len)
        o = np.zeros(n + 1, dtype=np.int32)
        np.cumsum(want_len, out=o[1:])
        ooffs[i] = torch.from_numpy(o).cuda()
        chars[i] = Guarded(int(o[-1]))
    assert chars[strs[0]].nbytes > 0
    cptr = dev_i64([chars[i].ptr if i in chars else 0
                    for i in range(len(dtypes))])
    optr = dev_i64([ooffs[i].data_ptr() if i in ooffs else 0
                    for i in range(len(dtypes))])
    # phase 1: fixed columns, chars and validity
    g.from_rows_var(desc.data_ptr(), cptr.data_ptr(), optr.data_ptr(),
                    len(dtypes), n, voff, row_offs.data_ptr(),
                    rows.data_ptr(), 1, stream)
    for i, dt in enumerate(dtypes):
        what = f"col {i} {dt.name}"
        masks[i].check(f"{what} validity")
        same_bytes(unpack_mask(masks[i].host(), n), vm[i], f"{what} validity")
        if dt == S:
            lens[i].check(f"{what} lengths")
            chars[i].check(f"{what} chars")
            same_bytes(chars[i].host(),
                       np.frombuffer(b"".join(cols[i]), dtype=np.uint8),
                       f"{what} chars")
        else:
            data[i].check(f"{what} data")
            same_bytes(data[i].host().reshape(n, SIZE[dt])[vm[i]],
                       cols[i][vm[i]], f"{what} data")
