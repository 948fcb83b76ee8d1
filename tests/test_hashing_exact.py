"""Exact tests of the Spark hash kernels (murmur3, xxhash64, hive_hash).

The oracle below is written from Spark's own definitions
(`Murmur3_x86_32.hashInt/hashLong/hashUnsafeBytes`, `XXH64`,
`HiveHashFunction`, `Float.floatToIntBits`) and shares no code with
`utils/sparkref.py` or the kernels' header. It recurses over Python values
with a small type description:

    DType.X                  a scalar leaf
    ("struct", [t, ...])     value: tuple, one entry per field
    ("list", t)              value: list

`None` is a null; `NullOver(v)` is a null whose buffers still hold `v` (a null
struct over live children, a null list over a non-empty range, a null scalar
over non-zero data), which must hash like `None`. FLOAT32 / FLOAT64 values are
raw bit patterns (ints), so NaN payloads and -0.0 are placed exactly.

The CPU tests pin the oracle to vectors that do not come from this project;
the GPU tests compare every row of every case with it, bit for bit.

Kept on purpose, and asserted here:
  * murmur3 / xxhash64 hash -0.0 as +0.0 (Spark's HashExpression), hive_hash
    hashes `floatToIntBits(-0.0f) = 0x80000000` unchanged.
  * hive_hash of the decimal types is not implemented and raises.
"""
import functools
import random
import re
import struct
from pathlib import Path

import numpy as np
import pytest
import torch

from spark_rapids_jni_amd.columnar import (Column, DType, _flatten,
                                           validity_from_bools)

M32 = 0xFFFFFFFF
M64 = 0xFFFFFFFFFFFFFFFF


# ---------------------------------------------------------------------------
# the oracle
# ---------------------------------------------------------------------------

class NullOver:
    """A null entry whose storage still holds `value`."""

    def __init__(self, value):
        self.value = value

    def __repr__(self):
        return f"NullOver({self.value!r})"


def _live(v):
    return None if v is None or isinstance(v, NullOver) else v


def _stored(v):
    return v.value if isinstance(v, NullOver) else v


def _s32(x):
    x &= M32
    return x - (1 << 32) if x >> 31 else x


def _s64(x):
    x &= M64
    return x - (1 << 64) if x >> 63 else x


def _rotl32(x, r):
    return ((x << r) | (x >> (32 - r))) & M32


def _rotl64(x, r):
    return ((x << r) | (x >> (64 - r))) & M64


# --- org.apache.spark.unsafe.hash.Murmur3_x86_32 ---------------------------

def _mm3_mix_k1(k1):
    k1 = (k1 * 0xCC9E2D51) & M32
    k1 = _rotl32(k1, 15)
    return (k1 * 0x1B873593) & M32


def _mm3_mix_h1(h1, k1):
    h1 = _rotl32(h1 ^ k1, 13)
    return (h1 * 5 + 0xE6546B64) & M32


def _mm3_fmix(h1, length):
    h1 ^= length
    h1 ^= h1 >> 16
    h1 = (h1 * 0x85EBCA6B) & M32
    h1 ^= h1 >> 13
    h1 = (h1 * 0xC2B2AE35) & M32
    return h1 ^ (h1 >> 16)


def mm3_int(v, seed):
    return _mm3_fmix(_mm3_mix_h1(seed & M32, _mm3_mix_k1(v & M32)), 4)


def mm3_long(v, seed):
    h1 = _mm3_mix_h1(seed & M32, _mm3_mix_k1(v & M32))
    h1 = _mm3_mix_h1(h1, _mm3_mix_k1((v >> 32) & M32))
    return _mm3_fmix(h1, 8)


def mm3_bytes(b, seed):
    """hashUnsafeBytes: little-endian words, then every tail byte mixed as a
    whole block of its own, sign-extended (Spark's variant, not the standard
    tail)."""
    h1 = seed & M32
    aligned = len(b) & ~3
    for i in range(0, aligned, 4):
        h1 = _mm3_mix_h1(h1, _mm3_mix_k1(int.from_bytes(b[i:i + 4], "little")))
    for i in range(aligned, len(b)):
        byte = b[i] - 256 if b[i] >= 128 else b[i]
        h1 = _mm3_mix_h1(h1, _mm3_mix_k1(byte & M32))
    return _mm3_fmix(h1, len(b))


# --- org.apache.spark.sql.catalyst.expressions.XXH64 -----------------------

_P1 = 0x9E3779B185EBCA87
_P2 = 0xC2B2AE3D27D4EB4F
_P3 = 0x165667B19E3779F9
_P4 = 0x85EBCA77C2B2AE63
_P5 = 0x27D4EB2F165667C5


def _xx_fmix(h):
    h ^= h >> 33
    h = (h * _P2) & M64
    h ^= h >> 29
    h = (h * _P3) & M64
    return h ^ (h >> 32)


def xx_int(v, seed):
    """XXH64.hashInt"""
    h = ((seed & M64) + _P5 + 4) & M64
    h ^= ((v & M32) * _P1) & M64
    h = (_rotl64(h, 23) * _P2 + _P3) & M64
    return _xx_fmix(h)


def xx_long(v, seed):
    """XXH64.hashLong"""
    h = ((seed & M64) + _P5 + 8) & M64
    h ^= (_rotl64(((v & M64) * _P2) & M64, 31) * _P1) & M64
    h = (_rotl64(h, 27) * _P1 + _P4) & M64
    return _xx_fmix(h)


def xx_bytes(b, seed):
    """XXH64.hashUnsafeBytes: the standard XXH64 of a byte string."""
    seed &= M64
    n = len(b)
    pos = 0
    if n >= 32:
        acc = [(seed + _P1 + _P2) & M64, (seed + _P2) & M64, seed,
               (seed - _P1) & M64]
        while pos + 32 <= n:
            for lane in range(4):
                word = int.from_bytes(b[pos:pos + 8], "little")
                a = (acc[lane] + word * _P2) & M64
                acc[lane] = (_rotl64(a, 31) * _P1) & M64
                pos += 8
        h = (_rotl64(acc[0], 1) + _rotl64(acc[1], 7) + _rotl64(acc[2], 12) +
             _rotl64(acc[3], 18)) & M64
        for a in acc:
            a = (_rotl64((a * _P2) & M64, 31) * _P1) & M64
            h = ((h ^ a) * _P1 + _P4) & M64
    else:
        h = (seed + _P5) & M64
    h = (h + n) & M64
    while pos + 8 <= n:
        k = (int.from_bytes(b[pos:pos + 8], "little") * _P2) & M64
        h ^= (_rotl64(k, 31) * _P1) & M64
        h = (_rotl64(h, 27) * _P1 + _P4) & M64
        pos += 8
    if pos + 4 <= n:
        h ^= (int.from_bytes(b[pos:pos + 4], "little") * _P1) & M64
        h = (_rotl64(h, 23) * _P2 + _P3) & M64
        pos += 4
    while pos < n:
        h ^= (b[pos] * _P5) & M64
        h = (_rotl64(h, 11) * _P1) & M64
        pos += 1
    return _xx_fmix(h)


# --- Java value semantics --------------------------------------------------

def float_to_int_bits(bits):
    """Float.floatToIntBits of the float with these raw bits."""
    bits &= M32
    if (bits & 0x7F800000) == 0x7F800000 and bits & 0x007FFFFF:
        return 0x7FC00000
    return bits


def double_to_long_bits(bits):
    bits &= M64
    if (bits & 0x7FF0000000000000) == 0x7FF0000000000000 and \
            bits & 0x000FFFFFFFFFFFFF:
        return 0x7FF8000000000000
    return bits


def java_bigint_bytes(v):
    """BigInteger.toByteArray(): bitLength() / 8 + 1 bytes, big-endian."""
    bit_length = (v if v >= 0 else ~v).bit_length()
    return v.to_bytes(bit_length // 8 + 1, "big", signed=True)


def _as_bytes(v):
    return v.encode("utf-8") if isinstance(v, str) else bytes(v)


_INT_LEAVES = (DType.INT8, DType.INT16, DType.INT32, DType.DATE32)
# Spark hashes a decimal of precision <= 18 as the long of its unscaled value
_LONG_LEAVES = (DType.INT64, DType.TIMESTAMP_US, DType.DECIMAL32,
                DType.DECIMAL64)


def _spark_leaf(fns, v, dt, seed):
    h_int, h_long, h_bytes = fns
    if dt == DType.BOOL8:
        return h_int(1 if v else 0, seed)
    if dt in _INT_LEAVES:
        return h_int(v, seed)
    if dt in _LONG_LEAVES:
        return h_long(v, seed)
    if dt == DType.DECIMAL128:
        return h_bytes(java_bigint_bytes(v), seed)
    if dt == DType.FLOAT32:    # HashExpression: -0.0f hashes as 0
        bits = float_to_int_bits(v)
        return h_int(0 if bits == 0x80000000 else bits, seed)
    if dt == DType.FLOAT64:
        bits = double_to_long_bits(v)
        return h_long(0 if bits == 1 << 63 else bits, seed)
    if dt == DType.STRING:
        return h_bytes(_as_bytes(v), seed)
    raise NotImplementedError(dt)


def _spark_value(fns, v, t, seed):
    """A null leaves the running hash alone; struct fields and list elements
    chain through it in order."""
    v = _live(v)
    if v is None:
        return seed
    if isinstance(t, tuple):
        if t[0] == "struct":
            for field, ft in zip(v, t[1]):
                seed = _spark_value(fns, field, ft, seed)
        else:
            for elem in v:
                seed = _spark_value(fns, elem, t[1], seed)
        return seed
    return _spark_leaf(fns, v, t, seed)


_MM3 = (mm3_int, mm3_long, mm3_bytes)
_XX = (xx_int, xx_long, xx_bytes)


def murmur3_row(values, types, seed=42):
    h = seed & M32
    for v, t in zip(values, types):
        h = _spark_value(_MM3, v, t, h)
    return _s32(h)


def xxhash64_row(values, types, seed=42):
    h = seed & M64
    for v, t in zip(values, types):
        h = _spark_value(_XX, v, t, h)
    return _s64(h)


def hive_timestamp(us):
    """HiveHashFunction.hashTimestamp; Java's / and % truncate toward zero."""
    sec = abs(us) // 1_000_000
    if us < 0:
        sec = -sec
    ns = (us - sec * 1_000_000) * 1000
    r = ((sec << 30) | ns) & M64
    return _s32((r >> 32) ^ r)


def hive_long(v):
    u = v & M64
    return _s32(u ^ (u >> 32))


def hive_string(b):
    h = 0
    for byte in b:
        h = (h * 31 + (byte - 256 if byte >= 128 else byte)) & M32
    return _s32(h)


def hive_value(v, t):
    v = _live(v)
    if v is None:
        return 0
    if isinstance(t, tuple):
        h = 0
        for elem, et in (zip(v, t[1]) if t[0] == "struct"
                         else ((e, t[1]) for e in v)):
            h = (31 * h + hive_value(elem, et)) & M32
        return _s32(h)
    if t == DType.BOOL8:
        return 1 if v else 0
    if t in _INT_LEAVES:
        return v
    if t == DType.INT64:
        return hive_long(v)
    if t == DType.TIMESTAMP_US:
        return hive_timestamp(v)
    if t == DType.FLOAT32:
        return _s32(float_to_int_bits(v))
    if t == DType.FLOAT64:
        return hive_long(double_to_long_bits(v))
    if t == DType.STRING:
        return hive_string(_as_bytes(v))
    raise NotImplementedError(t)


def hive_row(values, types):
    h = 0
    for v, t in zip(values, types):
        h = (31 * h + hive_value(v, t)) & M32
    return _s32(h)


ROW_ORACLES = {"murmur3": murmur3_row, "xxhash64": xxhash64_row,
               "hive": hive_row}


# ---------------------------------------------------------------------------
# the oracle is pinned (CPU)
# ---------------------------------------------------------------------------

def _pattern_bytes(n):
    return bytes((i * 131 + 89 + (i >> 3)) & 0xFF for i in range(n))


def test_oracle_xxh64_matches_xxhash_module():
    import xxhash
    for seed in (0, 42, 2**64 - 1):
        for n in list(range(101)) + [255, 256, 257]:
            b = _pattern_bytes(n)
            assert xx_bytes(b, seed) == xxhash.xxh64(b, seed=seed).intdigest(), \
                (seed, n)
        for v in (0, 1, -1, 42, 2**31 - 1, -2**31, 0x12345678):
            assert xx_int(v, seed) == xxhash.xxh64(
                struct.pack("<i", v), seed=seed).intdigest(), (seed, v)
        for v in (0, 1, -1, 42, 2**63 - 1, -2**63, 0x123456789ABCDEF):
            assert xx_long(v, seed) == xxhash.xxh64(
                struct.pack("<q", v), seed=seed).intdigest(), (seed, v)


def test_oracle_spark_sql_documentation_examples():
    # SELECT hash('Spark', array(123), 2) and SELECT xxhash64(...) in the
    # Spark SQL function reference; both chain from seed 42.
    types = [DType.STRING, ("list", DType.INT32), DType.INT32]
    row = ["Spark", [123], 2]
    assert murmur3_row(row, types) == -1321691492
    assert xxhash64_row(row, types) == 5602566077635097486


def test_oracle_murmur3_canonical_vectors():
    # published MurmurHash3_x86_32 verification vectors; for lengths that are
    # a multiple of 4 Spark's variant is the standard algorithm
    vecs = [(b"", 0, 0x00000000),
            (b"", 1, 0x514E28B7),
            (b"", 0xFFFFFFFF, 0x81F16F39),
            (b"\x00\x00\x00\x00", 0, 0x2362F9DE),
            (b"\xff\xff\xff\xff", 0, 0x76293B50),
            (b"\x21\x43\x65\x87", 0, 0xF55B516B),
            (b"\x21\x43\x65\x87", 0x5082EDEE, 0x2362F9DE),
            (b"aaaa", 0x9747B28C, 0x5A97808A),
            (b"abcd", 0x9747B28C, 0xF0478627)]
    for data, seed, exp in vecs:
        assert mm3_bytes(data, seed) == exp, (data, seed)
    assert mm3_int(0, 0) == 0x2362F9DE
    assert mm3_int(-1, 0) == 0x76293B50
    assert mm3_int(struct.unpack("<i", b"\x21\x43\x65\x87")[0], 0) == 0xF55B516B
    for v in (0, 1, -1, 42, 2**31 - 1, -2**31):
        assert mm3_int(v, 42) == mm3_bytes(struct.pack("<i", v), 42)
    for v in (0, 1, -1, 42, 2**63 - 1, -2**63):
        assert mm3_long(v, 42) == mm3_bytes(struct.pack("<q", v), 42)


def test_oracle_murmur3_iceberg_vectors():
    # Iceberg spec, Appendix B (the vectors of test_murmur3_std_oracle_vectors
    # whose byte length is a multiple of 4, where Spark's variant applies)
    assert _s32(mm3_long(34, 0)) == 2017239379
    assert _s32(mm3_long(17486, 0)) == -653330422
    assert _s32(mm3_long(1510871468000000, 0)) == -2047944441
    assert _s32(mm3_bytes(b"\x00\x01\x02\x03", 0)) == -188683207
    # a tail byte is mixed as a block of its own, so these two differ from the
    # standard algorithm's -500754589 and 1210000089
    assert _s32(mm3_bytes(b"\x05\x8c", 0)) != -500754589
    assert _s32(mm3_bytes(b"iceberg", 0)) != 1210000089


def test_oracle_hive_timestamp():
    # computed by hand from HiveHashFunction.hashTimestamp:
    # sec = us / 1e6, ns = (us % 1e6) * 1000 (truncating), r = sec << 30 | ns,
    # (int)((r >>> 32) ^ r)
    assert hive_timestamp(0x123456789ABCDEF) == -660040456
    assert hive_timestamp(-0x123456789ABCDEF) == 486894999
    assert hive_timestamp(1_000_000) == 1073741824
    assert hive_timestamp(-1_000_001) == 999
    assert hive_timestamp(100) == 100000
    assert hive_timestamp(-100) == 99999
    assert hive_timestamp(0) == 0


def test_oracle_hive_java_hashcodes():
    # String.hashCode
    assert hive_string(b"") == 0
    assert hive_string(b"a") == 97
    assert hive_string(b"ab") == 3105
    # Long.hashCode
    assert hive_long(1) == 1
    assert hive_long(-1) == 0
    assert hive_long(2**32) == 1
    assert hive_long(-2**63) == -2**31
    # Float.floatToIntBits / Double.doubleToLongBits
    assert float_to_int_bits(0x00000000) == 0
    assert float_to_int_bits(0x80000000) == 0x80000000
    assert float_to_int_bits(0x7F800000) == 0x7F800000
    assert float_to_int_bits(0xFF800000) == 0xFF800000
    for nan in (0x7F800001, 0x7FFFFFFF, 0xFF800001, 0xFFFFFFFF):
        assert float_to_int_bits(nan) == 0x7FC00000
    for nan in (0x7FF0000000000001, 0x7FFFFFFFFFFFFFFF, 0xFFF0000000000001,
                0xFFFFFFFFFFFFFFFF):
        assert double_to_long_bits(nan) == 0x7FF8000000000000
    assert double_to_long_bits(1 << 63) == 1 << 63
    # hive keeps the sign bit of -0.0 ...
    assert hive_value(0x80000000, DType.FLOAT32) == _s32(0x80000000)
    assert hive_value(1 << 63, DType.FLOAT64) == _s32(0x80000000)
    # ... murmur3 and xxhash64 hash it as +0.0
    assert murmur3_row([0x80000000], [DType.FLOAT32]) == \
        murmur3_row([0], [DType.FLOAT32])
    assert xxhash64_row([1 << 63], [DType.FLOAT64]) == \
        xxhash64_row([0], [DType.FLOAT64])
    # BigInteger.toByteArray
    for v, exp in [(0, "00"), (-1, "ff"), (127, "7f"), (128, "0080"),
                   (-128, "80"), (-129, "ff7f"), (255, "00ff"),
                   (-256, "ff00"), (2**127 - 1, "7f" + "ff" * 15),
                   (-2**127, "80" + "00" * 15)]:
        assert java_bigint_bytes(v).hex() == exp, v


def test_oracle_nested_rules():
    ll = ("list", ("list", DType.INT32))
    a, b = [[1, 0], [2]], [[1], [0, 2]]
    # hive: a list hashes to one int first, 31 * 31 + 2 against 31 + 2
    assert hive_row([a], [ll]) == 963
    assert hive_row([b], [ll]) == 33
    # murmur3 / xxhash64 chain the leaves, list boundaries leave no trace
    assert murmur3_row([a], [ll]) == murmur3_row([b], [ll])
    assert xxhash64_row([a], [ll]) == xxhash64_row([b], [ll])
    st = ("struct", [DType.INT32, DType.STRING])
    for fn, null in ((murmur3_row, 42), (xxhash64_row, 42), (hive_row, 0)):
        assert fn([None], [st]) == null
        assert fn([NullOver((7, "zz"))], [st]) == null
        assert fn([(7, "zz")], [st]) != null


# ---------------------------------------------------------------------------
# values and columns
# ---------------------------------------------------------------------------

SCALAR_DTYPES = [DType.BOOL8, DType.INT8, DType.INT16, DType.INT32,
                 DType.INT64, DType.FLOAT32, DType.FLOAT64, DType.DATE32,
                 DType.TIMESTAMP_US, DType.STRING, DType.DECIMAL32,
                 DType.DECIMAL64, DType.DECIMAL128]
DECIMALS = (DType.DECIMAL32, DType.DECIMAL64, DType.DECIMAL128)
HIVE_DTYPES = [dt for dt in SCALAR_DTYPES if dt not in DECIMALS]

_INT_BITS = {DType.INT8: 8, DType.INT16: 16, DType.INT32: 32, DType.DATE32: 32,
             DType.INT64: 64, DType.TIMESTAMP_US: 64, DType.DECIMAL32: 32,
             DType.DECIMAL64: 64, DType.DECIMAL128: 128}


def _high_bytes(rng, n):
    b = bytearray(rng.getrandbits(8) for _ in range(n))
    for i in range(0, n, 3):
        b[i] |= 0x80
    return bytes(b)


def _rand(dt, rng):
    if dt == DType.BOOL8:
        return rng.random() < 0.5
    if dt == DType.FLOAT32:
        return rng.getrandbits(32)
    if dt == DType.FLOAT64:
        return rng.getrandbits(64)
    if dt == DType.STRING:
        return _high_bytes(rng, rng.randint(0, 24))
    bits = _INT_BITS[dt]
    # every magnitude, so every DECIMAL128 byte length, turns up
    return rng.randint(-2**(bits - 1), 2**(bits - 1) - 1) >> rng.randint(0, bits - 2)


def _edges(dt, rng):
    if dt == DType.BOOL8:
        return [True, False]
    if dt == DType.FLOAT32:
        return [0x00000000, 0x80000000, 0x7F800000, 0xFF800000,     # +-0 +-inf
                0x7F800001, 0x7FFFFFFF, 0xFF800001, 0xFFFFFFFF,     # NaNs
                0x7FC00000, 0xFFC00000,
                0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF,     # denormal
                0x00800000, 0x7F7FFFFF, 0xFF7FFFFF, 0x3F800000, 0xBFC00000]
    if dt == DType.FLOAT64:
        return [0, 1 << 63, 0x7FF0000000000000, 0xFFF0000000000000,
                0x7FF0000000000001, 0x7FFFFFFFFFFFFFFF, 0xFFF0000000000001,
                0xFFFFFFFFFFFFFFFF, 0x7FF8000000000000, 0xFFF8000000000000,
                0x0000000000000001, 0x8000000000000001, 0x000FFFFFFFFFFFFF,
                0x800FFFFFFFFFFFFF, 0x0010000000000000, 0x7FEFFFFFFFFFFFFF,
                0xFFEFFFFFFFFFFFFF, 0x3FF0000000000000, 0xBFF8000000000000,
                # only one half non-zero: hive folds the halves together
                0x0000000080000000, 0x8000000080000000]
    if dt == DType.STRING:
        return [_high_bytes(rng, n) for n in
                list(range(41)) + [63, 64, 65, 127, 128, 129]]
    bits = _INT_BITS[dt]
    out = [-2**(bits - 1), 2**(bits - 1) - 1, 0, 1, -1]
    if dt == DType.TIMESTAMP_US:
        out += [999_999, -999_999, 1_000_000, -1_000_000, 1_000_001,
                -1_000_001, 0x123456789ABCDEF, -0x123456789ABCDEF]
    if dt == DType.DECIMAL128:
        for k in range(1, 17):      # BigInteger byte lengths 1..16, both signs
            out += [2**(8 * k - 1) - 1, -2**(8 * k - 1)]
            if k < 16:              # one past: needs the extra sign byte
                out += [2**(8 * k - 1), -2**(8 * k - 1) - 1]
    return out


N_SCALAR = 320      # more than one 256-thread block, five validity words


@functools.lru_cache(maxsize=None)
def _scalar_case(dt):
    """(values, {hash: expected per value}) for one dtype, computed once."""
    rng = random.Random(1000 + int(dt))
    vals = _edges(dt, rng)
    while len(vals) < N_SCALAR:
        vals.append(_rand(dt, rng))
    names = ["murmur3", "xxhash64"] + ([] if dt in DECIMALS else ["hive"])
    exp = {name: tuple(ROW_ORACLES[name]([v], [dt]) for v in vals)
           for name in names}
    return tuple(vals), exp


def _leaf_column(dt, values, device):
    n = len(values)
    stored = [_stored(v) for v in values]
    if dt in (DType.FLOAT32, DType.FLOAT64):
        raw, as_float = ((np.uint32, np.float32) if dt == DType.FLOAT32
                         else (np.uint64, np.float64))
        arr = np.array([0 if v is None else v for v in stored], dtype=raw)
        col = Column(dt, n, torch.from_numpy(arr.view(as_float)).to(device))
    else:
        col = Column.from_pylist(stored, dt, device)
    valid = [_live(v) is not None for v in values]
    if not all(valid):
        col.validity = validity_from_bools(valid, device)
        col._null_count = n - sum(valid)
    return col


def build_column(t, values, device="cuda"):
    """The Column of type description `t` holding `values`."""
    if not isinstance(t, tuple):
        return _leaf_column(t, values, device)
    n = len(values)
    valid = [_live(v) is not None for v in values]
    validity = None if all(valid) else validity_from_bools(valid, device)
    nulls = n - sum(valid)
    if t[0] == "struct":
        kids = [build_column(ft, [None if v is None else _stored(v)[k]
                                  for v in values], device)
                for k, ft in enumerate(t[1])]
        return Column(DType.STRUCT, n, None, validity, children=kids,
                      null_count=nulls)
    offsets, elems = [0], []
    for v in values:
        if v is not None:
            elems.extend(_stored(v))
        offsets.append(len(elems))
    child = build_column(t[1], elems, device)
    return Column(DType.LIST, n, None, validity,
                  torch.tensor(offsets, dtype=torch.int32, device=device),
                  [child], null_count=nulls)


def _gpu(name, cols, seed=None):
    from spark_rapids_jni_amd.ops import hashing
    if name == "hive":
        out = hashing.hive_hash(cols)
    else:
        fn = getattr(hashing, name)
        out = fn(cols) if seed is None else fn(cols, seed)
    return out.data.cpu().tolist()


def _assert_rows(name, got, exp, rows):
    assert len(got) == len(exp)
    bad = [i for i in range(len(exp)) if got[i] != exp[i]]
    assert not bad, (f"{name}: {len(bad)} of {len(exp)} rows differ; first "
                     f"row {bad[0]} {rows[bad[0]]!r}: got {got[bad[0]]}, "
                     f"expected {exp[bad[0]]}")


def _check_table(types, columns_values, names=("murmur3", "xxhash64", "hive"),
                 seeds=None):
    """Hash the table on the GPU with each hash and compare every row."""
    cols = [build_column(t, list(v)) for t, v in zip(types, columns_values)]
    rows = list(zip(*columns_values))
    results = {}
    for name in names:
        seed = (seeds or {}).get(name)
        kw = {} if seed is None or name == "hive" else {"seed": seed}
        exp = [ROW_ORACLES[name](r, types, **kw) for r in rows]
        got = _gpu(name, cols, seed)
        _assert_rows(name, got, exp, rows)
        results[name] = got
    return results


# ---------------------------------------------------------------------------
# CPU: layout, host checks, the two oracles
# ---------------------------------------------------------------------------

def test_flatten_keeps_siblings_adjacent():
    # STRUCT<STRUCT<int,float>, decimal64>: child k of a node is child0 + k
    t = ("struct", [("struct", [DType.INT32, DType.FLOAT32]), DType.DECIMAL64])
    s = build_column(t, [((1, 0), 2)], "cpu")
    a, b = s.children
    flat, top, child0 = _flatten([s, b])
    assert top == [0, 5]
    assert [id(c) for c in flat] == [id(c) for c in
                                     (s, a, b, a.children[0], a.children[1], b)]
    assert child0 == [1, 3, 0, 0, 0, 0]
    for i, c in enumerate(flat):
        for k, ch in enumerate(c.children):
            assert flat[child0[i] + k] is ch


def _nest(depth, kind):
    """A type nested `depth` deep over INT32: structs, lists or both in turn."""
    t = DType.INT32
    for level in range(depth):
        if kind == "struct" or (kind == "mixed" and level % 2 == 0):
            t = ("struct", [t, DType.INT32] if kind == "mixed" else [t])
        else:
            t = ("list", t)
    return t


@pytest.mark.parametrize("kind", ["struct", "list", "mixed"])
def test_depth_9_is_refused_on_the_host(kind):
    from spark_rapids_jni_amd.ops import hashing
    t = _nest(9, kind)
    rng = random.Random(9)
    col = build_column(t, [_gen(t, rng, max_len=1) for _ in range(4)], "cpu")
    for fn in (hashing.murmur3, hashing.xxhash64, hashing.hive_hash):
        # CPU columns: the refusal comes before the device is looked at
        with pytest.raises(ValueError, match="nested 9 deep"):
            fn([col])
        with pytest.raises(ValueError, match="nested 9 deep"):
            fn([build_column(DType.INT32, [1, 2, 3, 4], "cpu"), col])


@pytest.mark.parametrize("dt", DECIMALS, ids=lambda d: d.name)
def test_hive_hash_refuses_decimals_on_the_host(dt):
    from spark_rapids_jni_amd.ops import hashing
    leaf = build_column(dt, [1, None, -3], "cpu")
    with pytest.raises(ValueError, match="does not define"):
        hashing.hive_hash([leaf])
    nested = build_column(("list", ("struct", [DType.INT32, dt])),
                          [[(1, 2)], [], None], "cpu")
    with pytest.raises(ValueError, match="does not define"):
        hashing.hive_hash([build_column(DType.INT32, [1, 2, 3], "cpu"), nested])


def test_ragged_input_is_refused_on_the_host():
    from spark_rapids_jni_amd.ops import hashing
    a = build_column(DType.INT32, [1, 2, 3], "cpu")
    b = build_column(DType.INT32, [1, 2], "cpu")
    with pytest.raises(ValueError, match="rows"):
        hashing.murmur3([a, b])
    s = Column(DType.STRUCT, 3, None, children=[a, b])
    with pytest.raises(ValueError, match="rows"):
        hashing.hive_hash([s])


def _bits_to_float(dt, v):
    if dt == DType.FLOAT32:
        return struct.unpack("<f", struct.pack("<I", v))[0]
    if dt == DType.FLOAT64:
        return struct.unpack("<d", struct.pack("<Q", v))[0]
    return v


def test_oracles_agree():
    """utils/sparkref.py, the oracle of test_hashing.py, gives what this one
    gives on every scalar dtype (it has no nested types)."""
    from spark_rapids_jni_amd.utils import sparkref
    for dt in SCALAR_DTYPES:
        vals, exp = _scalar_case(dt)
        for i, v in enumerate(vals):
            pv = _bits_to_float(dt, v)
            assert sparkref.murmur3_row([pv], [dt]) == exp["murmur3"][i], (dt, v)
            assert sparkref.xxhash64_row([pv], [dt]) == exp["xxhash64"][i], (dt, v)
            if dt not in DECIMALS:
                assert sparkref.hive_hash_row([pv], [dt]) == exp["hive"][i], (dt, v)
    rng = random.Random(77)
    for _ in range(200):
        row = [None if rng.random() < 0.2 else _rand(dt, rng)
               for dt in HIVE_DTYPES]
        prow = [None if v is None else _bits_to_float(dt, v)
                for dt, v in zip(HIVE_DTYPES, row)]
        for seed in (0, 42, -1):
            assert sparkref.murmur3_row(prow, HIVE_DTYPES, seed) == \
                murmur3_row(row, HIVE_DTYPES, seed)
        assert sparkref.xxhash64_row(prow, HIVE_DTYPES, -2**63) == \
            xxhash64_row(row, HIVE_DTYPES, -2**63)
        assert sparkref.hive_hash_row(prow, HIVE_DTYPES) == \
            hive_row(row, HIVE_DTYPES)


# ---------------------------------------------------------------------------
# GPU: scalars
# ---------------------------------------------------------------------------

def _valid_mask(pattern, n):
    if pattern == "none":
        return [True] * n
    if pattern == "all":
        return [False] * n
    if pattern == "alternating":
        return [i % 2 == 1 for i in range(n)]
    return [i not in (63, 64, 65) for i in range(n)]   # byte and word boundary


@pytest.mark.gpu
@pytest.mark.parametrize("pattern", ["none", "all", "alternating", "b63_64_65"])
@pytest.mark.parametrize("dt", SCALAR_DTYPES, ids=lambda d: d.name)
def test_gpu_scalar(dt, pattern):
    vals, exp = _scalar_case(dt)
    valid = _valid_mask(pattern, len(vals))
    # a null keeps its data underneath, which must not be read into the hash
    col = build_column(dt, [v if ok else NullOver(v)
                            for v, ok in zip(vals, valid)])
    for name, exp_rows in exp.items():
        null = ROW_ORACLES[name]([None], [dt])
        want = [e if ok else null for e, ok in zip(exp_rows, valid)]
        _assert_rows(name, _gpu(name, [col]), want, vals)


@pytest.mark.gpu
@pytest.mark.parametrize("name,seed", [("murmur3", 0), ("murmur3", 1),
                                       ("murmur3", -1), ("xxhash64", 0),
                                       ("xxhash64", -2**63)])
def test_gpu_seeds(name, seed):
    # Java seeds are signed; -1 and Long.MIN_VALUE must reach the kernel whole
    rng = random.Random(31)
    types = [DType.INT32, DType.STRING, DType.FLOAT64, DType.INT64]
    cols = [[None if rng.random() < 0.15 else _rand(t, rng)
             for _ in range(300)] for t in types]
    cols[0][0] = cols[1][0] = cols[2][0] = cols[3][0] = None   # seed comes back
    got = _check_table(types, cols, names=(name,), seeds={name: seed})[name]
    assert got[0] == seed
    # and the seed matters: the default one gives other hashes
    assert got != _gpu(name, [build_column(t, c) for t, c in zip(types, cols)])


# ---------------------------------------------------------------------------
# GPU: column chaining
# ---------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("ncols", [1, 2, 17])
def test_gpu_chained_columns(ncols):
    rng = random.Random(50 + ncols)
    types = [HIVE_DTYPES[(3 * k + 3) % len(HIVE_DTYPES)] for k in range(ncols)]
    n = 300
    cols = [[None if rng.random() < 0.2 else _rand(t, rng) for _ in range(n)]
            for t in types]
    for c in cols:                      # rows 0, 64 and n-1 are null throughout
        c[0] = c[64] = c[n - 1] = None
    got = _check_table(types, cols)
    for r in (0, 64, n - 1):
        assert got["murmur3"][r] == 42
        assert got["xxhash64"][r] == 42
        assert got["hive"][r] == 0


@pytest.mark.gpu
def test_gpu_column_order_matters():
    a = list(range(1, 301))
    b = [1000 + 7 * i for i in range(300)]
    types = [DType.INT32, DType.INT32]
    ab = _check_table(types, [a, b])
    ba = _check_table(types, [b, a])
    for name in ab:
        # a[i] != b[i] in every row, and 30 * (a - b) != 0 mod 2^32 for hive
        assert all(x != y for x, y in zip(ab[name], ba[name])), name


# ---------------------------------------------------------------------------
# GPU: nested
# ---------------------------------------------------------------------------

def _gen(t, rng, max_len=4):
    r = rng.random()
    if isinstance(t, tuple):
        if t[0] == "struct":
            live = tuple(_gen(ft, rng, max_len) for ft in t[1])
            if r < 0.08:
                return None
            if r < 0.16:
                return NullOver(live)       # null parent over live children
            return live
        if r < 0.08:
            return None
        if r < 0.14:                        # null list over a non-empty range
            return NullOver([_gen(t[1], rng, max_len) for _ in range(2)])
        if r < 0.26:
            return []
        return [_gen(t[1], rng, max_len)
                for _ in range(rng.randint(1, max_len))]
    if r < 0.15:
        return None
    if t == DType.INT32:                    # small values collide in hive if
        return rng.randint(-3, 3)           # the structure is lost
    return _rand(t, rng)


_I, _L, _F, _S = DType.INT32, DType.INT64, DType.FLOAT32, DType.STRING
NESTED_SHAPES = {
    "struct_int_string": ("struct", [_I, _S]),
    "struct_struct_int_float_dec64": ("struct", [("struct", [_I, _F]),
                                                 DType.DECIMAL64]),
    "struct_list_int_long": ("struct", [("list", _I), _L]),
    "struct3_int": ("struct", [("struct", [("struct", [_I]), _I]), _I]),
    "list_int": ("list", _I),
    "list_string": ("list", _S),
    "list_list_int": ("list", ("list", _I)),
    "list_struct_int_string": ("list", ("struct", [_I, _S])),
    "struct_list_struct_int_list_int": ("struct", [("list", ("struct", [
        _I, ("list", _I)]))]),
}


def _has_decimal(t):
    if isinstance(t, tuple):
        return any(_has_decimal(x) for x in (t[1] if t[0] == "struct" else [t[1]]))
    return t in DECIMALS


def _hashes_for(t):
    return ("murmur3", "xxhash64") if _has_decimal(t) else \
        ("murmur3", "xxhash64", "hive")


@pytest.mark.gpu
@pytest.mark.parametrize("shape", list(NESTED_SHAPES))
def test_gpu_nested(shape):
    t = NESTED_SHAPES[shape]
    rng = random.Random(len(shape) * 101)
    vals = [_gen(t, rng) for _ in range(300)]
    _check_table([t], [vals], names=_hashes_for(t))
    # between two scalar columns the nested one still chains in its place
    before = [_rand(_L, rng) for _ in vals]
    after = [None if i % 5 == 0 else _rand(_S, rng) for i in range(len(vals))]
    _check_table([_L, t, _S], [before, vals, after], names=_hashes_for(t))


@pytest.mark.gpu
def test_gpu_struct_with_nested_first_child_under_hive():
    # the sibling-indexing shape with a hive-hashable second child
    t = ("struct", [("struct", [_I, _F]), _L])
    rng = random.Random(5)
    vals = [_gen(t, rng) for _ in range(300)]
    vals[0] = ((1, 0x3F800000), 2**40 + 5)
    _check_table([t], [vals])


@pytest.mark.gpu
def test_gpu_null_parent_hides_children():
    t = ("struct", [_I, _S])
    vals = [(7, "zz"), NullOver((7, "zz")), None, (None, "zz"), (7, None),
            (None, None)]
    got = _check_table([t], [vals])
    for name, null in (("murmur3", 42), ("xxhash64", 42), ("hive", 0)):
        g = got[name]
        assert g[1] == g[2] == null, name          # children do not contribute
        assert g[0] != null, name
        assert len({g[0], g[3], g[4]}) == 3, name  # a child's own nulls count
        assert g[5] == null, name   # valid struct, null fields: seed / 31*0+0
    lt = ("list", _I)
    lvals = [[1, 2], NullOver([1, 2]), None, [], [None, 2], [1, None]]
    got = _check_table([lt], [lvals])
    for name, null in (("murmur3", 42), ("xxhash64", 42), ("hive", 0)):
        g = got[name]
        assert g[1] == g[2] == g[3] == null, name
        assert g[0] != null, name


@pytest.mark.gpu
def test_gpu_sublist_structure():
    ll = ("list", ("list", _I))
    vals = [[[1, 0], [2]], [[1], [0, 2]], [[1, 0, 2]], [[], [1, 0, 2], []]]
    got = _check_table([ll], [vals])
    # hive hashes each inner list to an int first: 31 * (31 * 1 + 0) + 2
    # against 31 * 1 + (31 * 0 + 2)
    assert got["hive"][0] == 963
    assert got["hive"][1] == 33
    # murmur3 / xxhash64 chain the leaves and ignore where the lists end
    for name in ("murmur3", "xxhash64"):
        assert len(set(got[name])) == 1, name


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["struct", "list", "mixed"])
def test_gpu_depth_8(kind):
    t = _nest(8, kind)
    rng = random.Random(8)
    vals = [_gen(t, rng, max_len=2) for _ in range(200)]
    # a row that is live all the way down, so the deepest leaf is hashed
    v = 5
    for level in range(8):
        if kind == "struct" or (kind == "mixed" and level % 2 == 0):
            v = (v, level) if kind == "mixed" else (v,)
        else:
            v = [v, v] if level < 3 else [v]
    vals[0] = v
    _check_table([t], [vals])


# ---------------------------------------------------------------------------
# GPU: the grid-stride loop's second lap
# ---------------------------------------------------------------------------

def _launch_limits():
    """(grid cap, block size) of the hash launches, from the kernels' header."""
    text = (Path(__file__).resolve().parents[1] / "src" / "gpu" /
            "srj_common.hpp").read_text()
    block = int(re.search(r"constexpr int DEFAULT_BLOCK = (\d+);", text).group(1))
    cap = int(re.search(r"constexpr int64_t MAX_GRID = (\d+);", text).group(1))
    assert re.search(r"grid_1d\(int64_t n, int block = DEFAULT_BLOCK, "
                     r"int64_t cap = MAX_GRID\)", text)
    return cap, block


def _np_rotl(x, r, bits):
    return (x << x.dtype.type(r)) | (x >> x.dtype.type(bits - r))


def np_mm3_long(v, seed):
    u = v.view(np.uint64)
    h = np.full(v.shape, seed & M32, dtype=np.uint32)
    for half in ((u & np.uint64(M32)).astype(np.uint32),
                 (u >> np.uint64(32)).astype(np.uint32)):
        k = half * np.uint32(0xCC9E2D51)
        k = _np_rotl(k, 15, 32) * np.uint32(0x1B873593)
        h = _np_rotl(h ^ k, 13, 32) * np.uint32(5) + np.uint32(0xE6546B64)
    h ^= np.uint32(8)
    h ^= h >> np.uint32(16)
    h *= np.uint32(0x85EBCA6B)
    h ^= h >> np.uint32(13)
    h *= np.uint32(0xC2B2AE35)
    h ^= h >> np.uint32(16)
    return h.view(np.int32)


def np_xx_long(v, seed):
    u = v.view(np.uint64)
    h = np.full(v.shape, (seed + _P5 + 8) & M64, dtype=np.uint64)
    h ^= _np_rotl(u * np.uint64(_P2), 31, 64) * np.uint64(_P1)
    h = _np_rotl(h, 27, 64) * np.uint64(_P1) + np.uint64(_P4)
    h ^= h >> np.uint64(33)
    h *= np.uint64(_P2)
    h ^= h >> np.uint64(29)
    h *= np.uint64(_P3)
    h ^= h >> np.uint64(32)
    return h.view(np.int64)


def np_hive_long(v):
    u = v.view(np.uint64)
    return (u ^ (u >> np.uint64(32))).astype(np.uint32).view(np.int32)


def test_numpy_long_oracles_match_the_scalar_oracle():
    v = _lap_values(1000)
    for seed in (42, 0, -1):
        assert np_mm3_long(v, seed).tolist() == \
            [murmur3_row([x], [_L], seed) for x in v.tolist()]
        assert np_xx_long(v, seed).tolist() == \
            [xxhash64_row([x], [_L], seed) for x in v.tolist()]
    assert np_hive_long(v).tolist() == [hive_row([x], [_L]) for x in v.tolist()]


def _lap_values(n):
    v = np.random.default_rng(2048).integers(-2**63, 2**63 - 1, size=n,
                                             dtype=np.int64, endpoint=True)
    edge = np.array([0, 1, -1, 2**32, -2**63, 2**63 - 1], dtype=np.int64)
    v[:min(n, len(edge))] = edge[:n]
    return v


@pytest.mark.gpu
def test_gpu_second_lap():
    from spark_rapids_jni_amd.ops import hashing
    cap, block = _launch_limits()
    n = cap * block + 65        # every thread of the first wave, and one more
    v = _lap_values(n)
    head = v[:1000].tolist()
    assert np_mm3_long(v[:1000], 42).tolist() == \
        [murmur3_row([x], [_L]) for x in head]
    assert np_xx_long(v[:1000], 42).tolist() == \
        [xxhash64_row([x], [_L]) for x in head]
    assert np_hive_long(v[:1000]).tolist() == [hive_row([x], [_L]) for x in head]
    col = Column.from_torch(torch.from_numpy(v).cuda())
    for name, got, exp in (
            ("murmur3", hashing.murmur3([col]), np_mm3_long(v, 42)),
            ("xxhash64", hashing.xxhash64([col]), np_xx_long(v, 42)),
            ("hive", hashing.hive_hash([col]), np_hive_long(v))):
        got = got.data.cpu().numpy()
        bad = np.flatnonzero(got != exp)
        assert bad.size == 0, (f"{name}: {bad.size} rows differ, first row "
                               f"{bad[0]} of {n} (second lap starts at "
                               f"{cap * block}): got {got[bad[0]]}, expected "
                               f"{exp[bad[0]]}")


@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1])
def test_gpu_zero_and_one_row(n):
    vals = [-2**63][:n]
    col = Column.from_torch(torch.tensor(vals, dtype=torch.int64, device="cuda"))
    for name in ROW_ORACLES:
        assert _gpu(name, [col]) == [ROW_ORACLES[name]([x], [_L]) for x in vals]
