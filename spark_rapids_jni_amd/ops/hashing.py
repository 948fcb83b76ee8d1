"""Spark-exact hash ops (Java API parity: com.nvidia.spark.rapids.jni.Hash).

Reference behavior: Hash.java + src/main/cpp/src/hash/*.cu in
NVIDIA/spark-rapids-jni. Seeds chain column-to-column;
nulls pass the running seed/hash through (murmur3/xxhash64) or contribute 0
(hive). Defaults match Spark: murmur3 seed 42, xxhash64 seed 42.
"""
from typing import Sequence, Union

import torch

from .. import _native
from ..columnar import Column, DType, Table, pack_descriptors

DEFAULT_MURMUR3_SEED = 42
DEFAULT_XXHASH64_SEED = 42

# Maximum nesting depth accepted (Hash.java MAX_STACK_DEPTH): a LIST or STRUCT
# is one level deeper than its deepest child, a scalar column is depth 0.
MAX_STACK_DEPTH = 8

_NESTED = (DType.LIST, DType.STRUCT)
_SPARK_LEAVES = frozenset(DType) - frozenset(_NESTED)
# hive_hash of decimals (HiveHashFunction.normalizeDecimal + BigDecimal
# .hashCode) is not implemented; they are refused, never hashed as something
# else.
_HIVE_LEAVES = _SPARK_LEAVES - {DType.DECIMAL32, DType.DECIMAL64,
                                DType.DECIMAL128}


def _nested_depth(c: Column, leaves, name: str, path: str) -> int:
    """Depth of one column tree; raises ValueError on a dtype `name` does not
    define or a malformed LIST/STRUCT. Host-only: reads no device memory."""
    if c.dtype == DType.LIST:
        if len(c.children) != 1 or c.offsets is None:
            raise ValueError(f"{name}: {path} LIST needs offsets and one child")
        if c.offsets.numel() != c.size + 1:
            raise ValueError(f"{name}: {path} LIST of {c.size} rows has "
                             f"{c.offsets.numel()} offsets")
        return 1 + _nested_depth(c.children[0], leaves, name, path + "[]")
    if c.dtype == DType.STRUCT:
        depth = 0
        for k, ch in enumerate(c.children):
            if ch.size != c.size:
                raise ValueError(f"{name}: {path}.{k} has {ch.size} rows, "
                                 f"its struct {c.size}")
            depth = max(depth, _nested_depth(ch, leaves, name, f"{path}.{k}"))
        return 1 + depth
    if c.dtype not in leaves:
        raise ValueError(f"{name}: {path} has dtype {c.dtype.name}, which "
                         f"{name} does not define")
    return 0


def _cols(table_or_cols: Union[Table, Sequence[Column]], leaves, name: str):
    cols = table_or_cols.columns if isinstance(table_or_cols, Table) else list(table_or_cols)
    assert cols, "need at least one column"
    for i, c in enumerate(cols):
        if c.size != cols[0].size:
            raise ValueError(f"{name}: column {i} has {c.size} rows, "
                             f"column 0 {cols[0].size}")
        depth = _nested_depth(c, leaves, name, f"column {i}")
        if depth > MAX_STACK_DEPTH:
            raise ValueError(f"{name}: column {i} is nested {depth} deep, "
                             f"the maximum depth is {MAX_STACK_DEPTH}")
    dev = cols[0].device
    assert dev.type == "cuda", "hash ops run on GPU columns"
    return cols, dev


def murmur3(table_or_cols, seed: int = DEFAULT_MURMUR3_SEED) -> Column:
    cols, dev = _cols(table_or_cols, _SPARK_LEAVES, "murmur3")
    g = _native.gpu()
    n = cols[0].size
    out = torch.empty(n, dtype=torch.int32, device=dev)
    desc, top, keep = pack_descriptors(cols)
    g.murmur3(desc.data_ptr(), top.data_ptr(), len(cols), n, seed,
              out.data_ptr(), _native.current_stream())
    return Column.from_torch(out)


def xxhash64(table_or_cols, seed: int = DEFAULT_XXHASH64_SEED) -> Column:
    cols, dev = _cols(table_or_cols, _SPARK_LEAVES, "xxhash64")
    g = _native.gpu()
    n = cols[0].size
    out = torch.empty(n, dtype=torch.int64, device=dev)
    desc, top, keep = pack_descriptors(cols)
    g.xxhash64(desc.data_ptr(), top.data_ptr(), len(cols), n, seed,
               out.data_ptr(), _native.current_stream())
    return Column.from_torch(out)


def hive_hash(table_or_cols) -> Column:
    cols, dev = _cols(table_or_cols, _HIVE_LEAVES, "hive_hash")
    g = _native.gpu()
    n = cols[0].size
    out = torch.empty(n, dtype=torch.int32, device=dev)
    desc, top, keep = pack_descriptors(cols)
    g.hive_hash(desc.data_ptr(), top.data_ptr(), len(cols), n,
                out.data_ptr(), _native.current_stream())
    return Column.from_torch(out)
