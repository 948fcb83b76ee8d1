"""Stream compaction and fused multi-column gather (cudf apply_boolean_mask /
copy_if / multi-column gather), on the HIP kernels of src/gpu/compact.hip.

Two properties are design requirements, not tuning choices:

* **Stable order.** Kept rows come out in input order. Spark filter
  semantics and the sort/limit determinism tests rely on it, so selection is
  a deterministic two-pass count / scan / scatter with no atomics.
* **No spins.** The scan over tile counts is a single workgroup with a
  running carry. No kernel here waits on another workgroup (no decoupled
  look-back, no inter-workgroup flags), so none can hang on residency.

`mask` and `valid` are byte-per-row tensors (`bool`, `uint8` or `int8`; any
non-zero byte is true). A row is kept when `mask[i] != 0` and, if `valid` is
given, `valid[i] != 0`.

Rows of `compact_tensors` / `gather_tensors` inputs are 1, 2, 4, 8 or 16
bytes wide. A tensor is either 1-D (row = element; `complex128` is the
16-byte dtype) or 2-D contiguous `(n, w)` (row = `w` elements), which is how
the project's DECIMAL128 layout is passed: `data.view(n, 2)` of the int64
pair buffer. Outputs keep the input dtype and trailing shape.

CPU tensors take the equivalent torch expressions (the NDS CPU oracle and the
gloo tests run on them); CUDA tensors always take the native kernels.
"""
from typing import List, Optional, Sequence, Tuple, Union

import torch

from .. import _native
from ..columnar import Column, DType, Table, validity_to_bool

_BYTE_DTYPES = (torch.bool, torch.uint8, torch.int8)
_ROW_WIDTHS = (1, 2, 4, 8, 16)


def _byte_rows(t: torch.Tensor, what: str) -> torch.Tensor:
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{what} must be a torch.Tensor")
    if t.dtype not in _BYTE_DTYPES:
        raise TypeError(f"{what} must be bool, uint8 or int8, got {t.dtype}")
    if t.dim() != 1:
        raise ValueError(f"{what} must be 1-D, got shape {tuple(t.shape)}")
    return t.contiguous()


def _check_mask(mask, valid):
    mask = _byte_rows(mask, "mask")
    if valid is not None:
        valid = _byte_rows(valid, "valid")
        if valid.numel() != mask.numel():
            raise ValueError(
                f"mask has {mask.numel()} rows but valid has {valid.numel()}")
        if valid.device != mask.device:
            raise ValueError("mask and valid are on different devices")
    return mask, valid


def _keep_cpu(mask, valid):
    keep = mask != 0
    if valid is not None:
        keep = keep & (valid != 0)
    return keep


def _no_capture(what: str):
    if torch.cuda.is_current_stream_capturing():
        raise RuntimeError(
            f"{what} reads the kept-row count back to the host and cannot "
            "run under stream capture; compute the selection outside the "
            "graph and use gather_tensors inside it")


def _row_width(t: torch.Tensor, n: int, what: str) -> int:
    if t.dim() not in (1, 2) or t.shape[0] != n:
        raise ValueError(
            f"{what} must be 1-D of length {n} or 2-D ({n}, w), got shape "
            f"{tuple(t.shape)}")
    w = t.element_size() * (t.shape[1] if t.dim() == 2 else 1)
    if w not in _ROW_WIDTHS:
        raise ValueError(f"{what} has {w}-byte rows; supported: 1, 2, 4, 8, 16")
    return w


def _offsets(g, mask, valid, n, stream):
    """Count + scan. Returns (offsets tensor, k). One host sync (.item())."""
    ntiles = (n + g.compact_tile_rows() - 1) // g.compact_tile_rows()
    # one allocation: int64 offsets[ntiles], int64 total, int32 counts[ntiles]
    buf = torch.empty(ntiles + 1 + (ntiles + 1) // 2, dtype=torch.int64,
                      device=mask.device)
    base = buf.data_ptr()
    g.compact_offsets(mask.data_ptr(),
                      valid.data_ptr() if valid is not None else 0, n,
                      base + 8 * (ntiles + 1), base, base + 8 * ntiles, stream)
    return buf, int(buf[ntiles].item())


def nonzero(mask: torch.Tensor,
            valid: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Ascending int64 indices of the kept rows."""
    mask, valid = _check_mask(mask, valid)
    if not mask.is_cuda:
        return torch.nonzero(_keep_cpu(mask, valid), as_tuple=False).view(-1)
    _no_capture("nonzero")
    n = mask.numel()
    if n == 0:
        return torch.empty(0, dtype=torch.int64, device=mask.device)
    g = _native.gpu()
    stream = _native.current_stream()
    offs, k = _offsets(g, mask, valid, n, stream)
    out = torch.empty(k, dtype=torch.int64, device=mask.device)
    if k:
        g.compact_nonzero(mask.data_ptr(),
                          valid.data_ptr() if valid is not None else 0,
                          n, offs.data_ptr(), out.data_ptr(), stream)
    return out


def _launch_cols(launch, srcs, outs, widths, max_cols):
    for lo in range(0, len(srcs), max_cols):
        hi = lo + max_cols
        launch([t.data_ptr() for t in srcs[lo:hi]],
               [t.data_ptr() for t in outs[lo:hi]], widths[lo:hi])


def compact_tensors(tensors: Sequence[torch.Tensor], mask: torch.Tensor,
                    valid: Optional[torch.Tensor] = None
                    ) -> Tuple[List[torch.Tensor], int]:
    """Keep the selected rows of every tensor: `([t[keep] ...], k)`.

    One count + scan serves all tensors; the copies are fused, up to
    `compact_max_cols()` tensors per launch, and never build an index array.
    """
    mask, valid = _check_mask(mask, valid)
    n = mask.numel()
    tensors = list(tensors)
    widths = [_row_width(t, n, f"tensors[{i}]") for i, t in enumerate(tensors)]
    for t in tensors:
        if t.device != mask.device:
            raise ValueError("tensors and mask are on different devices")
    if not mask.is_cuda:
        idx = torch.nonzero(_keep_cpu(mask, valid), as_tuple=False).view(-1)
        return [t[idx] for t in tensors], idx.numel()
    _no_capture("compact_tensors")
    dev = mask.device
    if n == 0:
        return [torch.empty_like(t) for t in tensors], 0
    g = _native.gpu()
    stream = _native.current_stream()
    offs, k = _offsets(g, mask, valid, n, stream)
    outs = [torch.empty((k,) + tuple(t.shape[1:]), dtype=t.dtype, device=dev)
            for t in tensors]
    if k and tensors:
        srcs = [t.contiguous() for t in tensors]
        mp = mask.data_ptr()
        vp = valid.data_ptr() if valid is not None else 0
        op = offs.data_ptr()
        _launch_cols(
            lambda s, d, w: g.compact_cols(mp, vp, n, op, s, d, w, stream),
            srcs, outs, widths, g.compact_max_cols())
    return outs, k


def gather_tensors(tensors: Sequence[torch.Tensor],
                   idx: torch.Tensor) -> List[torch.Tensor]:
    """`[t[idx] ...]` for tensors that share their row count `n`.

    Precondition: `0 <= idx < n`. An entry outside that range is never
    dereferenced on the GPU; its output row is zero. That is documented
    behaviour, not error reporting. No host sync: works under stream capture.
    """
    if not isinstance(idx, torch.Tensor) or idx.dtype != torch.int64:
        raise TypeError("idx must be an int64 tensor")
    if idx.dim() != 1:
        raise ValueError(f"idx must be 1-D, got shape {tuple(idx.shape)}")
    tensors = list(tensors)
    if not tensors:
        return []
    n = tensors[0].shape[0] if tensors[0].dim() else -1
    widths = [_row_width(t, n, f"tensors[{i}]") for i, t in enumerate(tensors)]
    for t in tensors:
        if t.device != idx.device:
            raise ValueError("tensors and idx are on different devices")
    if not idx.is_cuda:
        return [t[idx] for t in tensors]
    m = idx.numel()
    dev = idx.device
    outs = [torch.empty((m,) + tuple(t.shape[1:]), dtype=t.dtype, device=dev)
            for t in tensors]
    if m == 0:
        return outs
    g = _native.gpu()
    idx = idx.contiguous()
    stream = _native.current_stream()
    srcs = [t.contiguous() for t in tensors]
    ip = idx.data_ptr()
    _launch_cols(lambda s, d, w: g.gather_cols(ip, m, n, s, d, w, stream),
                 srcs, outs, widths, g.compact_max_cols())
    return outs


def apply_boolean_mask(table: Table,
                       mask: Union[torch.Tensor, Column]) -> Table:
    """Keep the rows of `table` where `mask` is true (Spark Filter).

    `mask` is a byte tensor or a BOOL8 Column; a null mask row (validity bit
    clear) drops the row. Implemented as `nonzero` + the table gather, so
    strings, lists, structs and packed validity ride the existing kernels.
    """
    from .copying import gather
    valid = None
    if isinstance(mask, Column):
        if mask.dtype != DType.BOOL8:
            raise TypeError(f"mask column must be BOOL8, got {mask.dtype!r}")
        if mask.validity is not None:
            valid = validity_to_bool(mask.validity, mask.size)
        mask = mask.data
    if mask.numel() != table.num_rows:
        raise ValueError(f"mask has {mask.numel()} rows but the table has "
                         f"{table.num_rows}")
    return gather(table, nonzero(mask, valid))
