"""What ops/window.py and ops/segmented.py share: the code tables of
src/gpu/seg_scan.hpp, the result dtypes, the checks of one function's
`values` / `valid` and the packing of the kernels' function descriptors.
"""
import torch

# mirrors of src/gpu/seg_scan.hpp
MAX_FUNCS = 8
SMALL_ROWS = 2048
TILE_ROWS = 2048
CARRY_CHUNK = 1024  # tile carries per round of the carry scan

# mirrors of src/gpu/window_rolling.hpp
ROLL_TILE_ROWS = 1024  # sorted positions a workgroup of the rolling kernel owns
ROLL_MAX_REACH = 512   # widest |lo|, |hi| the staged path takes
ROLL_MAX_OFFSET = 2 ** 31 - 1
_FN_SHIFT = 8          # lag and lead

_RANKING = ("row_number", "rank", "dense_rank")
_AGGREGATES = ("count", "sum", "min", "max", "avg")
_SHIFTS = ("lag", "lead")
_FUNCS = {fn: i for i, fn in enumerate(_RANKING + _AGGREGATES)}
_CODES = dict(_FUNCS, lag=_FN_SHIFT, lead=_FN_SHIFT)
_FRAMES = {"partition": 0, "rows": 1, "range": 2}
_K_NONE, _K_BOOL, _K_SINT, _K_F32, _K_F64 = range(5)
_VALUE_KINDS = {
    torch.bool: _K_BOOL, torch.int8: _K_SINT, torch.int16: _K_SINT,
    torch.int32: _K_SINT, torch.int64: _K_SINT, torch.float32: _K_F32,
    torch.float64: _K_F64,
}
_BYTE_DTYPES = (torch.bool, torch.uint8, torch.int8)


class _Func:
    """One checked function; `frame` is the window's alone."""
    __slots__ = ("fn", "values", "valid", "frame")

    def __init__(self, fn, values, valid, frame="partition"):
        self.fn, self.values, self.valid, self.frame = fn, values, valid, frame

    def out_dtype(self):
        if self.fn in _RANKING or self.fn == "count":
            return torch.int64
        if self.fn == "avg":
            return torch.float64
        if self.fn == "sum":
            return (torch.float64 if self.values.dtype.is_floating_point
                    else torch.int64)
        return self.values.dtype

    def nullable(self):
        return (self.fn not in _RANKING and self.fn != "count"
                and self.valid is not None)


class _RollFunc(_Func):
    """One checked function of the rolling kernel: an aggregate over the
    bounded frame [i + lo, i + hi], or lag / lead as the value `shift`
    sorted positions away (lo = hi = shift)."""
    __slots__ = ("lo", "hi", "shift")

    def __init__(self, fn, values, valid, lo, hi, shift=0):
        super().__init__(fn, values, valid, "rows")
        self.lo, self.hi, self.shift = lo, hi, shift

    def out_dtype(self):
        if self.fn in _SHIFTS:
            return self.values.dtype
        return super().out_dtype()

    def nullable(self):
        if self.fn in _SHIFTS:
            return True
        if self.fn == "count":
            return False
        # a frame that leaves the current row out can be empty
        return self.valid is not None or self.lo > 0 or self.hi < 0


def _check_values(i, fn, values, valid, m, dev, anchor):
    """Checks `values` and `valid` of aggregate funcs[i] against the m rows
    and the device of the tensor called `anchor`; returns `valid` contiguous."""
    if values is None:
        if fn != "count":
            raise ValueError(f"funcs[{i}]: {fn} needs values")
    else:
        if not isinstance(values, torch.Tensor):
            raise TypeError(f"funcs[{i}]: values must be a torch.Tensor")
        if values.dtype not in _VALUE_KINDS:
            raise TypeError(f"funcs[{i}]: unsupported dtype "
                            f"{values.dtype}")
        if values.dim() != 1:
            raise ValueError(f"funcs[{i}]: values must be 1-D, got shape "
                             f"{tuple(values.shape)}")
        if values.numel() != m:
            raise ValueError(f"funcs[{i}]: values has {values.numel()} "
                             f"rows but {anchor} has {m}")
        if values.device != dev:
            raise ValueError(f"funcs[{i}]: values and {anchor} are on "
                             "different devices")
    if valid is not None:
        if not isinstance(valid, torch.Tensor) or \
                valid.dtype not in _BYTE_DTYPES:
            raise TypeError(f"funcs[{i}]: valid must be a bool, uint8 or "
                            "int8 tensor")
        if valid.dim() != 1 or valid.numel() != m:
            raise ValueError(f"funcs[{i}]: valid must be 1-D with {m} "
                             "rows")
        if valid.device != dev:
            raise ValueError(f"funcs[{i}]: valid and {anchor} are on "
                             "different devices")
        valid = valid.contiguous()
    return valid


def _outputs(f: _Func, n, dev):
    """Uninitialised `(data, valid or None)` of n rows for f."""
    return (torch.empty(n, dtype=f.out_dtype(), device=dev),
            torch.empty(n, dtype=torch.bool, device=dev)
            if f.nullable() else None)


def _descriptor(f: _Func, m, data, ov):
    """The tuple the bindings take for f over m rows, with outputs `data`
    and `ov` (or None)."""
    if f.values is None:
        kind, width, stride, vptr = _K_NONE, 1, 1, 0
    else:
        kind = _VALUE_KINDS[f.values.dtype]
        width = f.values.element_size()
        stride = f.values.stride(0) if m > 1 else 1
        if stride < 1:
            f.values = f.values.contiguous()
            stride = 1
        vptr = f.values.data_ptr()
    return (_CODES[f.fn], _FRAMES[f.frame], kind, width,
            stride, vptr, f.valid.data_ptr() if f.valid is not None else 0,
            data.data_ptr(), ov.data_ptr() if ov is not None else 0)


def _roll_descriptor(f: _RollFunc, m, data, ov):
    """The tuple the rolling binding takes for f."""
    return (_descriptor(f, m, data, ov), f.lo, f.hi, f.shift)


def _work_buffer(nbytes, dev):
    """The kernels' scratch (None on the one-workgroup path)."""
    return (torch.empty(nbytes // 8, dtype=torch.int64, device=dev)
            if nbytes else None)
