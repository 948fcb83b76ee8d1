"""Fused expression evaluation (cudf's compute_column for the reference's
project and filter execs): a typed, null-aware expression program evaluated
over the rows of a frame in ONE launch of the kernel of src/gpu/expr.hip.

A `Program` is a postfix list of instructions over a stack. The builder
types every instruction statically, as torch would type the same tensor
expression: two-operand arithmetic and the comparisons work in
`torch.promote_types` of their operands, `div` is float64, `and_`/`or_`/`not_`
and the comparisons give bool. Each value also carries, statically, whether
it can be null; an output gets a validity tensor exactly when it can.

Semantics (Spark, non-ANSI; the rules of the NDS torch evaluator):
  * data and validity are independent. Data operations ignore validity: the
    data under a null is what the same arithmetic gives on the bytes stored
    there. Validity of arithmetic and comparisons is the AND of the operands'.
  * integers wrap at the width of the result dtype; float32 results are
    rounded to float32 after every operation.
  * `div`: float64; a zero divisor is replaced by 1 and the result is null.
  * `and_` / `or_`: Kleene. valid = (lv & rv) | (lv & ~l) | (rv & ~r) for AND,
    (lv & rv) | (lv & l) | (rv & r) for OR; the data of AND is masked by its
    validity, the data of OR is not.
  * `in_set`: membership in a constant integer set; `lut`: table[value] of a
    constant int64 table (an index outside the table is clamped to it).
  * `select`: [running, value, cond] -> cond true and valid ? value : running,
    data and validity alike; `coalesce_step`: [running, next] -> running where
    it is valid, else next; valid where either is.
  * a float to integer cast of a value outside the integer's range is
    undefined, as in torch.
  * `store` pops into a new output; `store_keep` pops into a bool output that
    is true where the value is true and valid (what a filter keeps). A
    program may store several outputs.

Limits (mirrors of src/gpu/expr.hpp, checked by the builder and again by the
binding): MAX_INSTRS instructions, a stack of MAX_DEPTH, MAX_INPUTS input
columns, MAX_OUTPUTS outputs and MAX_CONSTS constant arrays per program.

CPU tensors take a torch twin that interprets the same program one
instruction at a time; it is the op's specification. CUDA tensors always take
the native kernel: the program travels in the kernel arguments, so there is no
copy, no host sync (the op runs under stream capture), no atomics, no
temporaries, and the same input gives bit-identical output on every run.
"""
import struct
from typing import List, Optional, Sequence, Tuple

import torch

from .. import _native

# mirrors of src/gpu/expr.hpp
MAX_INSTRS = 160
MAX_DEPTH = 16
MAX_INPUTS = 24
MAX_OUTPUTS = 8
MAX_CONSTS = 16
ROWS_PER_THREAD = 2
MAX_GRID = 2048
BLOCK = 256

BOOL, I8, I16, I32, I64, F32, F64 = range(7)
KIND_DTYPES = (torch.bool, torch.int8, torch.int16, torch.int32, torch.int64,
               torch.float32, torch.float64)
_KIND_OF = {dt: k for k, dt in enumerate(KIND_DTYPES)}

(LOAD_COL, LIT, ADD, SUB, MUL, DIV, EQ, NE, LT, LE, GT, GE, AND, OR, NOT,
 IS_NULL, IS_NOT_NULL, ABS, CAST, IN_SET, LUT, SELECT, COALESCE_STEP, STORE,
 STORE_KEEP) = range(25)
_CMP_OPS = {"==": EQ, "!=": NE, "<": LT, "<=": LE, ">": GT, ">=": GE}
_CMP_FN = {EQ: torch.eq, NE: torch.ne, LT: torch.lt, LE: torch.le,
           GT: torch.gt, GE: torch.ge}
_INSTR = struct.Struct("<BBHIq")
_F64 = struct.Struct("<d")
_I64 = struct.Struct("<q")


class ProgramError(ValueError):
    """A program the builder refuses: a type it cannot give, an operand that
    is missing, or a limit exceeded."""


def kind_of(dtype) -> int:
    try:
        return _KIND_OF[dtype]
    except KeyError:
        raise ProgramError(f"unsupported dtype {dtype}") from None


def _is_float(k):
    return k >= F32


def promote(ka: int, kb: int) -> int:
    return _KIND_OF[torch.promote_types(KIND_DTYPES[ka], KIND_DTYPES[kb])]


def _wrap_int(kind, v):
    if kind == BOOL:
        return int(v != 0)
    bits = (8, 16, 32, 64)[kind - I8]
    v &= (1 << bits) - 1
    return v - (1 << bits) if v >> (bits - 1) else v


class Program:
    """Builder of an expression program. `add_input` declares a column;
    every other method appends one instruction and updates the static stack
    of (kind, nullable)."""

    def __init__(self):
        self.instrs: List[Tuple[int, int, int, int]] = []
        self.inputs: List[Tuple[int, bool]] = []      # (kind, nullable)
        self.outputs: List[Tuple[int, bool, bool]] = []  # (kind, nullable, keep)
        self.consts: List[Tuple[int, ...]] = []
        self.stack: List[Tuple[int, bool]] = []
        self.depth = 0
        self._code = None
        self._const_tensors = {}

    # -- static state ------------------------------------------------------
    def add_input(self, dtype, nullable: bool) -> int:
        if len(self.inputs) >= MAX_INPUTS:
            raise ProgramError(f"more than {MAX_INPUTS} inputs")
        self.inputs.append((kind_of(dtype), bool(nullable)))
        return len(self.inputs) - 1

    @property
    def top_dtype(self):
        return KIND_DTYPES[self._peek(1)[0][0]]

    @property
    def top_nullable(self):
        return self._peek(1)[0][1]

    def _peek(self, n):
        if len(self.stack) < n:
            raise ProgramError(f"stack underflow: {n} operands needed, "
                               f"{len(self.stack)} on the stack")
        return self.stack[len(self.stack) - n:]

    def _emit(self, op, kind, arg, imm, pops, push):
        if len(self.instrs) >= MAX_INSTRS:
            raise ProgramError(f"more than {MAX_INSTRS} instructions")
        if pops:
            del self.stack[len(self.stack) - pops:]
        if push is not None:
            if len(self.stack) >= MAX_DEPTH:
                raise ProgramError(f"stack deeper than {MAX_DEPTH}")
            self.stack.append(push)
            self.depth = max(self.depth, len(self.stack))
        self.instrs.append((op, kind, arg, imm))
        self._code = None

    def _add_const(self, values) -> int:
        values = tuple(int(v) for v in values)
        for i, c in enumerate(self.consts):
            if c == values:
                return i
        if len(self.consts) >= MAX_CONSTS:
            raise ProgramError(f"more than {MAX_CONSTS} constant arrays")
        self.consts.append(values)
        return len(self.consts) - 1

    # -- instructions ------------------------------------------------------
    def load(self, index: int):
        if not 0 <= index < len(self.inputs):
            raise ProgramError(f"input {index} out of range")
        self._emit(LOAD_COL, self.inputs[index][0], index, 0, 0,
                   self.inputs[index])
        return self

    def lit(self, value, dtype=None):
        """A literal; `None` is a null (int64 zero unless `dtype` is given).
        Without `dtype`, bool -> bool, int -> int64, float -> float64."""
        if dtype is None:
            if isinstance(value, bool):
                dtype = torch.bool
            elif isinstance(value, int) or value is None:
                dtype = torch.int64
            elif isinstance(value, float):
                dtype = torch.float64
            else:
                raise ProgramError(f"unsupported literal {value!r}")
        kind = kind_of(dtype)
        null = value is None
        v = 0 if null else value
        if _is_float(kind):
            f = float(v)
            if kind == F32:
                f = struct.unpack("<f", struct.pack("<f", f))[0]
            imm = _I64.unpack(_F64.pack(f))[0]
        else:
            imm = _wrap_int(kind, int(v))
        self._emit(LIT, kind, int(null), imm, 0, (kind, null))
        return self

    def _binary(self, op, kind=None, nullable=None):
        (ka, na), (kb, nb) = self._peek(2)
        k = promote(ka, kb) if kind is None else kind
        return ka, kb, k, (na or nb) if nullable is None else nullable

    def _arith(self, op):
        ka, kb, k, n = self._binary(op)
        if op == SUB and k == BOOL:
            raise ProgramError("bool - bool is not defined")
        self._emit(op, k, ka | kb << 4, 0, 2, (k, n))
        return self

    def add(self): return self._arith(ADD)
    def sub(self): return self._arith(SUB)
    def mul(self): return self._arith(MUL)

    def div(self):
        ka, kb, _, _ = self._binary(DIV)
        self._emit(DIV, F64, ka | kb << 4, 0, 2, (F64, True))
        return self

    def cmp(self, op: str):
        if op not in _CMP_OPS:
            raise ProgramError(f"unknown comparison {op!r}")
        ka, kb, k, n = self._binary(op)
        self._emit(_CMP_OPS[op], k, ka | kb << 4, 0, 2, (BOOL, n))
        return self

    def and_(self):
        ka, kb, _, n = self._binary(AND)
        self._emit(AND, BOOL, ka | kb << 4, 0, 2, (BOOL, n))
        return self

    def or_(self):
        ka, kb, _, n = self._binary(OR)
        self._emit(OR, BOOL, ka | kb << 4, 0, 2, (BOOL, n))
        return self

    def not_(self):
        (k, n), = self._peek(1)
        self._emit(NOT, BOOL, k, 0, 1, (BOOL, n))
        return self

    def is_null(self, negate=False):
        self._peek(1)
        self._emit(IS_NOT_NULL if negate else IS_NULL, BOOL, 0, 0, 1,
                   (BOOL, False))
        return self

    def abs(self):
        (k, n), = self._peek(1)
        if k == BOOL:
            raise ProgramError("abs of bool is not defined")
        self._emit(ABS, k, k, 0, 1, (k, n))
        return self

    def cast(self, dtype):
        """Tensor.to(dtype). A cast that cannot change the slot (the same
        kind, a wider integer, float32 to float64) only retypes the value."""
        (k, n), = self._peek(1)
        to = kind_of(dtype)
        if to == k:
            return self
        widening = (to >= k and not _is_float(k) and not _is_float(to)) or \
            (k == F32 and to == F64)
        if widening:
            self.stack[-1] = (to, n)
            return self
        self._emit(CAST, to, k, 0, 1, (to, n))
        return self

    def in_set(self, values: Sequence[int]):
        (k, n), = self._peek(1)
        if _is_float(k):
            raise ProgramError("in_set needs an integer operand")
        c = self._add_const(sorted(set(int(v) for v in values)))
        self._emit(IN_SET, BOOL, k, c, 1, (BOOL, n))
        return self

    def lut(self, table: Sequence[int], dtype=torch.int64):
        (k, n), = self._peek(1)
        to = kind_of(dtype)
        if _is_float(k) or _is_float(to):
            raise ProgramError("lut needs an integer operand and result")
        if len(table) < 1:
            raise ProgramError("lut needs a table of at least one entry")
        c = self._add_const(table)
        self._emit(LUT, to, k, c, 1, (to, n))
        return self

    def select(self):
        """[running, value, cond] -> cond ? value : running."""
        (kr, _), (kv, _), (kc, _) = self._peek(3)
        if kr != kv:
            raise ProgramError("select: value and running result differ in "
                               "dtype; cast them first")
        self._emit(SELECT, kr, kc, 0, 3, (kr, True))
        return self

    def coalesce_step(self):
        """[running, next] -> running where valid, else next."""
        ka, kb, k, _ = self._binary(COALESCE_STEP)
        self._emit(COALESCE_STEP, k, ka | kb << 4, 0, 2, (k, True))
        return self

    def store(self) -> int:
        (k, n), = self._peek(1)
        return self._store(STORE, k, (k, n, False))

    def store_keep(self) -> int:
        (k, _), = self._peek(1)
        return self._store(STORE_KEEP, k, (BOOL, False, True))

    def _store(self, op, kind, out):
        if len(self.outputs) >= MAX_OUTPUTS:
            raise ProgramError(f"more than {MAX_OUTPUTS} outputs")
        self._emit(op, kind, len(self.outputs), 0, 1, None)
        self.outputs.append(out)
        return len(self.outputs) - 1

    # -- packed forms ------------------------------------------------------
    def code(self) -> bytes:
        if self._code is None:
            self._code = b"".join(_INSTR.pack(op, kind, arg, 0, imm)
                                  for op, kind, arg, imm in self.instrs)
        return self._code

    def const_tensors(self, device) -> List[torch.Tensor]:
        """The constant arrays as int64 tensors on `device`, uploaded once
        per device and value tuple."""
        out = []
        for c in self.consts:
            out.append(_const_tensor(c, device))
        return out

    def check_complete(self):
        if self.stack:
            raise ProgramError(f"{len(self.stack)} values left on the stack")
        if not self.outputs:
            raise ProgramError("the program stores no output")


_CONST_CACHE = {}
_CONST_CACHE_MAX = 4096


def _const_tensor(values: Tuple[int, ...], device) -> torch.Tensor:
    key = (values, str(device))
    t = _CONST_CACHE.get(key)
    if t is None:
        if len(_CONST_CACHE) >= _CONST_CACHE_MAX:
            _CONST_CACHE.clear()
        t = torch.tensor(values, dtype=torch.int64, device=device)
        _CONST_CACHE[key] = t
    return t


# ---------------------------------------------------------------------------
# CPU twin
# ---------------------------------------------------------------------------

def _mask(v, n, dev):
    return v if v is not None else torch.ones(n, dtype=torch.bool, device=dev)


def _and_valid(a, b):
    if a is None:
        return b
    if b is None:
        return a
    return a & b


def _fresh(t, cols):
    """An output never aliases an input."""
    for d, v in cols:
        if t is d or t is v:
            return t.clone()
    return t


def _eval_cpu(p: Program, cols, n, dev):
    """Interprets the program with torch ops, one instruction at a time. A
    stack entry is (data of the kind's dtype, bool validity or None)."""
    st = []
    outs = [None] * len(p.outputs)
    for op, kind, arg, imm in p.instrs:
        dt = KIND_DTYPES[kind]
        if op == LOAD_COL:
            st.append(cols[arg])
        elif op == LIT:
            if _is_float(kind):
                v = _F64.unpack(_I64.pack(imm))[0]
            else:
                v = bool(imm) if kind == BOOL else imm
            data = torch.full((n,), v, dtype=dt, device=dev)
            st.append((data, torch.zeros(n, dtype=torch.bool, device=dev)
                       if arg else None))
        elif op in (ADD, SUB, MUL):
            (b, bv), (a, av) = st.pop(), st.pop()
            a, b = a.to(dt), b.to(dt)
            data = a + b if op == ADD else a - b if op == SUB else a * b
            st.append((data, _and_valid(av, bv)))
        elif op == DIV:
            (b, bv), (a, av) = st.pop(), st.pop()
            a, b = a.to(torch.float64), b.to(torch.float64)
            zero = b == 0
            data = a / torch.where(zero, torch.ones_like(b), b)
            st.append((data, _and_valid(_and_valid(~zero, av), bv)))
        elif op in _CMP_FN:
            (b, bv), (a, av) = st.pop(), st.pop()
            st.append((_CMP_FN[op](a.to(dt), b.to(dt)), _and_valid(av, bv)))
        elif op in (AND, OR):
            (b, bv), (a, av) = st.pop(), st.pop()
            a, b = a.bool(), b.bool()
            if av is None and bv is None:
                st.append((a & b if op == AND else a | b, None))
                continue
            av, bv = _mask(av, n, dev), _mask(bv, n, dev)
            if op == AND:
                valid = (av & bv) | (av & ~a) | (bv & ~b)
                st.append((a & b & valid, valid))
            else:
                valid = (av & bv) | (av & a) | (bv & b)
                st.append((a | b, valid))
        elif op == NOT:
            a, av = st.pop()
            st.append((~a.bool(), av))
        elif op in (IS_NULL, IS_NOT_NULL):
            a, av = st.pop()
            m = _mask(av, n, dev)
            st.append((m if op == IS_NOT_NULL else ~m, None))
        elif op == ABS:
            a, av = st.pop()
            st.append((a.to(dt).abs(), av))
        elif op == CAST:
            a, av = st.pop()
            st.append((a.to(dt), av))
        elif op == IN_SET:
            a, av = st.pop()
            members = p.consts[imm]
            if members:
                t = torch.tensor(members, dtype=torch.int64, device=dev)
                data = torch.isin(a.to(torch.int64), t)
            else:
                data = torch.zeros(n, dtype=torch.bool, device=dev)
            st.append((data, av))
        elif op == LUT:
            a, av = st.pop()
            table = torch.tensor(p.consts[imm], dtype=torch.int64, device=dev)
            idx = a.to(torch.int64).clamp(0, len(p.consts[imm]) - 1)
            st.append((table[idx].to(dt), av))
        elif op == SELECT:
            (c, cv), (v, vv), (r, rv) = st.pop(), st.pop(), st.pop()
            hit = c.bool() & _mask(cv, n, dev)
            st.append((torch.where(hit, v.to(dt), r.to(dt)),
                       torch.where(hit, _mask(vv, n, dev),
                                   _mask(rv, n, dev))))
        elif op == COALESCE_STEP:
            (b, bv), (a, av) = st.pop(), st.pop()
            av, bv = _mask(av, n, dev), _mask(bv, n, dev)
            st.append((torch.where(av, a.to(dt), b.to(dt)), av | bv))
        elif op == STORE:
            a, av = st.pop()
            nullable = p.outputs[arg][1]
            outs[arg] = (_fresh(a.to(dt), cols),
                         _fresh(_mask(av, n, dev), cols) if nullable
                         else None)
        elif op == STORE_KEEP:
            a, av = st.pop()
            keep = a.bool()
            if av is not None:
                keep = keep & av
            outs[arg] = (_fresh(keep, cols), None)
        else:
            raise ProgramError(f"unknown op {op}")
    return outs


# ---------------------------------------------------------------------------
# public entry
# ---------------------------------------------------------------------------

_BYTE_DTYPES = (torch.bool, torch.uint8, torch.int8)


def _check_columns(p: Program, columns, nrows):
    if len(columns) != len(p.inputs):
        raise ValueError(f"the program declares {len(p.inputs)} inputs but "
                         f"{len(columns)} columns were given")
    cols = []
    dev = None
    for i, (c, (kind, nullable)) in enumerate(zip(columns, p.inputs)):
        data, valid = c if isinstance(c, (tuple, list)) else (c, None)
        if not isinstance(data, torch.Tensor):
            raise TypeError(f"columns[{i}]: data must be a torch.Tensor")
        if data.dtype != KIND_DTYPES[kind]:
            raise TypeError(f"columns[{i}]: declared {KIND_DTYPES[kind]}, "
                            f"got {data.dtype}")
        if data.dim() != 1 or data.numel() != nrows:
            raise ValueError(f"columns[{i}]: data must be 1-D with {nrows} "
                             "rows")
        if dev is None:
            dev = data.device
        elif data.device != dev:
            raise ValueError(f"columns[{i}] is on another device")
        if nullable != (valid is not None):
            raise ValueError(f"columns[{i}]: declared "
                             f"{'nullable' if nullable else 'not nullable'}")
        if valid is not None:
            if not isinstance(valid, torch.Tensor) or \
                    valid.dtype not in _BYTE_DTYPES:
                raise TypeError(f"columns[{i}]: valid must be a bool, uint8 "
                                "or int8 tensor")
            if valid.dim() != 1 or valid.numel() != nrows:
                raise ValueError(f"columns[{i}]: valid must be 1-D with "
                                 f"{nrows} rows")
            if valid.device != dev:
                raise ValueError(f"columns[{i}]: valid is on another device")
            valid = valid.contiguous()
        cols.append((data.contiguous(), valid))
    return cols, dev


def eval_program(program: Program, columns, nrows: int, device=None
                 ) -> List[Tuple[torch.Tensor, Optional[torch.Tensor]]]:
    """Evaluates `program` over `columns` (one `(data, valid or None)` or a
    bare tensor per declared input, each with `nrows` rows). Returns one
    `(data, valid)` per output in store order: `data` has the dtype the
    builder gave the output, `valid` is a bool tensor where the output can
    be null and None where it cannot. `device` is needed only by a program
    without inputs."""
    if nrows < 0:
        raise ValueError("nrows < 0")
    program.check_complete()
    cols, dev = _check_columns(program, columns, nrows)
    if dev is None:
        if device is None:
            raise ValueError("a program without inputs needs a device")
        dev = torch.device(device)
    if nrows == 0:
        return [(torch.empty(0, dtype=KIND_DTYPES[k], device=dev),
                 torch.empty(0, dtype=torch.bool, device=dev) if nl else None)
                for k, nl, _ in program.outputs]
    if dev.type != "cuda":
        cols = [(d, v != 0 if v is not None and v.dtype != torch.bool else v)
                for d, v in cols]
        return _eval_cpu(program, cols, nrows, dev)
    return _eval_gpu(program, cols, nrows, dev)


def _eval_gpu(p: Program, cols, n, dev):
    g = _native.gpu()
    consts = p.const_tensors(dev)
    outs = []
    descs = []
    for kind, nullable, _keep in p.outputs:
        data = torch.empty(n, dtype=KIND_DTYPES[kind], device=dev)
        valid = torch.empty(n, dtype=torch.bool, device=dev) \
            if nullable else None
        outs.append((data, valid))
        descs.append((data.data_ptr(),
                      valid.data_ptr() if valid is not None else 0))
    g.expr_eval(p.code(),
                [(d.data_ptr(), v.data_ptr() if v is not None else 0, k)
                 for (d, v), (k, _) in zip(cols, p.inputs)],
                descs,
                [(t.data_ptr() if len(c) else 0, len(c))
                 for t, c in zip(consts, p.consts)],
                n, _native.current_stream())
    return outs
