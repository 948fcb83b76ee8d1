"""Expression IR + torch evaluator for the NDS plan engine.

Spark SQL null semantics (the ones the reference's kernels implement):
arithmetic/comparison propagate null; AND/OR are three-valued Kleene;
Filter keeps rows whose predicate is TRUE (null -> dropped).

String dimension attributes are dictionary-encoded at generation time
(codes in the column, the dictionary in the table metadata), so string
predicates (=, IN, LIKE, substr) evaluate against the dictionary on host
and become integer-code predicates on device — a deliberate MI355X-first
design: the scan stays numeric and HBM-bandwidth-bound.
"""
import datetime
from typing import List, Optional, Sequence

import torch


class Val:
    """An evaluated expression: data tensor + optional validity (bool, True =
    valid) + optional string dictionary (data holds codes)."""
    __slots__ = ("data", "valid", "dict", "_all_true")

    def __init__(self, data, valid=None, dict=None):
        self.data = data
        self.valid = valid
        self.dict = dict
        self._all_true = None  # memo: valid mask known all-true (1 sync max)

    def valid_mask(self):
        if self.valid is None:
            return torch.ones_like(self.data, dtype=torch.bool)
        return self.valid


class Expr:
    def __add__(self, o): return BinOp("+", self, _wrap(o))
    def __radd__(self, o): return BinOp("+", _wrap(o), self)
    def __sub__(self, o): return BinOp("-", self, _wrap(o))
    def __rsub__(self, o): return BinOp("-", _wrap(o), self)
    def __mul__(self, o): return BinOp("*", self, _wrap(o))
    def __rmul__(self, o): return BinOp("*", _wrap(o), self)
    def __truediv__(self, o): return BinOp("/", self, _wrap(o))
    def __rtruediv__(self, o): return BinOp("/", _wrap(o), self)
    def __gt__(self, o): return BinOp(">", self, _wrap(o))
    def __ge__(self, o): return BinOp(">=", self, _wrap(o))
    def __lt__(self, o): return BinOp("<", self, _wrap(o))
    def __le__(self, o): return BinOp("<=", self, _wrap(o))
    def __eq__(self, o): return BinOp("==", self, _wrap(o))
    def __ne__(self, o): return BinOp("!=", self, _wrap(o))
    def __and__(self, o): return BinOp("and", self, _wrap(o))
    def __or__(self, o): return BinOp("or", self, _wrap(o))
    def __invert__(self): return Not(self)
    def __neg__(self): return BinOp("-", Lit(0), self)
    def __hash__(self): return id(self)

    def isin(self, values): return InList(self, list(values))
    def between(self, lo, hi):
        return BinOp("and", BinOp(">=", self, _wrap(lo)),
                     BinOp("<=", self, _wrap(hi)))
    def like(self, pattern): return Like(self, pattern)
    def substr(self, start, length): return Substr(self, start, length)
    def cast_float(self): return Cast(self, "float")
    def cast_int(self): return Cast(self, "int")


def _wrap(v):
    return v if isinstance(v, Expr) else Lit(v)


class Col(Expr):
    def __init__(self, name: str):
        self.name = name

    def __repr__(self):
        return f"col({self.name})"


class Lit(Expr):
    def __init__(self, value):
        self.value = value

    def __repr__(self):
        return f"lit({self.value!r})"


class BinOp(Expr):
    def __init__(self, op, l, r):
        self.op, self.l, self.r = op, l, r


class Not(Expr):
    def __init__(self, e):
        self.e = e


class IsNull(Expr):
    def __init__(self, e, negate=False):
        self.e, self.negate = e, negate


class InList(Expr):
    def __init__(self, e, values):
        self.e, self.values = e, values


class Like(Expr):
    def __init__(self, e, pattern):
        self.e, self.pattern = e, pattern


class Substr(Expr):
    def __init__(self, e, start, length):
        self.e, self.start, self.length = e, start, length


class Cast(Expr):
    def __init__(self, e, to):
        self.e, self.to = e, to


class CaseWhen(Expr):
    def __init__(self, branches, otherwise):
        self.branches = [(c, _wrap(v)) for c, v in branches]
        self.otherwise = _wrap(otherwise) if otherwise is not None else None


class Coalesce(Expr):
    def __init__(self, exprs):
        self.exprs = [_wrap(e) for e in exprs]


class Abs(Expr):
    def __init__(self, e):
        self.e = _wrap(e)


def abs_(e) -> Abs:
    return Abs(e)


def col(name: str) -> Col:
    return Col(name)


def lit(v) -> Lit:
    return Lit(v)


_EPOCH = datetime.date(1970, 1, 1)


def date_lit(s: str) -> Lit:
    """Date literal as days since epoch (d_date columns use this encoding)."""
    y, m, d = map(int, s.split("-"))
    return Lit((datetime.date(y, m, d) - _EPOCH).days)


def case_when(*branches, otherwise=None) -> CaseWhen:
    """case_when((cond, value), ..., otherwise=value)"""
    return CaseWhen(list(branches), otherwise)


def coalesce(*exprs) -> Coalesce:
    return Coalesce(list(exprs))


def is_null(e) -> IsNull:
    return IsNull(_wrap(e))


def is_not_null(e) -> IsNull:
    return IsNull(_wrap(e), negate=True)


# ---------------------------------------------------------------------------
# evaluation
# ---------------------------------------------------------------------------

def _like_match(s: str, pattern: str) -> bool:
    """SQL LIKE with % and _ (no escapes — TPC-DS uses only these)."""
    import re
    rx = "^" + re.escape(pattern).replace("%", ".*").replace("_", ".") + "$"
    return re.match(rx, s) is not None


def eval_expr(e: Expr, env: dict, nrows: int, device, stats=None) -> Val:
    """env: name -> Val. Returns Val with data on `device`.

    On a CUDA device the tree is compiled (`compile_expr`) and evaluated in
    one launch of the fused expression kernel; on the CPU, and for a tree the
    compiler does not cover (counted in `stats`), by the torch evaluator
    below, one torch op per node."""
    if isinstance(e, Col):
        v = env[e.name]
        if v is None:
            raise KeyError(e.name)
        return v
    if not isinstance(e, Lit) and _native_route(device, nrows):
        return eval_exprs([e], env, nrows, device, stats)[0]
    return _eval_torch(e, env, nrows, device)


def _eval_torch(e: Expr, env: dict, nrows: int, device) -> Val:
    """The torch evaluator: the CPU path and the NDS oracle."""
    if isinstance(e, Col):
        v = env[e.name]
        if v is None:
            raise KeyError(e.name)
        return v
    if isinstance(e, Lit):
        v = e.value
        if v is None:
            data = torch.zeros(nrows, dtype=torch.int64, device=device)
            return Val(data, torch.zeros(nrows, dtype=torch.bool, device=device))
        if isinstance(v, str):
            # standalone string literal: a single-entry-dictionary column
            return Val(torch.zeros(nrows, dtype=torch.int64, device=device),
                       None, [v])
        if isinstance(v, bool):
            dt = torch.bool
        elif isinstance(v, int):
            dt = torch.int64
        elif isinstance(v, float):
            dt = torch.float64
        else:
            raise TypeError(f"unsupported literal {v!r}")
        return Val(torch.full((nrows,), v, dtype=dt, device=device))
    if isinstance(e, Abs):
        v = _eval_torch(e.e, env, nrows, device)
        return Val(v.data.abs(), v.valid)
    if isinstance(e, BinOp):
        return _eval_binop(e, env, nrows, device)
    if isinstance(e, Not):
        v = _eval_torch(e.e, env, nrows, device)
        return Val(~v.data.bool(), v.valid)
    if isinstance(e, IsNull):
        v = _eval_torch(e.e, env, nrows, device)
        m = v.valid_mask()
        return Val(m if e.negate else ~m)
    if isinstance(e, InList):
        v = _eval_torch(e.e, env, nrows, device)
        vals = e.values
        if v.dict is not None:
            codes = [i for i, s in enumerate(v.dict) if s in set(vals)]
            vals = codes
        if not vals:
            return Val(torch.zeros(nrows, dtype=torch.bool, device=device),
                       v.valid)
        t = torch.tensor(vals, dtype=v.data.dtype, device=device)
        return Val(torch.isin(v.data, t), v.valid)
    if isinstance(e, Like):
        v = _eval_torch(e.e, env, nrows, device)
        assert v.dict is not None, "LIKE requires a dict-encoded column"
        codes = [i for i, s in enumerate(v.dict) if _like_match(s, e.pattern)]
        if not codes:
            return Val(torch.zeros(nrows, dtype=torch.bool, device=device),
                       v.valid)
        t = torch.tensor(codes, dtype=v.data.dtype, device=device)
        return Val(torch.isin(v.data, t), v.valid)
    if isinstance(e, Substr):
        v = _eval_torch(e.e, env, nrows, device)
        assert v.dict is not None, "substr requires a dict-encoded column"
        # remap codes through a substring'd dictionary
        sub = [s[e.start - 1:e.start - 1 + e.length] for s in v.dict]
        new_dict = sorted(set(sub))
        code_of = {s: i for i, s in enumerate(new_dict)}
        remap = torch.tensor([code_of[s] for s in sub], dtype=v.data.dtype,
                             device=device)
        return Val(remap[v.data.long()], v.valid, new_dict)
    if isinstance(e, Cast):
        v = _eval_torch(e.e, env, nrows, device)
        dt = torch.float64 if e.to == "float" else torch.int64
        return Val(v.data.to(dt), v.valid)
    if isinstance(e, CaseWhen):
        out_data = None
        out_valid = None
        decided = torch.zeros(nrows, dtype=torch.bool, device=device)
        for cond, value in e.branches:
            c = _eval_torch(cond, env, nrows, device)
            hit = c.data.bool() & c.valid_mask() & ~decided
            val = _eval_torch(value, env, nrows, device)
            if out_data is None:
                out_data = torch.zeros(nrows, dtype=val.data.dtype,
                                       device=device)
                out_valid = torch.zeros(nrows, dtype=torch.bool, device=device)
            if val.data.dtype != out_data.dtype:
                if out_data.dtype == torch.float64 or val.data.dtype == torch.float64:
                    out_data = out_data.to(torch.float64)
                    val = Val(val.data.to(torch.float64), val.valid, val.dict)
            out_data = torch.where(hit, val.data.to(out_data.dtype), out_data)
            out_valid = torch.where(hit, val.valid_mask(), out_valid)
            decided |= hit
        if e.otherwise is not None:
            val = _eval_torch(e.otherwise, env, nrows, device)
            if out_data is None:
                return val
            if val.data.dtype != out_data.dtype:
                out_data = out_data.to(torch.promote_types(out_data.dtype,
                                                           val.data.dtype))
            out_data = torch.where(decided, out_data,
                                   val.data.to(out_data.dtype))
            out_valid = torch.where(decided, out_valid, val.valid_mask())
        if out_data is None:
            out_data = torch.zeros(nrows, dtype=torch.int64, device=device)
            out_valid = torch.zeros(nrows, dtype=torch.bool, device=device)
        return Val(out_data, out_valid)
    if isinstance(e, Coalesce):
        out = _eval_torch(e.exprs[0], env, nrows, device)
        data, valid = out.data, out.valid_mask()
        for nxt in e.exprs[1:]:
            v = _eval_torch(nxt, env, nrows, device)
            need = ~valid
            if v.data.dtype != data.dtype:
                data = data.to(torch.promote_types(data.dtype, v.data.dtype))
            data = torch.where(need, v.data.to(data.dtype), data)
            valid = valid | (need & v.valid_mask())
        return Val(data, valid)
    raise TypeError(f"cannot evaluate {type(e).__name__}")


_CMP = {">": torch.gt, ">=": torch.ge, "<": torch.lt, "<=": torch.le,
        "==": torch.eq, "!=": torch.ne}


def _eval_binop(e: BinOp, env, nrows, device) -> Val:
    # string literal against a dict-encoded column: map to code space
    if e.op in ("==", "!="):
        lit_side = None
        if isinstance(e.r, Lit) and isinstance(e.r.value, str):
            col_v = _eval_torch(e.l, env, nrows, device)
            lit_side = e.r.value
        elif isinstance(e.l, Lit) and isinstance(e.l.value, str):
            col_v = _eval_torch(e.r, env, nrows, device)
            lit_side = e.l.value
        if lit_side is not None:
            assert col_v.dict is not None, "string literal vs non-dict column"
            try:
                code = col_v.dict.index(lit_side)
            except ValueError:
                code = -(2**40)  # never matches
            res = (col_v.data == code) if e.op == "==" else (col_v.data != code)
            return Val(res, col_v.valid)
    l = _eval_torch(e.l, env, nrows, device)
    r = _eval_torch(e.r, env, nrows, device)
    if (l.dict is not None and r.dict is not None
            and l.dict is not r.dict and e.op in ("==", "!=")):
        # two dict-encoded columns with different dictionaries: remap both
        # into a merged dictionary before comparing codes
        merged = {s: i for i, s in enumerate(sorted(set(l.dict) |
                                                    set(r.dict)))}
        lmap = torch.tensor([merged[s] for s in l.dict], dtype=torch.int64,
                            device=device)
        rmap = torch.tensor([merged[s] for s in r.dict], dtype=torch.int64,
                            device=device)
        l = Val(lmap[l.data.long()], l.valid)
        r = Val(rmap[r.data.long()], r.valid)
    if e.op == "and":
        ld, rd = l.data.bool(), r.data.bool()
        data = ld & rd
        if l.valid is None and r.valid is None:
            return Val(data)
        lv, rv = l.valid_mask(), r.valid_mask()
        # Kleene: FALSE and X = FALSE is definite
        valid = (lv & rv) | (lv & ~ld) | (rv & ~rd)
        return Val(data & valid, valid)
    if e.op == "or":
        ld, rd = l.data.bool(), r.data.bool()
        data = ld | rd
        if l.valid is None and r.valid is None:
            return Val(data)
        lv, rv = l.valid_mask(), r.valid_mask()
        valid = (lv & rv) | (lv & ld) | (rv & rd)
        return Val(data, valid)
    ld, rd = l.data, r.data
    if ld.dtype != rd.dtype:
        t = torch.promote_types(ld.dtype, rd.dtype)
        ld, rd = ld.to(t), rd.to(t)
    if e.op in _CMP:
        data = _CMP[e.op](ld, rd)
    elif e.op == "+":
        data = ld + rd
    elif e.op == "-":
        data = ld - rd
    elif e.op == "*":
        data = ld * rd
    elif e.op == "/":
        # SQL division: null on divide-by-zero, float result
        ld = ld.to(torch.float64)
        rd = rd.to(torch.float64)
        zero = rd == 0
        data = ld / torch.where(zero, torch.ones_like(rd), rd)
        valid = ~zero
        if l.valid is not None:
            valid &= l.valid
        if r.valid is not None:
            valid &= r.valid
        return Val(data, valid)
    else:
        raise ValueError(e.op)
    if l.valid is None and r.valid is None:
        return Val(data)
    return Val(data, l.valid_mask() & r.valid_mask())


# ---------------------------------------------------------------------------
# compilation to the fused expression kernel (ops/expr.py)
# ---------------------------------------------------------------------------

# Routing: frames below this many rows keep the torch evaluator on the GPU.
# Zero routes every size class to the kernel (docs/PERF.md, fused expression
# evaluation, has the measurement the value comes from).
NATIVE_MIN_ROWS = 0
# Forces the torch evaluator on every device (bench_micro.py measures the
# kernel against it).
FORCE_TORCH = False


class ExprStats:
    """Counts of what the CUDA route did: kernel calls, and every fallback to
    the torch evaluator with its reason."""

    def __init__(self):
        from collections import Counter
        self.native_calls = 0
        self.fallbacks = 0
        self.fallback_reasons = Counter()

    def fallback(self, reason: str):
        self.fallbacks += 1
        self.fallback_reasons[reason] += 1


STATS = ExprStats()  # calls that pass no stats of their own


class Unsupported(Exception):
    """An expression the compiler does not cover; the message is the reason
    counted with the fallback."""


def _native_route(device, nrows) -> bool:
    return (not FORCE_TORCH and torch.device(device).type == "cuda"
            and nrows >= NATIVE_MIN_ROWS)


class _Node:
    """A lowered subtree: its static dtype and dictionary, and `emit(p)`,
    which appends its instructions to a Program."""
    __slots__ = ("dtype", "dict", "emit")

    def __init__(self, dtype, dict, emit):
        self.dtype, self.dict, self.emit = dtype, dict, emit


class _Lowering:
    def __init__(self, program, env):
        self.p = program
        self.env = env
        self.names: List[str] = []
        self._index = {}

    def input(self, name):
        i = self._index.get(name)
        if i is None:
            v = self.env[name]
            i = self.p.add_input(v.data.dtype, v.valid is not None)
            self._index[name] = i
            self.names.append(name)
        return i

    def lower(self, e: Expr) -> _Node:
        m = getattr(self, "_" + type(e).__name__.lower(), None)
        if m is None:
            raise Unsupported(f"no lowering for {type(e).__name__}")
        return m(e)

    def _col(self, e):
        v = self.env[e.name]
        if v is None:
            raise KeyError(e.name)
        i = self.input(e.name)
        return _Node(v.data.dtype, v.dict, lambda p: p.load(i))

    def _lit(self, e):
        v = e.value
        if isinstance(v, str):
            return _Node(torch.int64, [v], lambda p: p.lit(0))
        if v is None:
            return _Node(torch.int64, None, lambda p: p.lit(None))
        if isinstance(v, bool):
            dt = torch.bool
        elif isinstance(v, int):
            if not -(2 ** 63) <= v < 2 ** 63:
                raise Unsupported("integer literal beyond int64")
            dt = torch.int64
        elif isinstance(v, float):
            dt = torch.float64
        else:
            raise TypeError(f"unsupported literal {v!r}")
        return _Node(dt, None, lambda p: p.lit(v))

    def _unary(self, e, dtype, method, *args):
        c = self.lower(e.e)

        def emit(p):
            c.emit(p)
            getattr(p, method)(*args)
        return _Node(dtype if dtype is not None else c.dtype, None, emit)

    def _abs(self, e):
        return self._unary(e, None, "abs")

    def _not(self, e):
        return self._unary(e, torch.bool, "not_")

    def _isnull(self, e):
        return self._unary(e, torch.bool, "is_null", e.negate)

    def _cast(self, e):
        dt = torch.float64 if e.to == "float" else torch.int64
        return self._unary(e, dt, "cast", dt)

    def _member(self, c, members):
        if c.dtype.is_floating_point or c.dtype == torch.bool:
            raise Unsupported(f"membership test over {c.dtype}")
        members = tuple(members)

        def emit(p):
            c.emit(p)
            p.in_set(members)
        return _Node(torch.bool, None, emit)

    def _inlist(self, e):
        c = self.lower(e.e)
        vals = e.values
        if c.dict is not None:
            want = set(vals)
            vals = [i for i, s in enumerate(c.dict) if s in want]
        elif not all(isinstance(x, int) for x in vals):
            raise Unsupported("in-list of non-integer values")
        return self._member(c, vals)

    def _like(self, e):
        c = self.lower(e.e)
        assert c.dict is not None, "LIKE requires a dict-encoded column"
        return self._member(
            c, [i for i, s in enumerate(c.dict) if _like_match(s, e.pattern)])

    def _substr(self, e):
        c = self.lower(e.e)
        assert c.dict is not None, "substr requires a dict-encoded column"
        sub = [s[e.start - 1:e.start - 1 + e.length] for s in c.dict]
        new_dict = sorted(set(sub))
        code_of = {s: i for i, s in enumerate(new_dict)}
        table = tuple(code_of[s] for s in sub) or (0,)

        def emit(p):
            c.emit(p)
            p.lut(table, c.dtype)
        return _Node(c.dtype, new_dict, emit)

    def _binop(self, e):
        if e.op in ("==", "!="):
            side = None
            if isinstance(e.r, Lit) and isinstance(e.r.value, str):
                side, other = e.r.value, e.l
            elif isinstance(e.l, Lit) and isinstance(e.l.value, str):
                side, other = e.l.value, e.r
            if side is not None:
                c = self.lower(other)
                assert c.dict is not None, "string literal vs non-dict column"
                try:
                    code = c.dict.index(side)
                except ValueError:
                    code = -(2 ** 40)  # never matches

                def emit_code(p):
                    # tensor == python scalar compares in the column's
                    # dtype, the scalar wrapped to it, as torch does
                    c.emit(p)
                    p.lit(code, c.dtype)
                    p.cmp(e.op)
                return _Node(torch.bool, None, emit_code)
        l, r = self.lower(e.l), self.lower(e.r)
        ltab = rtab = None
        ldt, rdt = l.dtype, r.dtype
        if (l.dict is not None and r.dict is not None
                and l.dict is not r.dict and e.op in ("==", "!=")):
            merged = {s: i for i, s in enumerate(sorted(set(l.dict) |
                                                        set(r.dict)))}
            ltab = tuple(merged[s] for s in l.dict) or (0,)
            rtab = tuple(merged[s] for s in r.dict) or (0,)
            ldt = rdt = torch.int64
        if e.op in ("and", "or") or e.op in _CMP:
            dt = torch.bool
        elif e.op == "/":
            dt = torch.float64
        elif e.op in ("+", "-", "*"):
            dt = torch.promote_types(ldt, rdt)
        else:
            raise ValueError(e.op)

        def emit(p):
            l.emit(p)
            if ltab is not None:
                p.lut(ltab)
            r.emit(p)
            if rtab is not None:
                p.lut(rtab)
            if e.op == "and":
                p.and_()
            elif e.op == "or":
                p.or_()
            elif e.op in _CMP:
                p.cmp(e.op)
            elif e.op == "+":
                p.add()
            elif e.op == "-":
                p.sub()
            elif e.op == "*":
                p.mul()
            else:
                p.div()
        return _Node(dt, None, emit)

    def _casewhen(self, e):
        conds = [self.lower(c) for c, _ in e.branches]
        vals = [self.lower(v) for _, v in e.branches]
        ow = self.lower(e.otherwise) if e.otherwise is not None else None
        if not vals:
            if ow is not None:
                return ow
            return _Node(torch.int64, None, lambda p: p.lit(None))
        # the dtypes every branch value passes through, as the torch
        # evaluator converts the running column branch after branch
        out_dt = None
        chains = []
        f64 = torch.float64
        for v in vals:
            if out_dt is None:
                out_dt = v.dtype
                chains.append([])
            elif v.dtype != out_dt and f64 in (out_dt, v.dtype):
                out_dt = f64
                for ch in chains:
                    ch.append(f64)
                chains.append([f64])
            else:
                chains.append([out_dt])
        if ow is not None and ow.dtype != out_dt:
            out_dt = torch.promote_types(out_dt, ow.dtype)
            for ch in chains:
                ch.append(out_dt)
        final = out_dt

        def emit(p):
            # last branch first: the first hit is applied last and wins
            if ow is not None:
                ow.emit(p)
                p.cast(final)
            else:
                p.lit(None, final)
            for c, v, ch in zip(reversed(conds), reversed(vals),
                                reversed(chains)):
                v.emit(p)
                for dt in ch:
                    p.cast(dt)
                c.emit(p)
                p.select()
        return _Node(final, None, emit)

    def _coalesce(self, e):
        nodes = [self.lower(x) for x in e.exprs]
        dt = nodes[0].dtype
        for nd in nodes[1:]:
            dt = torch.promote_types(dt, nd.dtype)

        def emit(p):
            if len(nodes) == 1:
                # only attaches a validity column: a null of the same dtype
                # below the value always yields the value's data
                p.lit(None, nodes[0].dtype)
                nodes[0].emit(p)
                p.coalesce_step()
                return
            nodes[0].emit(p)
            for nd in nodes[1:]:
                nd.emit(p)
                p.coalesce_step()
        return _Node(dt, None, emit)


class Compiled:
    """A compiled group of expressions: the Program, the frame columns it
    reads in input order, and the dictionary of every output."""
    __slots__ = ("program", "names", "dicts", "exprs", "env_dicts")

    def __init__(self, program, names, dicts, exprs, env_dicts):
        self.program, self.names, self.dicts = program, names, dicts
        # referenced so that the ids in the memo key stay unique
        self.exprs, self.env_dicts = exprs, env_dicts


def _compile(exprs, env, keep=False) -> Compiled:
    from ..ops.expr import Program, ProgramError
    p = Program()
    low = _Lowering(p, env)
    dicts = []
    try:
        for e in exprs:
            node = low.lower(e)
            node.emit(p)
            if keep:
                p.store_keep()
            else:
                p.store()
            dicts.append(node.dict)
    except ProgramError as err:
        raise Unsupported(str(err)) from None
    return Compiled(p, low.names, dicts, list(exprs),
                    [env[n].dict for n in low.names])


def compile_expr(e: Expr, env: dict):
    """The Program that evaluates `e` over a frame with the columns of `env`
    (one output), the names of the columns it reads in input order, and the
    result's dictionary. Only dtypes, validity presence and dictionaries of
    `env` are looked at, no tensor data. Raises `Unsupported` for a tree the
    kernel cannot evaluate."""
    c = _compile([e], env)
    return c.program, c.names, c.dicts[0]


_REFS = {}      # id(expr) -> (expr, columns it reads, structural key)
_PROGRAMS = {}  # (structural keys, keep, column signature) -> Compiled
_MEMO_MAX = 8192


def _structure(e: Expr, names: list):
    """A hashable key equal for trees of equal structure (queries rebuild
    their plans on every run), collecting the columns read into `names`."""
    if isinstance(e, Col):
        if e.name not in names:
            names.append(e.name)
        return ("col", e.name)
    if isinstance(e, Lit):
        return ("lit", type(e.value).__name__, repr(e.value))
    if isinstance(e, BinOp):
        return (e.op, _structure(e.l, names), _structure(e.r, names))
    if isinstance(e, CaseWhen):
        return ("case", tuple((_structure(c, names), _structure(v, names))
                              for c, v in e.branches),
                _structure(e.otherwise, names)
                if e.otherwise is not None else None)
    if isinstance(e, Coalesce):
        return ("coalesce", tuple(_structure(x, names) for x in e.exprs))
    if isinstance(e, IsNull):
        return ("isnull", e.negate, _structure(e.e, names))
    if isinstance(e, InList):
        return ("in", tuple((type(x).__name__, repr(x)) for x in e.values),
                _structure(e.e, names))
    if isinstance(e, Like):
        return ("like", e.pattern, _structure(e.e, names))
    if isinstance(e, Substr):
        return ("substr", e.start, e.length, _structure(e.e, names))
    if isinstance(e, Cast):
        return ("cast", e.to, _structure(e.e, names))
    if isinstance(e, (Not, Abs)):
        return (type(e).__name__, _structure(e.e, names))
    raise Unsupported(f"no lowering for {type(e).__name__}")


def _refs(e: Expr):
    hit = _REFS.get(id(e))
    if hit is None:
        names = []
        key = _structure(e, names)
        if len(_REFS) >= _MEMO_MAX:
            _REFS.clear()
        hit = _REFS[id(e)] = (e, tuple(names), key)
    return hit


def _compiled(exprs, env, keep) -> Compiled:
    """Memoised per (expression structure, input kinds, validity presence,
    dictionary identity)."""
    sig = []
    keys = []
    for e in exprs:
        _, names, key = _refs(e)
        keys.append(key)
        for n in names:
            v = env[n]
            if v is None:
                raise KeyError(n)
            sig.append((n, v.data.dtype, v.valid is not None, id(v.dict)))
    key = (tuple(keys), keep, tuple(sig))
    c = _PROGRAMS.get(key)
    if c is None:
        if len(_PROGRAMS) >= _MEMO_MAX:
            _PROGRAMS.clear()
        try:
            c = _compile(exprs, env, keep)
        except Unsupported as err:
            c = err
        _PROGRAMS[key] = c
    if isinstance(c, Unsupported):
        raise c
    return c


def _run(c: Compiled, env, nrows, device, stats):
    from ..ops.expr import eval_program
    outs = eval_program(c.program,
                        [(env[n].data, env[n].valid) for n in c.names],
                        nrows, device=device)
    stats.native_calls += 1
    return outs


def _eval_group(exprs, env, nrows, device, stats, keep=False):
    """One launch for the group; a group over a limit is halved, a single
    expression the compiler refuses takes the torch evaluator."""
    try:
        c = _compiled(exprs, env, keep)
    except Unsupported as err:
        if len(exprs) > 1:
            h = len(exprs) // 2
            return (_eval_group(exprs[:h], env, nrows, device, stats, keep) +
                    _eval_group(exprs[h:], env, nrows, device, stats, keep))
        stats.fallback(str(err))
        v = _eval_torch(exprs[0], env, nrows, device)
        if keep:
            m = v.data.bool()
            return [m & v.valid if v.valid is not None else m]
        return [v]
    outs = _run(c, env, nrows, device, stats)
    if keep:
        return [d for d, _ in outs]
    return [Val(d, v, dic) for (d, v), dic in zip(outs, c.dicts)]


def eval_exprs(exprs: Sequence[Expr], env: dict, nrows: int, device,
               stats=None) -> List[Val]:
    """`eval_expr` of every expression; on a CUDA device the computed ones
    share launches, up to the kernel's output limit per launch."""
    from ..ops.expr import MAX_OUTPUTS
    stats = stats if stats is not None else STATS
    out: List[Optional[Val]] = [None] * len(exprs)
    todo = []
    for i, e in enumerate(exprs):
        if isinstance(e, Col):
            v = env[e.name]
            if v is None:
                raise KeyError(e.name)
            out[i] = v
        elif isinstance(e, Lit) or not _native_route(device, nrows):
            out[i] = _eval_torch(e, env, nrows, device)
        else:
            todo.append(i)
    for lo in range(0, len(todo), MAX_OUTPUTS):
        part = todo[lo:lo + MAX_OUTPUTS]
        vals = _eval_group([exprs[i] for i in part], env, nrows, device,
                           stats)
        for i, v in zip(part, vals):
            out[i] = v
    return out


def eval_keep(e: Expr, env: dict, nrows: int, device, stats=None):
    """The rows a filter on `e` keeps: a bool tensor, true where `e` is true
    and not null. On a CUDA device one launch writes it directly."""
    stats = stats if stats is not None else STATS
    if isinstance(e, (Col, Lit)) or not _native_route(device, nrows):
        v = eval_expr(e, env, nrows, device, stats)
        m = v.data.bool()
        return m & v.valid if v.valid is not None else m
    return _eval_group([e], env, nrows, device, stats, keep=True)[0]
