"""Fused expression evaluation (ops/expr.py): the builder's typing, the CPU
twin against hand-written torch, the error paths, and on the GPU the kernel
against the twin, bit for bit, data under nulls included."""
import itertools

import pytest
import torch

from spark_rapids_jni_amd import _native
from spark_rapids_jni_amd.ops import expr as E
from spark_rapids_jni_amd.ops.expr import Program, ProgramError, eval_program

KINDS = list(range(7))
INT_KINDS = [E.I8, E.I16, E.I32, E.I64]
DT = E.KIND_DTYPES
T = torch.tensor


# ---------------------------------------------------------------------------
# shared data and programs
# ---------------------------------------------------------------------------

_EDGE_INT = {E.I8: [0, 1, -1, 127, -128, 100, -100],
             E.I16: [0, 1, -1, 32767, -32768, 20000, -20000],
             E.I32: [0, 1, -1, 2 ** 31 - 1, -2 ** 31, 2 ** 30, 46341],
             E.I64: [0, 1, -1, 2 ** 63 - 1, -2 ** 63, 2 ** 53 + 1, 2 ** 53,
                     2 ** 60 + 1, 2 ** 60, 3037000500]}
_EDGE_F = [0.0, -0.0, 1.0, -1.0, float("nan"), float("inf"), -float("inf"),
           1e-45, 3.4e38, 0.1, 16777217.0]


def _column(kind, n, seed, nullable, small=False):
    """Random column of a kind with its edge values up front. `small`: values
    that every kind can hold (for casts from float to integers)."""
    g = torch.Generator().manual_seed(seed)
    dt = DT[kind]
    if kind == E.BOOL:
        data = torch.rand(n, generator=g) < 0.5
    elif kind in INT_KINDS:
        if small:
            data = torch.randint(-100, 100, (n,), generator=g).to(dt)
        else:
            info = torch.iinfo(dt)
            data = torch.randint(info.min, info.max, (n,), generator=g,
                                 dtype=torch.int64).to(dt)
            edge = T(_EDGE_INT[kind], dtype=dt)[:n]
            data[:edge.numel()] = edge
    else:
        if small:
            data = (torch.rand(n, generator=g, dtype=torch.float64) * 200
                    - 100).to(dt)
            edge = T([0.0, -0.0, 99.5, -99.5], dtype=dt)[:n]
        else:
            data = (torch.randn(n, generator=g, dtype=torch.float64)
                    * 1e6).to(dt)
            edge = T(_EDGE_F, dtype=dt)[:n]
        data[:edge.numel()] = edge
        # equal pairs for the comparisons
        if n > 40:
            data[20:40] = data[20:40].round()
    valid = (torch.rand(n, generator=g) < 0.7) if nullable else None
    return data, valid


class Case:
    """A program and the columns it runs on."""

    def __init__(self, name, specs, build):
        # specs: (kind, nullable, small) per input
        self.name, self.specs, self.build = name, specs, build
        self.program = Program()
        for kind, nullable, _ in specs:
            self.program.add_input(DT[kind], nullable)
        build(self.program)

    def columns(self, n):
        return [_column(k, n, 17 * i + 3 * k + n, nl, small)
                for i, (k, nl, small) in enumerate(self.specs)]


def _binary_cases():
    out = []
    combos = [(False, False), (True, False), (False, True), (True, True)]
    for ka, kb in itertools.product(KINDS, KINDS):
        for na, nb in combos:
            def build1(p, ka=ka, kb=kb):
                for m in ("add", "sub", "mul", "div"):
                    if m == "sub" and E.promote(ka, kb) == E.BOOL:
                        continue
                    getattr(p.load(0).load(1), m)().store()
                for op in ("==", "!=", "<", "<="):
                    p.load(0).load(1).cmp(op).store()

            def build2(p):
                for op in (">", ">="):
                    p.load(0).load(1).cmp(op).store()
                p.load(0).load(1).and_().store()
                p.load(0).load(1).or_().store()
                p.load(0).load(1).coalesce_step().store()
                p.load(0).load(1).and_().store_keep()
            specs = [(ka, na, False), (kb, nb, False)]
            tag = f"{ka}{'n' if na else ''}-{kb}{'n' if nb else ''}"
            out.append(Case(f"arith-cmp {tag}", specs, build1))
            out.append(Case(f"cmp-logic {tag}", specs, build2))
    return out


def _unary_cases():
    out = []
    for k in KINDS:
        for nl in (False, True):
            def build(p, k=k):
                p.load(0).not_().store()
                p.load(0).is_null().store()
                p.load(0).is_null(negate=True).store()
                if k != E.BOOL:
                    p.load(0).abs().store()
                p.load(0).store()
                p.load(0).store_keep()
            out.append(Case(f"unary {k}{'n' if nl else ''}",
                            [(k, nl, False)], build))
        # casts: float sources hold values every integer kind can hold
        # (a float beyond the integer's range converts to anything)
        for lo in (0, 4):
            def build(p, lo=lo):
                for to in KINDS[lo:lo + 4]:
                    p.load(0).cast(DT[to]).store()
                    # a cast followed by arithmetic in the new kind
                    p.load(0).cast(DT[to]).load(0).cast(DT[to]).add().store()
            out.append(Case(f"cast {k} to {lo}..", [(k, True, k >= E.F32)],
                            build))
            if k < E.F32:
                out.append(Case(f"cast full-range {k} to {lo}..",
                                [(k, False, False)], build))
    return out


_SETS = {1: [37], 2: [-5, 90], 1000: list(range(-3000, 3000, 6))}


def _table_cases():
    out = []
    for k in INT_KINDS:
        def build(p):
            for members in _SETS.values():
                p.load(0).in_set(members).store()
            p.load(0).in_set([]).store()
            # probes below, between and above the members, and the members
            p.load(1).in_set(_SETS[1000]).store()
            p.load(1).in_set([-5, 90]).store()
        out.append(Case(f"in_set {k}", [(k, True, True), (k, False, False)],
                        build))

        def build_lut(p, k=k):
            table = [(i * 2654435761) % (2 ** 40) - 2 ** 39
                     for i in range(150)]
            for to in INT_KINDS:
                p.load(0).lut(table, DT[to]).store()
            p.load(0).lut([7], DT[k]).store()
            p.load(0).lut(table).load(0).add().store()
        out.append(Case(f"lut {k}", [(k, True, True)], build_lut))
    return out


def _select_cases():
    out = []
    for k in KINDS:
        def build(p):
            # [running, value, cond]
            p.load(0).load(1).load(2).select().store()
            p.lit(None, DT[k]).load(1).load(3).select().store()
        out.append(Case(f"select {k}", [(k, True, False), (k, True, False),
                                        (E.BOOL, True, False),
                                        (E.F64, True, False)], build))

    def case5(p):
        # 5 branches mixing int and float values, the last branch first
        p.lit(None, torch.float64)
        p.load(0).cast(torch.float64).load(4).load(0).cmp(">").select()
        p.load(1).load(0).lit(50).cmp("<").select()
        p.load(2).cast(torch.float64).load(2).lit(0).cmp("<").select()
        p.lit(2.5).load(3).select()
        p.load(0).load(2).mul().cast(torch.float64).load(4).lit(10)
        p.cmp("==").select()
        p.store()
    out.append(Case("case_when 5 branches",
                    [(E.I32, True, False), (E.F64, True, False),
                     (E.I64, False, False), (E.BOOL, True, False),
                     (E.I32, True, True)], case5))

    def coalesce4(p):
        p.load(0).load(1).coalesce_step().load(2).coalesce_step()
        p.lit(0.5).coalesce_step().store()
        p.load(0).load(1).coalesce_step().load(3).coalesce_step()
        p.load(2).coalesce_step().store()
    out.append(Case("coalesce 4-way",
                    [(E.I32, True, False), (E.I64, True, False),
                     (E.F64, True, False), (E.F32, True, False)], coalesce4))

    def many(p):
        for i in range(E.MAX_OUTPUTS):
            p.load(i % 3).load((i + 1) % 3).mul().lit(i).add().store()
    out.append(Case("max outputs", [(E.I32, True, False),
                                    (E.I64, False, False),
                                    (E.F64, True, False)], many))

    def limits(p):
        # exactly MAX_DEPTH deep and exactly MAX_INSTRS long
        for i in range(E.MAX_DEPTH):
            p.load(i % 2)
        for _ in range(E.MAX_DEPTH - 1):
            p.add()
        while len(p.instrs) < E.MAX_INSTRS - 1:
            p.load(1).mul() if len(p.instrs) % 4 else p.load(0).sub()
            if len(p.instrs) == E.MAX_INSTRS - 2:
                p.abs()
        p.store()
        assert len(p.instrs) == E.MAX_INSTRS and p.depth == E.MAX_DEPTH
    out.append(Case("limits", [(E.I32, True, False), (E.I64, False, False)],
                    limits))

    def beyond53(p):
        # int64 neighbours beyond 2^53: equal as doubles, not as integers
        p.load(0).load(0).lit(1).add().cmp("<").store()
        p.load(0).load(0).lit(1).add().cmp("==").store()
        p.load(0).lit(2 ** 60 + 1).cmp("==").store()
        p.load(0).lit(2 ** 53).cmp(">").store()
        p.load(0).load(0).mul().store()
    out.append(Case("int64 beyond 2^53", [(E.I64, True, False)], beyond53))
    return out


_CASES = None


def all_cases():
    global _CASES
    if _CASES is None:
        _CASES = (_binary_cases() + _unary_cases() + _table_cases()
                  + _select_cases())
    return _CASES


def _bits_equal(a, b):
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype.is_floating_point:
        it = torch.int64 if a.dtype == torch.float64 else torch.int32
        same = (a.view(it) == b.view(it)) | (a.isnan() & b.isnan())
        return bool(same.all())
    return torch.equal(a, b)


def _assert_same(got, want, what):
    assert len(got) == len(want), what
    for i, ((gd, gv), (wd, wv)) in enumerate(zip(got, want)):
        assert _bits_equal(gd.cpu(), wd), f"{what}: output {i} data"
        assert (gv is None) == (wv is None), f"{what}: output {i} None-ness"
        if wv is not None:
            assert gv.dtype == torch.bool
            assert torch.equal(gv.cpu(), wv), f"{what}: output {i} validity"


# ---------------------------------------------------------------------------
# CPU tier: builder typing
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("ka,kb", itertools.product(KINDS, KINDS))
def test_builder_types_like_torch(ka, kb):
    want = torch.promote_types(DT[ka], DT[kb])
    for m in ("add", "mul", "sub", "coalesce_step"):
        if m == "sub" and want == torch.bool:
            continue
        p = Program()
        p.add_input(DT[ka], False)
        p.add_input(DT[kb], True)
        getattr(p.load(0).load(1), m)()
        assert p.top_dtype == want
        assert p.top_nullable is True
    p = Program()
    p.add_input(DT[ka], False)
    p.add_input(DT[kb], False)
    p.load(0).load(1).div()
    assert p.top_dtype == torch.float64 and p.top_nullable
    for op in ("==", "<"):
        p.load(0).load(1).cmp(op)
        assert p.top_dtype == torch.bool and not p.top_nullable
    p.load(0).load(1).and_()
    assert p.top_dtype == torch.bool and not p.top_nullable
    # the twin gives the dtype the builder announced
    a = torch.ones(3, dtype=DT[ka])
    b = torch.ones(3, dtype=DT[kb])
    q = Program()
    q.add_input(DT[ka], False)
    q.add_input(DT[kb], False)
    q.load(0).load(1).add().store()
    (data, valid), = eval_program(q, [a, b], 3)
    assert data.dtype == want and valid is None
    assert data.dtype == (a + b).dtype


def test_builder_static_nullability_and_literals():
    p = Program()
    p.add_input(torch.int32, True)
    assert p.load(0).top_nullable
    assert not p.is_null().top_nullable
    assert p.lit(3).top_dtype == torch.int64
    assert p.lit(True).top_dtype == torch.bool
    assert p.lit(1.5).top_dtype == torch.float64
    assert p.lit(None).top_nullable and p.top_dtype == torch.int64
    assert p.lit(7, torch.int8).top_dtype == torch.int8
    p.load(0).cast(torch.int64)  # widening: retyped, no instruction
    n = len(p.instrs)
    assert p.top_dtype == torch.int64
    p.cast(torch.int64)
    assert len(p.instrs) == n
    p.cast(torch.float64)
    assert len(p.instrs) == n + 1 and p.top_dtype == torch.float64
    # the same constant array is shared
    q = Program()
    q.add_input(torch.int32, False)
    q.load(0).in_set([3, 1, 2]).store()
    q.load(0).in_set([1, 2, 3, 3]).store()
    assert len(q.consts) == 1 and q.consts[0] == (1, 2, 3)


# ---------------------------------------------------------------------------
# CPU tier: the twin against hand-written torch
# ---------------------------------------------------------------------------

def _run1(build, cols, n=None):
    p = Program()
    for c in cols:
        d, v = c if isinstance(c, tuple) else (c, None)
        p.add_input(d.dtype, v is not None)
    build(p)
    n = cols[0][0].numel() if isinstance(cols[0], tuple) else cols[0].numel()
    return eval_program(p, cols, n)


A32 = T([2 ** 31 - 1, -2 ** 31, 7, 0, -9], dtype=torch.int32)
B32 = T([2, -1, 0, 5, 3], dtype=torch.int32)
A64 = T([2 ** 63 - 1, 2 ** 53 + 1, 7, 0, -9], dtype=torch.int64)
F64 = T([1.5, float("nan"), -0.0, 0.0, -2.25], dtype=torch.float64)
F32 = T([0.1, 16777216.0, -0.0, 3e38, 1.0], dtype=torch.float32)
VA = T([True, False, True, True, False])
VB = T([True, True, False, True, False])
TF = T([True, False, True, False, True])
FT = T([True, True, False, False, True])


def test_twin_arithmetic_wraps_and_rounds():
    (add, av), (mul, _), (sub, _) = _run1(
        lambda p: (p.load(0).load(1).add().store(),
                   p.load(0).load(1).mul().store(),
                   p.load(0).load(1).sub().store()), [(A32, VA), (B32, VB)])
    assert torch.equal(add, A32 + B32) and add.dtype == torch.int32
    assert torch.equal(mul, A32 * B32) and torch.equal(sub, A32 - B32)
    assert torch.equal(av, VA & VB)
    (m64, v), = _run1(lambda p: p.load(0).load(1).mul().store(), [A64, B32])
    assert v is None and torch.equal(m64, A64 * B32.to(torch.int64))
    (f, _), = _run1(lambda p: p.load(0).load(1).add().store(), [F32, A32])
    assert f.dtype == torch.float32 and torch.equal(f, F32 + A32)
    (f, _), = _run1(lambda p: p.load(0).lit(3).mul().store(), [A32])
    assert f.dtype == torch.int64 and torch.equal(f, A32.to(torch.int64) * 3)


def test_twin_div():
    (d, v), = _run1(lambda p: p.load(0).load(1).div().store(),
                    [(A32, VA), B32])
    den = B32.double()
    assert torch.equal(d, A32.double() / torch.where(den == 0,
                                                     torch.ones(5).double(),
                                                     den))
    assert torch.equal(v, VA & (B32 != 0))


def test_twin_comparisons():
    for op, fn in (("==", torch.eq), ("!=", torch.ne), ("<", torch.lt),
                   ("<=", torch.le), (">", torch.gt), (">=", torch.ge)):
        (d, v), = _run1(lambda p: p.load(0).load(1).cmp(op).store(),
                        [(F64, VA), (A32, VB)])
        assert torch.equal(d, fn(F64, A32.double()))
        assert torch.equal(v, VA & VB)
    # int64 beyond 2^53 compares as an integer
    (d, _), = _run1(lambda p: p.load(0).lit(2 ** 53).cmp("==").store(), [A64])
    assert d.tolist() == [False] * 5


def test_twin_kleene_logic():
    (a, av), (o, ov) = _run1(
        lambda p: (p.load(0).load(1).and_().store(),
                   p.load(0).load(1).or_().store()), [(TF, VA), (FT, VB)])
    v = (VA & VB) | (VA & ~TF) | (VB & ~FT)
    assert torch.equal(av, v) and torch.equal(a, TF & FT & v)
    v = (VA & VB) | (VA & TF) | (VB & FT)
    assert torch.equal(ov, v) and torch.equal(o, TF | FT)
    (a, av), = _run1(lambda p: p.load(0).load(1).and_().store(), [TF, A32])
    assert av is None and torch.equal(a, TF & (A32 != 0))


def test_twin_unary():
    (n, nv), (isn, x), (nn, y), (ab, abv), (fab, _) = _run1(
        lambda p: (p.load(0).not_().store(), p.load(0).is_null().store(),
                   p.load(0).is_null(negate=True).store(),
                   p.load(0).abs().store(), p.load(1).abs().store()),
        [(A32, VA), F64])
    assert torch.equal(n, A32 == 0) and torch.equal(nv, VA)
    assert torch.equal(isn, ~VA) and x is None
    assert torch.equal(nn, VA) and y is None
    assert torch.equal(ab, A32.abs()) and torch.equal(abv, VA)
    assert _bits_equal(fab, F64.abs())


def test_twin_cast():
    small = T([1.9, -1.9, 0.0, -0.0, 99.0], dtype=torch.float64)
    (i, _), (f, _), (b, _), (n, _) = _run1(
        lambda p: (p.load(0).cast(torch.int64).store(),
                   p.load(1).cast(torch.float64).store(),
                   p.load(0).cast(torch.bool).store(),
                   p.load(1).cast(torch.int8).store()), [small, A64])
    assert torch.equal(i, small.to(torch.int64))
    assert torch.equal(f, A64.double()) and torch.equal(b, small != 0)
    assert torch.equal(n, A64.to(torch.int8))


def test_twin_in_set_and_lut():
    x = T([-7, 0, 3, 4, 9], dtype=torch.int32)
    (a, av), (e, _), (l, _) = _run1(
        lambda p: (p.load(0).in_set([9, 3, -7]).store(),
                   p.load(0).in_set([]).store(),
                   p.load(0).lut([10, 11, 12, 13, 14], torch.int16).store()),
        [(x, VA)])
    assert a.tolist() == [True, False, True, False, True]
    assert torch.equal(av, VA) and e.tolist() == [False] * 5
    assert l.dtype == torch.int16 and l.tolist() == [10, 10, 13, 14, 14]


def test_twin_select_and_coalesce():
    (s, sv), (c, cv) = _run1(
        lambda p: (p.load(0).load(1).load(2).select().store(),
                   p.load(0).load(1).coalesce_step().store()),
        [(A32, VA), (B32, VB), (TF, FT)])
    hit = TF & FT
    assert torch.equal(s, torch.where(hit, B32, A32))
    assert torch.equal(sv, torch.where(hit, VB, VA))
    assert torch.equal(c, torch.where(VA, A32, B32))
    assert torch.equal(cv, VA | VB)


def test_twin_store_keep_and_empty():
    (k, v), = _run1(lambda p: p.load(0).store_keep(), [(A32, VA)])
    assert v is None and k.dtype == torch.bool
    assert torch.equal(k, (A32 != 0) & VA)
    p = Program()
    p.add_input(torch.float32, True)
    p.load(0).lit(1).add().store()
    (d, v), = eval_program(p, [(F32[:0], VA[:0])], 0)
    assert d.dtype == torch.float32 and d.numel() == 0
    assert v.dtype == torch.bool and v.numel() == 0
    # an output never aliases an input
    (d, _), = _run1(lambda p: p.load(0).store(), [A32])
    assert d is not A32 and torch.equal(d, A32)


# ---------------------------------------------------------------------------
# CPU tier: error paths
# ---------------------------------------------------------------------------

def _prog1():
    p = Program()
    p.add_input(torch.int32, False)
    return p


def test_builder_errors():
    with pytest.raises(ProgramError, match="underflow"):
        _prog1().load(0).add()
    with pytest.raises(ProgramError, match="underflow"):
        _prog1().store()
    with pytest.raises(ProgramError, match="out of range"):
        _prog1().load(1)
    with pytest.raises(ProgramError, match="unsupported dtype"):
        Program().add_input(torch.uint8, False)
    with pytest.raises(ProgramError, match="unsupported literal"):
        _prog1().lit("x")
    with pytest.raises(ProgramError, match="unknown comparison"):
        _prog1().load(0).load(0).cmp("<>")
    with pytest.raises(ProgramError, match="bool - bool"):
        _prog1().lit(True).lit(False).sub()
    with pytest.raises(ProgramError, match="abs of bool"):
        _prog1().lit(True).abs()
    with pytest.raises(ProgramError, match="integer operand"):
        _prog1().lit(1.0).in_set([1])
    with pytest.raises(ProgramError, match="integer operand"):
        _prog1().load(0).lut([1], torch.float64)
    with pytest.raises(ProgramError, match="at least one"):
        _prog1().load(0).lut([])
    with pytest.raises(ProgramError, match="differ in dtype"):
        _prog1().load(0).lit(1).lit(True).select()
    p = _prog1()
    for _ in range(E.MAX_DEPTH):
        p.load(0)
    with pytest.raises(ProgramError, match="deeper"):
        p.load(0)
    p = _prog1()
    for _ in range(E.MAX_OUTPUTS):
        p.load(0).store()
    with pytest.raises(ProgramError, match="outputs"):
        p.load(0).store()
    p = _prog1().load(0)
    for _ in range(E.MAX_INSTRS - 1):
        p.abs()
    with pytest.raises(ProgramError, match="instructions"):
        p.abs()
    p = Program()
    for _ in range(E.MAX_INPUTS):
        p.add_input(torch.int8, False)
    with pytest.raises(ProgramError, match="inputs"):
        p.add_input(torch.int8, False)
    p = _prog1().load(0)
    for i in range(E.MAX_CONSTS):
        p.in_set([i]).cast(torch.int32)
    with pytest.raises(ProgramError, match="constant arrays"):
        p.in_set([-1])


def test_eval_program_errors():
    x = torch.zeros(4, dtype=torch.int32)
    ok = _prog1()
    ok.load(0).store()
    with pytest.raises(ValueError, match="declares 1 inputs"):
        eval_program(ok, [], 4, device="cpu")
    with pytest.raises(TypeError, match="declared torch.int32"):
        eval_program(ok, [x.long()], 4)
    with pytest.raises(ValueError, match="4 rows"):
        eval_program(ok, [x[:3]], 4)
    with pytest.raises(ValueError, match="not nullable"):
        eval_program(ok, [(x, x == 0)], 4)
    with pytest.raises(TypeError, match="valid must be"):
        p = Program()
        p.add_input(torch.int32, True)
        p.load(0).store()
        eval_program(p, [(x, x)], 4)
    with pytest.raises(ValueError, match="nrows < 0"):
        eval_program(ok, [x], -1)
    with pytest.raises(ProgramError, match="left on the stack"):
        p = _prog1()
        p.load(0).store()
        p.load(0)
        eval_program(p, [x], 4)
    with pytest.raises(ProgramError, match="stores no output"):
        eval_program(_prog1(), [x], 4)
    with pytest.raises(ValueError, match="needs a device"):
        p = Program()
        p.lit(1).store()
        eval_program(p, [], 4)


def _ins(op, kind=E.I64, arg=0, imm=0):
    return E._INSTR.pack(op, kind, arg, 0, imm)


def test_binding_errors():
    g = _native.gpu()
    assert g.EXPR_MAX_INSTRS == E.MAX_INSTRS
    assert g.EXPR_MAX_DEPTH == E.MAX_DEPTH
    assert g.EXPR_MAX_INPUTS == E.MAX_INPUTS
    assert g.EXPR_MAX_OUTPUTS == E.MAX_OUTPUTS
    assert g.EXPR_MAX_CONSTS == E.MAX_CONSTS
    assert g.EXPR_ROWS_PER_THREAD == E.ROWS_PER_THREAD
    assert g.EXPR_MAX_GRID == E.MAX_GRID
    ins = [(4096, 0, E.I64)]
    outs = [(8192, 0)]
    load, store = _ins(E.LOAD_COL), _ins(E.STORE)
    good = load + store
    assert g.expr_check(good, ins, outs, [], 10) == 1
    ii = E.I64 | E.I64 << 4

    def bad(match, code=good, inputs=ins, outputs=outs, consts=(), rows=10):
        with pytest.raises(ValueError, match=match):
            g.expr_check(code, inputs, outputs, list(consts), rows)

    bad("rows < 0", rows=-1)
    bad("whole number", code=good + b"\0")
    bad("empty program", code=b"")
    bad("unknown op", code=_ins(E.STORE_KEEP + 1) + good)
    bad("unknown kind", code=_ins(E.LOAD_COL, kind=7) + store)
    bad("unknown kind", inputs=[(4096, 0, 9)])
    bad("input out of range", code=_ins(E.LOAD_COL, arg=1) + store)
    bad("output out of range", code=load + _ins(E.STORE, arg=1))
    bad("arg must be 0 or 1", code=_ins(E.LIT, arg=2) + store)
    bad("constant array out of range",
        code=load + _ins(E.IN_SET, E.BOOL, E.I64, 0) + store)
    bad("constant array out of range", consts=[(4096, 4)],
        code=load + _ins(E.LUT, E.I64, E.I64, -1) + store)
    bad("empty lookup table", consts=[(0, 0)],
        code=load + _ins(E.LUT, E.I64, E.I64, 0) + store)
    bad("operand must be an integer", consts=[(4096, 4)],
        code=load + _ins(E.IN_SET, E.BOOL, E.F64, 0) + store)
    bad("unknown operand kind",
        code=load + load + _ins(E.ADD, E.I64, 7 | E.I64 << 4) + store)
    bad("unknown operand kind", code=load + _ins(E.CAST, E.I64, 9) + store)
    bad("DIV is F64", code=load + load + _ins(E.DIV, E.I64, ii) + store)
    bad("null data", inputs=[(0, 0, E.I64)])
    bad("null data", outputs=[(0, 0)])
    bad("null data", consts=[(0, 3)])
    bad("negative length", consts=[(4096, -1)])
    bad("not aligned to its element", inputs=[(4100, 0, E.I64)])
    bad("not aligned to its element", outputs=[(8196, 0)])
    bad("not aligned to 8", consts=[(4100, 3)])
    bad("EXPR_MAX_INSTRS",
        code=load + _ins(E.ABS) * E.MAX_INSTRS + store)
    bad("EXPR_MAX_INPUTS", inputs=ins * (E.MAX_INPUTS + 1))
    bad("EXPR_MAX_OUTPUTS", outputs=outs * (E.MAX_OUTPUTS + 1))
    bad("EXPR_MAX_OUTPUTS", outputs=[])
    bad("EXPR_MAX_CONSTS", consts=[(4096, 1)] * (E.MAX_CONSTS + 1))
    bad("stack underflow", code=store)
    bad("stack underflow", code=load + _ins(E.ADD, E.I64, ii) + store)
    bad("stack underflow", code=load + load + _ins(E.SELECT) + store)
    bad("deeper than EXPR_MAX_DEPTH",
        code=load * (E.MAX_DEPTH + 1) + store * (E.MAX_DEPTH + 1))
    bad("values left", code=load + good)
    bad("never stored", outputs=outs * 2)
    bad("stored twice", code=good + good)
    # a 4-byte output may sit on a 4-byte boundary
    assert g.expr_check(load + _ins(E.STORE, E.I32), ins, [(8196, 0)], [],
                        10) == 1
    assert g.expr_check(load * E.MAX_DEPTH
                        + _ins(E.ADD, E.I64, ii) * (E.MAX_DEPTH - 1) + store,
                        ins, outs, [], 10) == E.MAX_DEPTH


def test_cases_cover_every_opcode():
    """The GPU cases below exercise every opcode with every kind it takes."""
    seen = set()
    for c in all_cases():
        for op, kind, arg, _ in c.program.instrs:
            seen.add(op)
    assert seen == set(range(E.STORE_KEEP + 1))
    for c in all_cases():
        n = 65
        cols = c.columns(n)
        outs = eval_program(c.program, cols, n)
        assert len(outs) == len(c.program.outputs), c.name


# ---------------------------------------------------------------------------
# GPU tier: the kernel against the twin
# ---------------------------------------------------------------------------

def _to_cuda(cols):
    return [(d.cuda(), v.cuda() if v is not None else None) for d, v in cols]


FULL_PASS = E.MAX_GRID * E.BLOCK * E.ROWS_PER_THREAD


@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257])
def test_kernel_matches_twin(n):
    for c in all_cases():
        cols = c.columns(n)
        want = eval_program(c.program, cols, n)
        got = eval_program(c.program, _to_cuda(cols), n)
        for d, _ in got:
            assert d.is_cuda
        _assert_same(got, want, f"{c.name} rows {n}")


@pytest.mark.gpu
def test_kernel_matches_twin_past_one_grid_pass():
    # the grid-stride loop does not depend on the opcode: one case of each
    # family, each with a row in the second pass of the last workgroups
    n = FULL_PASS + 1
    picked = {}
    for c in all_cases():
        picked.setdefault(c.name.split()[0], c)
    assert len(picked) >= 8
    for c in picked.values():
        cols = c.columns(n)
        want = eval_program(c.program, cols, n)
        got = eval_program(c.program, _to_cuda(cols), n)
        _assert_same(got, want, f"{c.name} rows {n}")


@pytest.mark.gpu
def test_kernel_is_deterministic():
    n = 5000
    for c in all_cases()[::7]:
        cols = _to_cuda(c.columns(n))
        a = eval_program(c.program, cols, n)
        b = eval_program(c.program, cols, n)
        _assert_same(a, [(d.cpu(), v.cpu() if v is not None else None)
                         for d, v in b], c.name)


@pytest.mark.gpu
def test_kernel_under_graph_capture():
    n = 3000
    c = next(c for c in all_cases() if c.name == "case_when 5 branches")
    first = c.columns(n)
    cols = _to_cuda(first)
    eval_program(c.program, cols, n)  # constants are uploaded outside
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            outs = eval_program(c.program, cols, n)
    torch.cuda.current_stream().wait_stream(side)
    # new inputs, written in place
    fresh = [_column(k, n, 991 + i, nl, small)
             for i, (k, nl, small) in enumerate(c.specs)]
    for (d, v), (nd, nv) in zip(cols, fresh):
        d.copy_(nd)
        if v is not None:
            v.copy_(nv)
    graph.replay()
    torch.cuda.synchronize()
    _assert_same(outs, eval_program(c.program, fresh, n), "replay")
    assert not _bits_equal(outs[0][0].cpu(),
                           eval_program(c.program, first, n)[0][0])
