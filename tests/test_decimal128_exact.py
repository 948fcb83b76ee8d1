"""DECIMAL128 arithmetic over its whole domain against an exact oracle.

The oracle is plain Python integer arithmetic (arbitrary precision). The CPU
tests check it against decimal.Decimal and check the result-type helpers; the
GPU tests compare the HIP kernels with it: validity exactly, data exactly
wherever the oracle's result is non-null.

Divide is the exact HALF_UP of the true quotient. For
e = out_scale - s1 + s2 < 0 the reference divides twice and truncates the
first time, so it can differ in the last digit; the exact value is what this
project computes and what is tested here.
"""
import functools
import os
import random
import subprocess
from decimal import ROUND_HALF_UP, Decimal, localcontext

import numpy as np
import pytest
import torch

from spark_rapids_jni_amd.columnar import Column, DType, validity_nbytes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAXV = 10**38 - 1


# ---------------------------------------------------------------------------
# the oracle
# ---------------------------------------------------------------------------
def half_up(num, den):
    q, r = divmod(abs(num), abs(den))
    q += 2 * r >= abs(den)
    return -q if (num < 0) != (den < 0) else q


def _fit(r, precision):
    return None if abs(r) >= 10**precision else r


def o_mul(x, y, s1, s2, out_scale, precision=38):
    if x is None or y is None:
        return None
    d = s1 + s2 - out_scale
    r = half_up(x * y, 10**d) if d > 0 else x * y * 10**(-d)
    return _fit(r, precision)


def o_div(x, y, s1, s2, out_scale, precision=38):
    if x is None or y is None or y == 0:
        return None
    e = out_scale - s1 + s2
    r = half_up(x * 10**e, y) if e >= 0 else half_up(x, y * 10**(-e))
    return _fit(r, precision)


def o_intdiv(x, y, s1, s2):
    if x is None or y is None or y == 0:
        return None
    q = (abs(x) * 10**s2) // (abs(y) * 10**s1)
    return _fit(-q if (x < 0) != (y < 0) else q, 38)


def o_rem(x, y, s1, s2):
    if x is None or y is None or y == 0:
        return None
    s = max(s1, s2)
    xx, yy = x * 10**(s - s1), y * 10**(s - s2)
    r = abs(xx) % abs(yy)
    return -r if xx < 0 else r


def o_add(x, y, s1, s2, precision=38, sub=False):
    if x is None or y is None:
        return None
    s = max(s1, s2)
    xx, yy = x * 10**(s - s1), y * 10**(s - s2)
    return _fit(xx - yy if sub else xx + yy, precision)


def o_sub(x, y, s1, s2, precision=38):
    return o_add(x, y, s1, s2, precision, sub=True)


# ---------------------------------------------------------------------------
# operands
# ---------------------------------------------------------------------------
def _directed():
    mags = [0, 1, 2**63, 2**64 + 1, 2**64 - 1, 2**96, 2**126, MAXV]
    for k in (1, 18, 19, 20, 37):
        mags += [10**k, 10**k + 1, 10**k - 1, 5 * 10**k, 5 * 10**k - 1]
    return [m for m in mags] + [-m for m in mags if m]


DIRECTED = _directed()
# Each case: every directed value against a random one on either side, this
# many shuffled directed-against-directed pairings, random pairs for the rest.
DIRECTED_ROUNDS = 8
ROWS = 1500
MASKS = ("both", "a", "b", "neither")


FULL = 126  # bits: the whole domain, values capped at 10^38 - 1


def rand_operand(rng, max_bits=FULL):
    """bit length uniform in [1, max_bits], value uniform at that length"""
    if max_bits < 1:
        return 0
    bits = rng.randint(1, max_bits)
    v = min(rng.randrange(2**(bits - 1), 2**bits), MAXV)
    return -v if rng.random() < 0.5 else v


@functools.lru_cache(maxsize=None)
def operands(seed, n=ROWS, mask="both", bits=(FULL, FULL)):
    """(xs, ys) of n rows, None = null; about 10% null rows, on the side(s)
    that `mask` names. bits: the widest random operand of either side; the
    directed values are always the same."""
    rng = random.Random(seed)
    xs = list(DIRECTED) + [rand_operand(rng, bits[0]) for _ in DIRECTED]
    ys = [rand_operand(rng, bits[1]) for _ in DIRECTED] + list(DIRECTED)
    for _ in range(DIRECTED_ROUNDS):
        perm = list(DIRECTED)
        rng.shuffle(perm)
        xs += DIRECTED
        ys += perm
    while len(xs) < n:
        xs.append(rand_operand(rng, bits[0]))
        ys.append(rand_operand(rng, bits[1]))
    order = list(range(len(xs)))
    rng.shuffle(order)
    xs = [xs[i] for i in order][:n]
    ys = [ys[i] for i in order][:n]
    for i in range(n):
        if mask != "neither" and rng.random() < 0.1:
            side = mask if mask != "both" else rng.choice("ab")
            if side == "a":
                xs[i] = None
            else:
                ys[i] = None
    return tuple(xs), tuple(ys)


def _mask_of(index):
    return MASKS[index % len(MASKS)]


# (s1, s2, out_scale, out_precision)
MUL_CONFIGS = [(0, 0, 0, 38), (3, 2, 4, 38), (10, 10, 6, 38), (18, 18, 6, 38),
               (38, 38, 38, 38), (2, 3, 10, 38), (0, 0, 5, 38), (3, 2, 4, 20)]
DIV_CONFIGS = [(2, 3, 6, 38), (0, 0, 6, 38), (18, 2, 21, 38), (0, 20, 6, 38),
               (6, 38, 6, 38), (0, 38, 0, 38), (38, 0, 38, 38),
               (10, 0, 6, 38), (20, 0, 6, 38), (2, 3, 6, 18)]
INTDIV_CONFIGS = [(0, 0), (2, 4), (19, 19), (20, 38), (0, 38), (38, 0)]
REM_CONFIGS = [(0, 0), (2, 4), (0, 10), (10, 0), (5, 30)]
ADD_CONFIGS = [(s1, s2, p) for p in (38, 20)
               for s1, s2 in [(0, 0), (2, 4), (0, 1), (0, 10), (5, 30)]]


# Random operands are full width wherever a configuration can hold them. Two
# kinds of configuration cannot: with full-width operands the oracle leaves
# them 64% to 100% null, more once the directed rows and the input nulls are
# mixed in, and a case of nulls checks no arithmetic. Their random operands
# are drawn narrower, by these rules; the directed rows still overflow them.
#  * add / subtract: a side scaled up by k digits under precision p has room
#    for p - k digits. Where that is 20 digits or fewer (every precision-20
#    case, and the 25-digit gap of (5, 30)) the side is drawn within that
#    room, as a full-width operand is within 38 digits. No room: the side is 0.
#  * multiply: x * y has to stay below 10^(p + drop). Where that limit is
#    below 10^38 (precision 20, and the two scale-up shapes) each factor gets
#    three quarters of the limit's bits, so that about a fifth of the random
#    products still pass the limit.
def _pow10_bits(digits):
    return (10**digits).bit_length() - 1 if digits > 0 else 0


def add_bits(s1, s2, precision):
    room = [precision - (max(s1, s2) - s) for s in (s1, s2)]
    return tuple(_pow10_bits(r) if r <= 20 else FULL for r in room)


def mul_bits(s1, s2, out_scale, precision):
    limit = precision + s1 + s2 - out_scale
    if limit >= 38:
        return FULL, FULL
    return (3 * _pow10_bits(limit) // 4,) * 2


def full_bits(*cfg):
    return FULL, FULL


def _ids(configs):
    return ["-".join(map(str, c)) for c in configs]


def _case(op_seed, configs, cfg, oracle, bits=full_bits):
    """Operands of one configuration and the oracle's column for them."""
    idx = configs.index(cfg)
    xs, ys = operands(op_seed * 100 + idx, mask=_mask_of(idx), bits=bits(*cfg))
    exp = [oracle(x, y, *cfg) for x, y in zip(xs, ys)]
    live = sum(e is not None for e in exp)
    # from the oracle alone: a kernel that nulls everything cannot pass
    assert live >= 0.3 * len(exp), f"only {live}/{len(exp)} non-null rows"
    return xs, ys, exp


# ---------------------------------------------------------------------------
# CPU tier: the oracle against decimal.Decimal
# ---------------------------------------------------------------------------
def _dec(v, scale):
    return Decimal(v).scaleb(-scale)


def _unscaled(d, scale):
    q = d.quantize(Decimal(1).scaleb(-scale), rounding=ROUND_HALF_UP)
    return int(q.scaleb(scale))


def _rows(seed, n=400):
    xs, ys = operands(seed, n=n, mask="neither")
    return list(zip(xs, ys))


@pytest.mark.parametrize("cfg", MUL_CONFIGS, ids=_ids(MUL_CONFIGS))
def test_oracle_multiply_vs_decimal(cfg):
    s1, s2, out_scale, prec = cfg
    with localcontext() as ctx:
        ctx.prec, ctx.rounding = 120, ROUND_HALF_UP
        for x, y in _rows(11):
            u = _unscaled(_dec(x, s1) * _dec(y, s2), out_scale)
            exp = None if abs(u) >= 10**prec else u
            assert o_mul(x, y, *cfg) == exp, (x, y)


@pytest.mark.parametrize("cfg", DIV_CONFIGS, ids=_ids(DIV_CONFIGS))
def test_oracle_divide_vs_decimal(cfg):
    s1, s2, out_scale, prec = cfg
    with localcontext() as ctx:
        ctx.prec, ctx.rounding = 120, ROUND_HALF_UP
        for x, y in _rows(12):
            if y == 0:
                assert o_div(x, y, *cfg) is None
                continue
            # 120 digits hold the widest quotient (76 integral digits and
            # 38 decimals) with six to spare. A quotient closer than that
            # below a tie would be rounded twice here and disagree with the
            # exact oracle; these seeded rows hold none.
            u = _unscaled(_dec(x, s1) / _dec(y, s2), out_scale)
            exp = None if abs(u) >= 10**prec else u
            assert o_div(x, y, *cfg) == exp, (x, y)


@pytest.mark.parametrize("cfg", INTDIV_CONFIGS, ids=_ids(INTDIV_CONFIGS))
def test_oracle_integer_divide_vs_decimal(cfg):
    s1, s2 = cfg
    with localcontext() as ctx:
        ctx.prec, ctx.rounding = 120, ROUND_HALF_UP
        for x, y in _rows(13):
            if y == 0:
                assert o_intdiv(x, y, *cfg) is None
                continue
            u = int(_dec(x, s1) // _dec(y, s2))  # truncates toward zero
            exp = None if abs(u) >= 10**38 else u
            assert o_intdiv(x, y, *cfg) == exp, (x, y)


@pytest.mark.parametrize("cfg", REM_CONFIGS, ids=_ids(REM_CONFIGS))
def test_oracle_remainder_vs_decimal(cfg):
    s1, s2 = cfg
    with localcontext() as ctx:
        ctx.prec, ctx.rounding = 120, ROUND_HALF_UP
        for x, y in _rows(14):
            if y == 0:
                assert o_rem(x, y, *cfg) is None
                continue
            r = _dec(x, s1) % _dec(y, s2)  # sign of the dividend, exact
            assert o_rem(x, y, *cfg) == int(r.scaleb(max(s1, s2))), (x, y)


@pytest.mark.parametrize("cfg", ADD_CONFIGS, ids=_ids(ADD_CONFIGS))
def test_oracle_add_subtract_vs_decimal(cfg):
    s1, s2, prec = cfg
    s = max(s1, s2)
    with localcontext() as ctx:
        ctx.prec, ctx.rounding = 120, ROUND_HALF_UP
        for x, y in _rows(15):
            for oracle, d in ((o_add, _dec(x, s1) + _dec(y, s2)),
                              (o_sub, _dec(x, s1) - _dec(y, s2))):
                u = int(d.scaleb(s))
                exp = None if abs(u) >= 10**prec else u
                assert oracle(x, y, *cfg) == exp, (x, y)


def test_oracle_half_up():
    assert [half_up(n, 2) for n in (1, -1, 3, -3, 2, 0)] == [1, -1, 2, -2, 1, 0]
    assert half_up(5, -10) == -1 and half_up(-5, -10) == 1
    assert half_up(49, 100) == 0 and half_up(-49, 100) == 0
    assert half_up(10**40 + 5 * 10**19 - 1, 10**20) == 10**20
    assert half_up(10**40 + 5 * 10**19, 10**20) == 10**20 + 1


def test_random_cases_keep_enough_non_null_rows():
    """The 30% floor of every random case, checked without a GPU."""
    for cfg in MUL_CONFIGS:
        _case(1, MUL_CONFIGS, cfg, o_mul, mul_bits)
    for cfg in DIV_CONFIGS:
        _case(2, DIV_CONFIGS, cfg, o_div)
    for cfg in INTDIV_CONFIGS:
        _case(3, INTDIV_CONFIGS, cfg, o_intdiv)
    for cfg in REM_CONFIGS:
        _case(4, REM_CONFIGS, cfg, o_rem)
    for cfg in ADD_CONFIGS:
        _case(5, ADD_CONFIGS, cfg, o_add, add_bits)
        _case(6, ADD_CONFIGS, cfg, o_sub, add_bits)


# ---------------------------------------------------------------------------
# CPU tier: Spark's result types. Expected values are worked out by hand from
# Spark's rule: precision capped at 38; the scale gives up the digits that
# the integral part needs, but not below min(scale, 6).
# ---------------------------------------------------------------------------
def test_adjust():
    from spark_rapids_jni_amd.ops.decimal import _adjust
    assert _adjust(38, 10) == (38, 10)    # at the cap: unchanged
    assert _adjust(21, 4) == (21, 4)
    assert _adjust(39, 0) == (38, 0)      # 39 integral digits, no scale to give
    assert _adjust(50, 30) == (38, 18)    # 20 integral digits leave 18
    assert _adjust(45, 6) == (38, 6)      # 39 integral digits: floor of 6
    assert _adjust(60, 4) == (38, 4)      # floor is min(scale, 6) = 4
    assert _adjust(77, 20) == (38, 6)


def test_multiply_result_type():
    from spark_rapids_jni_amd.ops.decimal import multiply_result_type
    # p1 + p2 + 1, s1 + s2
    assert multiply_result_type(10, 2, 10, 2) == (21, 4)
    assert multiply_result_type(18, 0, 19, 0) == (38, 0)
    assert multiply_result_type(38, 10, 38, 10) == (38, 6)    # (77, 20)
    assert multiply_result_type(38, 38, 38, 38) == (38, 37)   # (77, 76)
    assert multiply_result_type(20, 3, 20, 3) == (38, 6)      # (41, 6)
    assert multiply_result_type(20, 2, 20, 2) == (38, 4)      # (41, 4)


def test_divide_result_type():
    from spark_rapids_jni_amd.ops.decimal import divide_result_type
    # scale = max(6, s1 + p2 + 1); precision = p1 - s1 + s2 + scale
    assert divide_result_type(10, 2, 5, 0) == (16, 8)
    assert divide_result_type(5, 0, 3, 0) == (11, 6)
    assert divide_result_type(38, 10, 38, 10) == (38, 6)      # (87, 49)
    assert divide_result_type(38, 0, 38, 38) == (38, 6)       # (115, 39)
    assert divide_result_type(20, 10, 10, 0) == (31, 21)
    assert divide_result_type(30, 10, 10, 5) == (38, 13)      # (46, 21)


def test_add_result_type():
    from spark_rapids_jni_amd.ops.decimal import add_result_type
    # scale = max(s1, s2); precision = max(p1 - s1, p2 - s2) + scale + 1
    assert add_result_type(10, 2, 10, 2) == (11, 2)
    assert add_result_type(20, 2, 10, 5) == (24, 5)
    assert add_result_type(38, 10, 38, 10) == (38, 9)         # (39, 10)
    assert add_result_type(38, 0, 38, 38) == (38, 6)          # (77, 38)
    assert add_result_type(38, 3, 38, 3) == (38, 3)           # (39, 3): floor 3
    assert add_result_type(37, 0, 10, 0) == (38, 0)


# ---------------------------------------------------------------------------
# CPU tier: the kernels' per-row arithmetic, built for the host
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_rows(tmp_path_factory):
    """Builds tests/dec128_host_check.cpp around src/gpu/decimal128_core.hpp;
    returns a function from rows of its input format to its results."""
    exe = tmp_path_factory.mktemp("dec128") / "dec128_host_check"
    subprocess.run(
        [os.environ.get("CXX", "g++"), "-O2", "-std=c++17",
         "-I" + os.path.join(ROOT, "src", "gpu"),
         os.path.join(ROOT, "tests", "dec128_host_check.cpp"), "-o", str(exe)],
        check=True)

    def run(rows):
        text = "".join(" ".join(map(str, r + (0,) * (7 - len(r)))) + "\n"
                       for r in rows)
        out = subprocess.run([str(exe)], input=text, capture_output=True,
                             text=True, check=True).stdout.split()
        assert len(out) == len(rows)
        return [None if v == "null" else int(v) for v in out]

    return run


def _host_row(op, x, y, s1, s2, out_scale, precision):
    """One row in the driver's format, with the arguments that
    ops/decimal.py hands the kernels for this operation."""
    s = max(s1, s2)
    return {"mul": (0, x, y, s1 + s2, out_scale, precision),
            "div": (1, x, y, s1, s2, out_scale, precision),
            "intdiv": (2, x, y, s1, s2, 38),
            "rem": (3, x, y, s - s1, s - s2),
            "add": (4, x, y, s - s1, s - s2, precision),
            "sub": (5, x, y, s - s1, s - s2, precision)}[op]


def _host_cases():
    """(op, s1, s2, out_scale, precision, xs, ys, expected) of every random
    case of the GPU tier"""
    for cfg in MUL_CONFIGS:
        yield ("mul",) + cfg + _case(1, MUL_CONFIGS, cfg, o_mul, mul_bits)
    for cfg in DIV_CONFIGS:
        yield ("div",) + cfg + _case(2, DIV_CONFIGS, cfg, o_div)
    for cfg in INTDIV_CONFIGS:
        yield ("intdiv",) + cfg + (0, 38) + _case(3, INTDIV_CONFIGS, cfg,
                                                  o_intdiv)
    for cfg in REM_CONFIGS:
        yield ("rem",) + cfg + (0, 38) + _case(4, REM_CONFIGS, cfg, o_rem)
    for (s1, s2, p) in ADD_CONFIGS:
        yield ("add", s1, s2, 0, p) + _case(5, ADD_CONFIGS, (s1, s2, p),
                                            o_add, add_bits)
        yield ("sub", s1, s2, 0, p) + _case(6, ADD_CONFIGS, (s1, s2, p),
                                            o_sub, add_bits)


def test_host_build_random_cases(host_rows):
    rows, want, where = [], [], []
    for op, s1, s2, out_scale, prec, xs, ys, exp in _host_cases():
        for x, y, e in zip(xs, ys, exp):
            if x is not None and y is not None:
                rows.append(_host_row(op, x, y, s1, s2, out_scale, prec))
                want.append(e)
                where.append((op, s1, s2, out_scale, prec, x, y))
    got = host_rows(rows)
    bad = [i for i in range(len(rows)) if got[i] != want[i]]
    assert not bad, (f"{len(bad)} of {len(rows)} rows differ; first "
                     f"{where[bad[0]]}: got {got[bad[0]]}, expected "
                     f"{want[bad[0]]}")


def test_host_build_named_rows(host_rows):
    named = _named_rows()
    got = host_rows([_host_row(op, x, y, s1, s2, out_scale, prec)
                     for _, op, x, s1, y, s2, out_scale, prec, _ in named])
    failures = [f"{row[0]}: got {g}, expected {row[-1]}"
                for row, g in zip(named, got) if g != row[-1]]
    assert not failures, "\n".join(failures)


def test_host_build_int128_extremes(host_rows):
    """-2^127 has no positive counterpart; nothing may negate it as a signed
    value. It is outside every precision, so results that hold it are null,
    but its remainder and its quotients are ordinary values."""
    lo = -2**127
    got = host_rows([
        _host_row("add", lo, 0, 0, 0, 0, 38),
        _host_row("add", lo, lo, 0, 0, 0, 38),
        _host_row("sub", lo, 2**127 - 1, 0, 0, 0, 38),
        _host_row("mul", lo, 1, 0, 0, 0, 38),
        _host_row("mul", lo, lo, 38, 38, 0, 38),     # 2^254 / 10^76
        _host_row("div", lo, lo, 0, 0, 6, 38),
        _host_row("div", lo, 10**10, 0, 0, 0, 38),
        _host_row("intdiv", lo, -3, 0, 0, 0, 38),
        _host_row("rem", lo, 10**37, 0, 0, 0, 38),
        _host_row("rem", 7, lo, 0, 0, 0, 38),
    ])
    assert got == [None, None, None, None, half_up(2**254, 10**76), 10**6,
                   -half_up(2**127, 10**10), 2**127 // 3, -(2**127 % 10**37),
                   7]


# ---------------------------------------------------------------------------
# GPU tier
# ---------------------------------------------------------------------------
def _words(vals):
    """int64 words (low, high per row) of the unscaled values, None as 0."""
    u = [(v or 0) & (2**128 - 1) for v in vals]
    w = np.empty(2 * len(u), dtype=np.uint64)
    w[0::2] = [v & (2**64 - 1) for v in u]
    w[1::2] = [v >> 64 for v in u]
    return w.view(np.int64)


def _bits(valid):
    """validity buffer (whole 64-bit words) of a bool sequence"""
    buf = np.zeros(validity_nbytes(len(valid)), dtype=np.uint8)
    packed = np.packbits(np.asarray(valid, dtype=bool), bitorder="little")
    buf[:packed.size] = packed
    return buf


def _column(words, bits, n, scale):
    data = torch.from_numpy(np.ascontiguousarray(words)).cuda()
    validity = None if bits is None else torch.from_numpy(bits).cuda()
    return Column(DType.DECIMAL128, n, data, validity, scale=scale,
                  null_count=None)


def _col(vals, scale, mask=None):
    """mask=None: a validity mask only when there are nulls."""
    valid = [v is not None for v in vals]
    if mask is None:
        mask = not all(valid)
    assert mask or all(valid)
    return _column(_words(vals), _bits(valid) if mask else None, len(vals),
                   scale)


def _cols(xs, ys, s1, s2, mask):
    return (_col(xs, s1, mask in ("a", "both")),
            _col(ys, s2, mask in ("b", "both")))


def _result(col):
    """values of a result column, None for null; only the first n validity
    bits mean anything"""
    n = col.size
    words = col.data.cpu().numpy().view(np.uint64).tolist()
    valid = np.unpackbits(col.validity.cpu().numpy(), bitorder="little")[:n]
    out = []
    for i in range(n):
        u = (words[2 * i + 1] << 64) | words[2 * i]
        out.append((u - 2**128 if u >= 2**127 else u) if valid[i] else None)
    return out


def _compare(got_col, xs, ys, exp, what):
    assert got_col.size == len(exp)
    got = _result(got_col)
    bad = [i for i in range(len(exp)) if got[i] != exp[i]]
    assert not bad, (
        f"{what}: {len(bad)} of {len(exp)} rows differ; first at row "
        f"{bad[0]}: a={xs[bad[0]]} b={ys[bad[0]]} got {got[bad[0]]} "
        f"expected {exp[bad[0]]}")


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", MUL_CONFIGS, ids=_ids(MUL_CONFIGS))
def test_multiply_exact(cfg):
    from spark_rapids_jni_amd.ops.decimal import multiply_128
    s1, s2, out_scale, prec = cfg
    xs, ys, exp = _case(1, MUL_CONFIGS, cfg, o_mul, mul_bits)
    a, b = _cols(xs, ys, s1, s2, _mask_of(MUL_CONFIGS.index(cfg)))
    _compare(multiply_128(a, b, out_scale, prec), xs, ys, exp, "multiply")


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", DIV_CONFIGS, ids=_ids(DIV_CONFIGS))
def test_divide_exact(cfg):
    from spark_rapids_jni_amd.ops.decimal import divide_128
    s1, s2, out_scale, prec = cfg
    xs, ys, exp = _case(2, DIV_CONFIGS, cfg, o_div)
    a, b = _cols(xs, ys, s1, s2, _mask_of(DIV_CONFIGS.index(cfg)))
    _compare(divide_128(a, b, out_scale, prec), xs, ys, exp, "divide")


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", INTDIV_CONFIGS, ids=_ids(INTDIV_CONFIGS))
def test_integer_divide_exact(cfg):
    from spark_rapids_jni_amd.ops.decimal import integer_divide_128
    xs, ys, exp = _case(3, INTDIV_CONFIGS, cfg, o_intdiv)
    a, b = _cols(xs, ys, *cfg, _mask_of(INTDIV_CONFIGS.index(cfg)))
    got = integer_divide_128(a, b)
    assert got.scale == 0
    _compare(got, xs, ys, exp, "integer divide")


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", REM_CONFIGS, ids=_ids(REM_CONFIGS))
def test_remainder_exact(cfg):
    from spark_rapids_jni_amd.ops.decimal import remainder_128
    xs, ys, exp = _case(4, REM_CONFIGS, cfg, o_rem)
    a, b = _cols(xs, ys, *cfg, _mask_of(REM_CONFIGS.index(cfg)))
    got = remainder_128(a, b)
    assert got.scale == max(cfg)
    _compare(got, xs, ys, exp, "remainder")


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", ADD_CONFIGS, ids=_ids(ADD_CONFIGS))
def test_add_exact(cfg):
    from spark_rapids_jni_amd.ops.decimal import add_128
    s1, s2, prec = cfg
    xs, ys, exp = _case(5, ADD_CONFIGS, cfg, o_add, add_bits)
    a, b = _cols(xs, ys, s1, s2, _mask_of(ADD_CONFIGS.index(cfg)))
    got = add_128(a, b, prec)
    assert got.scale == max(s1, s2)
    _compare(got, xs, ys, exp, "add")


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", ADD_CONFIGS, ids=_ids(ADD_CONFIGS))
def test_subtract_exact(cfg):
    from spark_rapids_jni_amd.ops.decimal import subtract_128
    s1, s2, prec = cfg
    xs, ys, exp = _case(6, ADD_CONFIGS, cfg, o_sub, add_bits)
    a, b = _cols(xs, ys, s1, s2, _mask_of(ADD_CONFIGS.index(cfg)))
    _compare(subtract_128(a, b, prec), xs, ys, exp, "subtract")


# -- named rows -------------------------------------------------------------
def _product_ending(tail, drop):
    """x, y with x * y = tail modulo 10^drop, both below 10^38"""
    if tail == 5 * 10**(drop - 1):
        # 5^drop * 2^(drop-1) times an odd number ends in 5000...
        return 3 * 5**drop, 12345677 * 2**(drop - 1)
    y = 10**10 + 1
    while True:
        if y % 5:
            x = tail * pow(y, -1, 10**drop) % 10**drop
            if x + 987654321 * 10**drop <= MAXV:
                return x + 987654321 * 10**drop, y  # same tail, more digits
            if x <= MAXV:
                return x, y
        y += 2


def _named_rows():
    """(name, op, x, s1, y, s2, out_scale, precision, expected)"""
    rows = [
        # the five defects this suite was written against
        ("add: rescale overflow 7e37@0 + 1@1", "add",
         7 * 10**37, 0, 1, 1, None, 38, None),
        ("add: 2^126 + 2^126 = 2^127", "add",
         2**126, 0, 2**126, 0, None, 38, None),
        ("intdiv: scaled divisor above 2^128", "intdiv",
         10**37, 20, 10**25, 38, None, 38, 10**30),
        ("rem: rescale above int128, 1e37@0 % 3@10", "rem",
         10**37, 0, 3, 10, None, 38, 10**47 % 3),
        # 10^9 / (7 * 10^4) = 14285.714...
        ("divide: e < 0, 1e9@10 / 7@0 at scale 6", "div",
         10**9, 10, 7, 0, 6, 38, 14286),
    ]
    # divide ties, e = 0: x = y*q + y/2 rounds away from zero, one less
    # rounds toward zero
    for y, q in ((2, 7), (10, 10**36), (2**64, 12345), (10**20, 10**17 - 1),
                 (2 * (10**37 - 1), 3)):
        for sx in (1, -1):
            for sy in (1, -1):
                sign = sx * sy
                rows.append((f"divide tie y={sy * y} q={q} sx={sx}", "div",
                             sx * (y * q + y // 2), 0, sy * y, 0, 0, 38,
                             sign * (q + 1)))
                rows.append((f"divide below tie y={sy * y} q={q} sx={sx}",
                             "div", sx * (y * q + y // 2 - 1), 0, sy * y, 0,
                             0, 38, sign * q))
    # multiply ties: the dropped digits are 5000... (up) or 4999... (down);
    # drop 1 is the single divide, 4 and 20 one chunk, 39 two chunks, 19 and
    # 20 sit either side of the 19-digit chunk
    for drop, s1, s2 in ((1, 1, 0), (4, 2, 2), (19, 10, 9), (20, 10, 10),
                         (39, 20, 19)):
        half = 5 * 10**(drop - 1)
        for tail, up in ((half, 1), (half - 1, 0)):
            x, y = _product_ending(tail, drop)
            for sign in (1, -1):
                rows.append((f"multiply drop={drop} tail={'5000' if up else '4999'} "
                             f"sign={sign}", "mul", sign * x, s1, y, s2, 0, 38,
                             sign * (x * y // 10**drop + up)))
    # results of exactly +-(10^38 - 1) are valid, +-10^38 are null
    for sign in (1, -1):
        rows += [
            (f"multiply to {sign}*(1e38-1)", "mul",
             sign * (10**19 - 1), 0, 10**19 + 1, 0, 0, 38, sign * MAXV),
            (f"multiply to {sign}*1e38", "mul",
             sign * 10**19, 0, 10**19, 0, 0, 38, None),
            (f"add to {sign}*(1e38-1)", "add",
             sign * 5 * 10**37, 0, sign * (5 * 10**37 - 1), 0, None, 38,
             sign * MAXV),
            (f"add to {sign}*1e38", "add",
             sign * MAXV, 0, sign, 0, None, 38, None),
            (f"add scaled to {sign}*(1e38-1)", "add",
             sign * (10**37 - 1), 0, sign * 9, 1, None, 38, sign * MAXV),
            (f"add scaled to {sign}*1e38", "add",
             sign * (10**37 - 1), 0, sign * 10, 1, None, 38, None),
            (f"divide to {sign}*(1e38-1)", "div",
             sign * MAXV, 0, 1, 0, 0, 38, sign * MAXV),
            (f"divide scaled to {sign}*(1e38-1)", "div",
             sign * MAXV, 0, 10, 1, 0, 38, sign * MAXV),
            (f"divide to {sign}*1e38", "div",
             sign * 10**37, 0, 1, 1, 0, 38, None),
            (f"divide by zero, x={sign}", "div", sign, 0, 0, 0, 6, 38, None),
            (f"remainder by zero, x={sign}", "rem", sign, 2, 0, 4, None, 38,
             None),
            (f"integer divide by zero, x={sign}", "intdiv", sign, 2, 0, 4,
             None, 38, None),
        ]
    return rows


NAMED_ORACLES = {
    "mul": lambda x, s1, y, s2, o, p: o_mul(x, y, s1, s2, o, p),
    "div": lambda x, s1, y, s2, o, p: o_div(x, y, s1, s2, o, p),
    "intdiv": lambda x, s1, y, s2, o, p: o_intdiv(x, y, s1, s2),
    "rem": lambda x, s1, y, s2, o, p: o_rem(x, y, s1, s2),
    "add": lambda x, s1, y, s2, o, p: o_add(x, y, s1, s2, p),
}


def test_named_rows_agree_with_oracle():
    """The expected values of the named rows are worked out by hand; the
    oracle has to give the same."""
    for name, op, x, s1, y, s2, out_scale, prec, exp in _named_rows():
        assert abs(x) <= MAXV and abs(y) <= MAXV, name
        assert NAMED_ORACLES[op](x, s1, y, s2, out_scale, prec) == exp, name


def _run_named(op, x, s1, y, s2, out_scale, prec, ansi=False):
    from spark_rapids_jni_amd.ops import decimal as dec
    a, b = _col([x], s1), _col([y], s2)
    if op == "mul":
        return dec.multiply_128(a, b, out_scale, prec, ansi=ansi)
    if op == "div":
        return dec.divide_128(a, b, out_scale, prec, ansi=ansi)
    if op == "intdiv":
        return dec.integer_divide_128(a, b, ansi=ansi)
    if op == "rem":
        return dec.remainder_128(a, b, ansi=ansi)
    return dec.add_128(a, b, prec, ansi=ansi)


@pytest.mark.gpu
def test_named_rows():
    failures = []
    for name, op, x, s1, y, s2, out_scale, prec, exp in _named_rows():
        got = _result(_run_named(op, x, s1, y, s2, out_scale, prec))[0]
        if got != exp:
            failures.append(f"{name}: {x}@{s1} {op} {y}@{s2} -> {got}, "
                            f"expected {exp}")
    assert not failures, "\n".join(failures)


@pytest.mark.gpu
@pytest.mark.parametrize("op", ["div", "rem", "intdiv"])
def test_zero_divisor_ansi_reports_the_row(op):
    from spark_rapids_jni_amd.ops import decimal as dec
    a, b = _col([6, 7, 8], 2), _col([3, 0, 0], 4)
    fn = {"div": lambda: dec.divide_128(a, b, 6, ansi=True),
          "rem": lambda: dec.remainder_128(a, b, ansi=True),
          "intdiv": lambda: dec.integer_divide_128(a, b, ansi=True)}[op]
    with pytest.raises(dec.DecimalOverflowError) as ei:
        fn()
    assert ei.value.row_with_error == 1


# -- launch shapes ----------------------------------------------------------
SHAPES = [0, 1, 63, 64, 65, 127, 257, 1000]


@functools.lru_cache(maxsize=None)
def _shape_case():
    xs, ys = operands(77, n=1000, mask="both")
    return (xs, ys, [o_mul(x, y, 3, 2, 4) for x, y in zip(xs, ys)],
            [o_add(x, y, 2, 4) for x, y in zip(xs, ys)])


@pytest.mark.gpu
@pytest.mark.parametrize("n", SHAPES)
def test_multiply_shapes(n):
    from spark_rapids_jni_amd.ops.decimal import multiply_128
    xs, ys, exp, _ = _shape_case()
    got = multiply_128(_col(xs[:n], 3, True), _col(ys[:n], 2, True), 4)
    _compare(got, xs[:n], ys[:n], exp[:n], f"multiply n={n}")


@pytest.mark.gpu
@pytest.mark.parametrize("n", SHAPES)
def test_add_shapes(n):
    from spark_rapids_jni_amd.ops.decimal import add_128
    xs, ys, _, exp = _shape_case()
    got = add_128(_col(xs[:n], 2, True), _col(ys[:n], 4, True))
    _compare(got, xs[:n], ys[:n], exp[:n], f"add n={n}")


@pytest.mark.gpu
def test_multiply_second_grid_stride_trip():
    """One row past 2048 workgroups of 256 threads, plus a ragged last wave:
    a 4,099-row pattern tiled, its oracle tiled the same way."""
    from spark_rapids_jni_amd.ops.decimal import multiply_128
    n, m = 2048 * 256 + 65, 4099
    xs, ys = operands(78, n=m, mask="both")
    exp = [o_mul(x, y, 3, 2, 4) for x, y in zip(xs, ys)]
    assert sum(e is not None for e in exp) >= 0.3 * m
    reps = -(-n // m)

    def tiled(vals):
        w = np.tile(_words(vals).reshape(m, 2), (reps, 1))[:n]
        v = np.tile(np.array([x is not None for x in vals]), reps)[:n]
        return w, v

    (xw, xv), (yw, yv), (ew, ev) = tiled(xs), tiled(ys), tiled(exp)
    a = _column(xw.reshape(-1), _bits(xv), n, 3)
    b = _column(yw.reshape(-1), _bits(yv), n, 2)
    got = multiply_128(a, b, 4)
    gv = np.unpackbits(got.validity.cpu().numpy(), bitorder="little")[:n]
    gw = got.data.cpu().numpy().reshape(n, 2)
    bad = np.flatnonzero(gv.astype(bool) != ev)
    assert bad.size == 0, f"validity differs at {bad.size} rows, first {bad[0]}"
    bad = np.flatnonzero(ev & (gw != ew).any(axis=1))
    assert bad.size == 0, f"data differs at {bad.size} rows, first {bad[0]}"


# -- ANSI -------------------------------------------------------------------
def _ansi_ops():
    from spark_rapids_jni_amd.ops import decimal as dec
    # op -> (call, a row that fails: (x, y))
    return {
        "multiply overflow": (
            lambda a, b, ansi: dec.multiply_128(a, b, 0, ansi=ansi),
            (10**37, 10**37)),
        "add overflow": (
            lambda a, b, ansi: dec.add_128(a, b, ansi=ansi), (MAXV, MAXV)),
        "divide by zero": (
            lambda a, b, ansi: dec.divide_128(a, b, 6, ansi=ansi), (5, 0)),
    }


@pytest.mark.gpu
@pytest.mark.parametrize("op", ["multiply overflow", "add overflow",
                                "divide by zero"])
def test_ansi_reports_the_first_failing_row(op):
    from spark_rapids_jni_amd.ops.decimal import DecimalOverflowError
    call, (fx, fy) = _ansi_ops()[op]
    n = 1000
    xs, ys = [i + 1 for i in range(n)], [3] * n
    for i in (700, 300, 999):  # three different workgroups
        xs[i], ys[i] = fx, fy
    # a null row ahead of them is not an error, whatever its data holds
    xs[100], ys[100] = fx, fy
    valid = [i != 100 for i in range(n)]

    def cols():
        return _column(_words(xs), _bits(valid), n, 0), _col(ys, 0)

    a, b = cols()
    with pytest.raises(DecimalOverflowError) as ei:
        call(a, b, True)
    assert ei.value.row_with_error == 300
    got = _result(call(a, b, False))
    assert [i for i in range(n) if got[i] is None] == [100, 300, 700, 999]

    for i in (700, 300, 999):
        xs[i], ys[i] = 1, 3
    got = _result(call(*cols(), True))  # nothing raised
    assert [i for i in range(n) if got[i] is None] == [100]
