"""The wide, narrow and dense join tables share one probe kernel template:
every layout must give the pairs of a Python dict join on the CPU, compared
as sorted (probe_idx, build_idx) lists."""
import random

import pytest
import torch

from spark_rapids_jni_amd.columnar import Column

pytestmark = pytest.mark.gpu

INT64_MIN, INT64_MAX = -2**63, 2**63 - 1
LAYOUTS = {"wide": dict(narrow=False), "narrow": dict(narrow=True),
           "dense": dict(dense=True)}
# the edges of 8- and 16-row batches and of one wave iteration (64 lanes:
# 512 rows at batch 8, 1024 at batch 16)
PROBE_SIZES = [0, 1, 7, 8, 9, 15, 16, 17, 511, 512, 513, 1023, 1025]


def _col(vals, valid=None):
    return Column.from_torch(torch.tensor(vals, dtype=torch.int64,
                                          device="cuda"), valid)


def _oracle(bvals, bvalid, pvals, pvalid):
    rows = {}
    for i, k in enumerate(bvals):
        if bvalid is None or bvalid[i]:
            rows.setdefault(k, []).append(i)
    return sorted((j, i) for j, k in enumerate(pvals)
                  if pvalid is None or pvalid[j] for i in rows.get(k, ()))


def _pairs(bi, pi):
    return sorted(zip(pi.cpu().tolist(), bi.cpu().tolist()))


def _flags(ref, nbuild):
    f = [0] * nbuild
    for _, i in ref:
        f[i] = 1
    return f


@pytest.fixture(scope="module")
def unique_case():
    """300 unique build keys, a shuffled arange(-7, 293), 5 % of the rows null
    with their stored value left inside the range; per probe size a key list
    from [-27, 313) and a validity that nulls the first and last rows."""
    from spark_rapids_jni_amd.ops.join import HashJoinTable
    rnd = random.Random(11)
    bvals = list(range(-7, 293))
    rnd.shuffle(bvals)
    bvalid = [True] * 300
    for i in rnd.sample(range(300), 15):
        bvalid[i] = False
    b = _col(bvals, bvalid)
    tables = {name: HashJoinTable.build(b, **kw)
              for name, kw in LAYOUTS.items()}
    probes = []
    for n in PROBE_SIZES:
        pvals = [rnd.randrange(-27, 313) for _ in range(n)]
        pvalid = [rnd.random() > 0.1 for _ in range(n)]
        if n:
            pvalid[0] = pvalid[-1] = False
        for valid in (None, pvalid):
            probes.append((pvals, valid,
                           _oracle(bvals, bvalid, pvals, valid)))
    return tables, probes


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_layouts_agree_with_dict_join(unique_case, layout):
    tables, probes = unique_case
    tbl = tables[layout]
    assert tbl.layout == layout and tbl.num_build_rows == 300
    nonempty = 0
    for pvals, pvalid, ref in probes:
        p = _col(pvals, pvalid)
        assert (p.validity is not None) == (pvalid is not None)
        nonempty += bool(ref)
        # a third of the exact size forces the overflow rerun
        for hint in (None, len(ref), len(ref) // 3):
            assert _pairs(*tbl.inner_join(p, out_hint=hint)) == ref, (
                len(pvals), pvalid is not None, hint)
        bi, pi, matched = tbl.inner_join(p, track_build_matches=True)
        flags = _flags(ref, 300)
        assert _pairs(bi, pi) == ref
        assert matched.cpu().tolist() == flags
        # capacity-0 mark-only probe
        assert tbl.mark_matches(p).cpu().tolist() == flags
    assert nonempty >= 2 * (len(PROBE_SIZES) - 3)


@pytest.mark.parametrize("layout", ["wide", "narrow"])
def test_duplicate_build_keys(layout):
    """One batch of 8 probe rows mixes 0, 1 and many matches, and one key's
    chain (70 rows) is longer than a batch."""
    from spark_rapids_jni_amd.ops.join import HashJoinTable
    rnd = random.Random(29)
    # keys 0..9 once each, 190 rows over keys 10..39, then 70 rows of key 1000
    bvals = list(range(10)) + [rnd.randrange(10, 40) for _ in range(190)]
    rnd.shuffle(bvals)
    bvals += [1000] * 70
    pvals = [rnd.choice([rnd.randrange(-5, 60), rnd.randrange(0, 10), 1000])
             for _ in range(600)]
    ref = _oracle(bvals, None, pvals, None)
    per_row = {}
    for j, _ in ref:
        per_row[j] = per_row.get(j, 0) + 1
    assert {1, 70} <= set(per_row.values()) and len(per_row) < 600
    tbl = HashJoinTable.build(_col(bvals), **LAYOUTS[layout])
    assert tbl.layout == layout
    p = _col(pvals)
    for hint in (None, len(ref) // 3):
        assert _pairs(*tbl.inner_join(p, out_hint=hint)) == ref
    bi, pi, matched = tbl.inner_join(p, track_build_matches=True)
    assert _pairs(bi, pi) == ref
    assert matched.cpu().tolist() == _flags(ref, len(bvals))


def test_wide_keys_differing_in_the_high_half():
    from spark_rapids_jni_amd.ops.join import HashJoinTable

    def wrap(v):
        return (v - INT64_MIN) % 2**64 + INT64_MIN

    bvals = [INT64_MIN, INT64_MAX, 0, -1, 12345, 1 << 32, -(1 << 32)]
    pvals = list(bvals)
    for k in bvals:
        pvals += [wrap(k ^ (1 << 32)), wrap(k ^ (1 << 63)),
                  wrap(k + (1 << 32)), wrap(k ^ (0xffffffff << 32))]
    pvals += [INT64_MIN + 1, INT64_MAX - 1, 1, -2]
    ref = _oracle(bvals, None, pvals, None)
    assert len(bvals) <= len(ref) < len(pvals)
    tbl = HashJoinTable.build(_col(bvals), narrow=False)
    assert tbl.layout == "wide"
    assert _pairs(*tbl.inner_join(_col(pvals))) == ref
