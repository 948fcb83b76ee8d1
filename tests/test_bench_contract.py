"""bench.py driver-contract guard: tiny-config runs must emit the JSON line
with every required field (the round-end driver depends on this shape)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

REQUIRED = {"metric", "value", "unit", "n_gpus", "steps", "warmup",
            "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
            "dtype", "data", "config"}


def _run(args):
    out = subprocess.run(
        [sys.executable, os.path.join(REPO, "bench.py")] + args,
        capture_output=True, text=True, timeout=420, cwd=REPO)
    assert out.returncode == 0, out.stderr[-2000:]
    line = out.stdout.strip().splitlines()[-1]
    d = json.loads(line)
    assert REQUIRED <= set(d), sorted(REQUIRED - set(d))
    assert d["n_gpus"] == 1 and d["value"] > 0
    return d


def test_join_contract_tiny():
    d = _run(["--build-rows", "1000000", "--probe-rows", "4000000",
              "--chunk-rows", "2000000", "--steps", "2", "--warmup", "1"])
    assert d["metric"] == "hash_join_probe_rows_per_sec"
    assert d["config"]["global_batch"] == 4000000


def test_groupby_contract_tiny():
    d = _run(["--op", "groupby", "--build-rows", "2000000", "--steps", "2",
              "--warmup", "1"])
    assert d["metric"] == "hash_aggregate_rows_per_sec"


def test_q3_contract_tiny():
    d = _run(["--op", "q3", "--probe-rows", "2000000", "--steps", "2",
              "--warmup", "1"])
    assert d["metric"] == "nds_q3_rows_per_sec"


def test_join_dump_outputs_tiny(tmp_path):
    """--dump-outputs writes the last timed step's join output in canonical
    order; with seeded inputs two runs give identical arrays. At this size
    the sample stride is 1, so the dump is the whole output: the build side
    is arange(build_rows) and every probe key hits exactly one build row."""
    tiny = ["--build-rows", "1000000", "--probe-rows", "2000001",
            "--chunk-rows", "1500000", "--steps", "2", "--warmup", "1"]
    dumps = []
    for name in ("a", "b"):
        d = _run(tiny + ["--full", "--dump-outputs", str(tmp_path / name)])
        assert d["steps"] == 2 and d["ms_per_step"] > 0
        dumps.append({f[:-4]: np.load(tmp_path / name / f)
                      for f in sorted(os.listdir(tmp_path / name))})
    a, b = dumps
    assert set(a) == {"build_idx", "probe_idx", "num_pairs", "pair_checksum"}
    assert sum(v.nbytes for v in a.values()) <= 64 * 10**6
    for k in a:
        assert a[k].dtype == np.float64
        assert np.array_equal(a[k], b[k]), k
    assert a["num_pairs"].tolist() == [1500000.0, 500001.0]
    assert np.array_equal(a["probe_idx"], np.arange(2000001, dtype=np.float64))
    bi = a["build_idx"].astype(np.int64)
    assert bi.min() >= 0 and bi.max() < 1000000
    assert len(np.unique(bi)) > 800000          # uniform keys, not a constant
    # checksum over all pairs agrees with the dumped pairs, chunk by chunk
    pi = a["probe_idx"].astype(np.int64)
    for c, (lo, hi) in enumerate([(0, 1500000), (1500000, 2000001)]):
        want = int(np.sum(bi[lo:hi] ^ (pi[lo:hi] - lo)))
        got = (int(a["pair_checksum"][c, 0]) << 32) \
            + int(a["pair_checksum"][c, 1])
        assert got == want
