"""bench.py end to end at a small size, in fresh processes: a plain run prints the headline line and nothing measured beside it;
--full adds every block it measured before the option existed, each without an error."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--steps", "2", "--warmup", "1", "--genomes", "4", "--genome-len", "200000", "--queries", "1000000"]
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "parity_ok", "present_fraction")
FULL_ONLY = ("roofline", "footprint", "cpu_baseline", "container_walk", "k31", "config2", "sequence_queries", "insert", "dist_path_check")


def _bench(args, timeout):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_plain_run_prints_the_headline_alone(tmp_path):
    d = _bench(SMALL + ["--dump-outputs", str(tmp_path)], 300)
    assert all(k in d for k in HEADLINE), d.keys()
    assert d["steps"] == 2 and d["warmup"] == 1 and d["parity_ok"] is True and d["value"] > 0 and d["ms_per_step"] > 0
    assert not [k for k in FULL_ONLY if k in d]
    assert d["dumped_outputs"]["queries"] == 1_000_000
    p = np.load(tmp_path / "presence.npy")
    assert p.dtype == np.float32 and len(p) == 1_000_000 and abs(float(p.mean()) - d["present_fraction"]) < 1e-3


def test_full_run_measures_every_block():
    d = _bench(SMALL + ["--full"], 600)
    assert all(k in d for k in HEADLINE) and d["parity_ok"] is True
    assert all(k in d for k in FULL_ONLY), [k for k in FULL_ONLY if k not in d]
    assert not [k for k in FULL_ONLY if "error" in d[k]], {k: d[k].get("error") for k in FULL_ONLY}
    assert d["oracle_parity_ok"] is True and d["dist_path_check"]["ok"] is True
    assert d["k31"]["all_answers_checked"] and d["config2"]["all_answers_checked"]
