"""bench.py as the driver runs it: a plain run times the steps and prints the headline only; --full adds the per-kernel
timings, the legs and the oracle checks; both dump the same answer of their last timed step (--dump-outputs).  Child
processes: bench.py owns its process's stdout and HIP runtime."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# one query set in the rotation: the last timed step answers the batch the --full run checks against the oracle
SMALL = ["--tweets", "2000000", "--queries-per-gpu", "128", "--steps", "3", "--warmup", "1", "--rotate", "1"]


def _bench(*extra):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *SMALL, *extra], capture_output=True, text=True,
                       timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_and_full_runs_dump_the_same_answer(tmp_path):
    plain = _bench("--dump-outputs", str(tmp_path / "plain"))
    full = _bench("--full", "--no-cpu-baseline", "--quality-topical-tweets", "0", "--mb-requests", "2048",
                  "--dump-outputs", str(tmp_path / "full"))
    for line in (plain, full):
        assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0 and line["value"] > 0
        assert line["unit"] == "candidates/sec" and line["higher_is_better"] is True and line["dtype"] == "f64"
        assert line["fallback_units"] == 0
    assert plain["metric"] == full["metric"]
    assert plain["full"] is False and full["full"] is True
    for key in ("roofline", "end_to_end", "micro_batched", "cpu_baseline", "recall_at_400_parity", "recall_at_400_quality"):
        assert plain[key] is None, key
    assert full["recall_at_400_parity"] == 1.0 and full["parity_checked_queries"] == 16
    assert full["roofline"]["kernel_avg_ms"] > 0 and full["end_to_end"]["equals_replayed_batch"] is True
    assert full["micro_batched"]["requests"] > 0

    names = sorted(os.listdir(str(tmp_path / "plain")))
    assert names == sorted(os.listdir(str(tmp_path / "full")))
    assert names == ["counts.npy", "map_sizes.npy", "query_index.npy", "scores.npy", "tweet_ids_hi32.npy", "tweet_ids_lo32.npy"]
    for n in names:
        a, b = np.load(str(tmp_path / "plain" / n)), np.load(str(tmp_path / "full" / n))
        assert a.dtype == np.float64 and np.array_equal(a, b), n
    counts = np.load(str(tmp_path / "plain" / "counts.npy"))
    assert counts.shape == (128,) and counts.max() <= 400 and counts.sum() > 0
    assert np.load(str(tmp_path / "plain" / "scores.npy")).shape == (128, 400)
