"""bench.py --dump-outputs on the GPU: a plain run writes its last step's outputs, and they are
what a caller of the same GpuRound.run over the same instances receives.

70 000 instances: more than bench.DUMP_SAMPLE, so the seeded sampling path runs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNT = 70_000
NAMES = ("summary", "fail_count", "term_hist", "digest", "sample_ids", "decision", "decision_round")


def _bench(out_dir, *extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
           "--instances", str(COUNT), "--dump-outputs", str(out_dir), *extra]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=110)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0]), {k: np.load(os.path.join(out_dir, k + ".npy")) for k in NAMES}


def test_full_run_adds_variants_and_cpu_baseline(tmp_path):
    line, _ = _bench(tmp_path / "f", "--full", "--variants", "2", "--cpu-seconds", "0.3")
    assert line["full"] is True and line["ms_per_step"] > 0
    assert list(line["variants"]) == ["V=2"] and line["variants"]["V=2"]["value"] > 0
    assert all(v == 0 for v in line["variants"]["V=2"]["violations"].values())
    assert line["cpu_baseline"]["value"] > 0 and line["cpu_baseline"]["single_core"]["value"] > 0


def test_plain_run_dumps_what_the_timed_path_returned(tmp_path):
    sys.path.insert(0, ROOT)
    import bench
    from round_amd import psync
    line, got = _bench(tmp_path / "a")
    # the plain line: the headline fields, and nothing that takes runs of its own
    assert line["steps"] == 2 and line["warmup"] == 1 and line["full"] is False
    assert line["ms_per_step"] > 0 and line["higher_is_better"] is True and line["dtype"] == "int32"
    assert line["value"] == pytest.approx(COUNT * 64 * 20 / (line["ms_per_step"] * 1e-3), rel=1e-9)
    assert line["variants"] is None and line["cpu_baseline"] is None and "profile" not in line["roofline"]
    assert sorted(os.listdir(tmp_path / "a")) == sorted(k + ".npy" for k in NAMES)
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= 64 << 20
    # the same batch run here
    with psync.GpuRound(psync.OTR(), 64, rounds=20, seed=2, value_range=64,
                        schedule=psync.HOSchedule(drop_log2=3, good_round=0.25), device=0,
                        batch_capacity=COUNT) as gr:
        s = gr.run(0, COUNT).summary
        dec, dr = gr._ctx.copy_decisions_np()
    assert got["summary"].tolist() == [s.instances, s.process_rounds, s.active_process_rounds,
                                       s.live_instance_rounds, s.decided_processes]
    assert got["fail_count"].tolist() == list(s.fail_count)
    assert got["term_hist"].tolist() == [s.term_hist[i] for i in range(22)]
    assert got["digest"].tolist() == bench._limbs16(int(s.digest))
    rows = got["sample_ids"].astype(np.int64)
    assert rows.shape == (bench.DUMP_SAMPLE,) and (np.diff(rows) > 0).all() and 0 <= rows[0] and rows[-1] < COUNT
    assert got["decision"].shape == got["decision_round"].shape == (bench.DUMP_SAMPLE, 64)
    assert (got["decision"] == dec[rows]).all() and (got["decision_round"] == dr[rows]).all()
    assert (dr[rows] >= 0).sum() > 0  # some process of the sample decided
    # same arguments, same inputs, same sample: a second run writes the same arrays
    _, again = _bench(tmp_path / "b")
    for k in NAMES:
        assert (got[k] == again[k]).all(), k
