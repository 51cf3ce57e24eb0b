"""-m gpu: bench.py's plain run (the headline leg only) and --dump-outputs.  The dumped MSM is the result the line hashes, it is the
same result the --full run checks against its closed form, and the same arguments give the same bytes again."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOG_N, STEPS = 14, 3


def _lines(args):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--steps", str(STEPS), "--warmup", "1", "--log-n", str(LOG_N)] + args
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    return [json.loads(l) for l in out.stdout.splitlines() if l.startswith("{")]


def _dumped(d):
    got = np.load(os.path.join(d, "msm_result.npy"))
    assert got.dtype == np.float64 and got.shape == (96,) and ((got >= 0) & (got <= 255) & (got == np.round(got))).all()
    return bytes(got.astype(np.uint8))


def test_plain_run_is_the_headline_leg_and_dumps_its_result(tmp_path):
    lines = _lines(["--dump-outputs", str(tmp_path / "plain")])
    assert len(lines) == 1
    line = lines[0]
    assert line["metric"] == "g1_msm_scalar_muls_per_s" and line["unit"] == "scalar-muls/s" and line["higher_is_better"] is True
    assert line["steps"] == STEPS and line["legs_finished"] == ["weak_msm"] and line["provisional"] is False
    assert line["value"] * line["ms_per_step"] * 1e-3 == pytest.approx(1 << LOG_N, rel=1e-9)
    assert line["config"]["srs_tables"]["used"] is True
    for leg in ("ntt", "strong_scaling", "prove", "pipelined", "msm_without_tables", "cpu_baseline", "other_sizes", "equals_closed_form"):
        assert line.get(leg) is None, leg
    res = _dumped(tmp_path / "plain")
    assert hashlib.sha256(res).hexdigest()[:16] == line["result_sha"]
    # the same MSM in a --full run: checked against its closed form there, and the same bytes dumped
    full = _lines(["--full", "--skip-cpu", "--skip-seams", "--skip-pipelined", "--other-sizes", "--ntt-log-n", "14", "--strong-log-n", "0",
                   "--prove-log-n", "0", "--dump-outputs", str(tmp_path / "full")])[-1]
    assert full["equals_closed_form"] is True and full["result_sha"] == line["result_sha"] and full["msm_without_tables"]["value"] > 0
    assert _dumped(tmp_path / "full") == res


def test_plain_run_two_ranks_rehearsal(tmp_path):
    """the plain run under the launcher (gloo, two ranks on this card): one provisional and one final line, rank 0 alone dumps"""
    lines = _lines(["--gpus", "2", "--backend", "gloo", "--dump-outputs", str(tmp_path / "two")])
    assert [l["provisional"] for l in lines] == [True, False] and all(l["legs_finished"] == ["weak_msm"] for l in lines)
    assert lines[-1]["n_gpus"] == 2 and lines[-1]["value"] > 0 and lines[-1].get("ntt_columns") is None
    assert hashlib.sha256(_dumped(tmp_path / "two")).hexdigest()[:16] == lines[-1]["result_sha"]
