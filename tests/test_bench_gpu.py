"""bench.py's own contract on a small workload: a plain run prints the headline line only, --dump-outputs writes the last
timed step's game records and repeats array for array from run to run, --full adds the roofline pass and the companion legs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

SMALL = ["--gpus", "1", "--slots", "256", "--playouts", "50", "--blocks", "2", "--steps", "2", "--warmup", "1"]


def _bench(flags):
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + SMALL + flags, env=env, capture_output=True,
                         text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout[-3000:]
    return json.loads(lines[0])


def test_plain_run_dumps_the_last_step_and_repeats(tmp_path):
    runs = []
    for i in range(2):
        d = tmp_path / ("run%d" % i)
        line = _bench(["--dump-outputs", str(d)])
        assert line["steps"] == 2 and line["value"] > 0 and line["ms_per_step"] > 0 and line["higher_is_better"] is True
        assert not {"roofline", "roofline_tree", "opt_in_f16", "cpu_baseline"} & set(line)
        runs.append({f[:-4]: np.load(d / f) for f in sorted(os.listdir(d))})
    a, b = runs
    assert sorted(a) == ["child_action", "child_visits", "game_id", "game_len", "game_ret0", "move", "n_children", "states", "value"]
    assert sum(v.nbytes for v in a.values()) <= 64e6
    assert a["game_id"].tolist() == list(range(2 * 256, 3 * 256))  # the last step's games: ids (W+K-1)*G .. (W+K)*G-1
    assert (a["game_len"] > 0).all() and (a["child_visits"].sum(axis=2)[:, 0] > 0).all()
    for name in a:
        assert a[name].dtype in (np.float32, np.float64), name
        assert np.array_equal(a[name], b[name]), name


def test_full_run_adds_the_roofline_pass_and_the_companion_legs():
    line = _bench(["--full", "--cpu-baseline", "off", "--ref-seconds", "1", "--companion-steps", "1"])
    assert line["roofline"]["ms_per_launch"] > 0 and line["roofline_tree"]["ms_per_launch"] > 0
    assert line["opt_in_f16"]["steps"] == 1 and line["opt_in_f16"]["torch_fp32"]["value"] >= 0
