"""bench.py's command line, two runs of three steps each in the deterministic mode:

* plain: --steps 2 --warmup 1 — the result line without the probes and the CPU baseline;
* full:  --steps 3 --warmup 0 --full --no-cpu-baseline — the roofline object with its probes.

The dumped device step counter (step.npy) reads warmup + steps, so with no warm-up it counts the
timed steps alone: the timed loop runs exactly --steps steps. Both runs took three steps from the
same inputs, so their dumps (loss, the seeded parameter sample) are equal bit for bit."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCH = 64


def _bench(out_dir, *args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--batch",
                        str(BATCH), "--deterministic", "--dump-outputs", str(out_dir), *args],
                       capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    dump = {f[:-4]: np.load(os.path.join(out_dir, f)) for f in sorted(os.listdir(out_dir))}
    return json.loads(lines[0]), dump


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    d = tmp_path_factory.mktemp("bench_cli")
    return (_bench(d / "plain", "--steps", "2", "--warmup", "1"),
            _bench(d / "full", "--steps", "3", "--warmup", "0", "--full", "--no-cpu-baseline"))


def test_plain_result_line(runs):
    line, _ = runs[0]
    assert line["steps"] == 2 and line["warmup"] == 1 and line["ms_per_step"] > 0
    assert line["unit"] == "samples/s" and line["higher_is_better"] is True and line["dtype"] == "bf16"
    assert abs(line["value"] - BATCH * 1e3 / line["ms_per_step"]) <= 1e-3 * line["value"]
    assert line["roofline"] is None and line["cpu_baseline"] is None   # --full only


def test_full_adds_probes(runs):
    line, _ = runs[1]
    assert line["steps"] == 3 and line["warmup"] == 0 and line["ms_per_step"] > 0
    roof = line["roofline"]
    assert roof["avg_launch_us"] > 0 and 0 < roof["frac"] < 1          # the mlp_dw headline probe
    names = {k["name"] for k in roof["kernels"]}
    assert {"mlp_up_fwd", "attn_fwd", "attn_bwd", "tome_match", "seqnorm_fwd"} <= names
    assert all(k["avg_launch_us"] > 0 for k in roof["kernels"])
    assert line["cpu_baseline"] is None                                # --no-cpu-baseline


def test_dump_counts_steps_and_reproduces(runs):
    (pl, a), (fl, b) = runs
    assert sorted(a) == sorted(b) == ["loss", "params", "step"]
    assert a["loss"].dtype == a["params"].dtype == np.float32 and a["step"].dtype == np.float64
    assert sum(x.nbytes for x in a.values()) <= 64 * 2 ** 20
    assert a["params"].size > 0 and np.isfinite(a["params"]).all() and np.isfinite(a["loss"]).all()
    assert b["step"].tolist() == [3.0]      # no warm-up: the timed loop alone took --steps steps
    assert a["step"].tolist() == [3.0]      # 1 warm-up + 2 timed
    for k in ("loss", "params"):            # same inputs, same three steps: bit-equal outputs
        np.testing.assert_array_equal(a[k], b[k])
    assert float(a["loss"][0]) == pytest.approx(pl["final_loss"], abs=1e-5)
    assert pl["final_loss"] == fl["final_loss"]
