"""bench.py --dump-outputs on a real MI355X: the files of two runs with the same arguments are equal bit for bit (same
seeded inputs, deterministic bf16 kernels), and the eager loop writes what the hipGraph replay writes for the same
number of training steps.  A plain run prints the headline line alone; --full runs the other legs behind the same timed
steps.  Small model (2 levels, 32 features, 32^3 patches); run with `-m gpu`.  The roofline leg of --full counts launches
with ops.Probe, which is ru3d_probe_begin / ru3d_probe_end."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no HIP device", allow_module_level=True)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("loss", "logits", "params", "grads")
NARROW = ("--no-probe", "--no-cpu-baseline", "--no-parity", "--no-torch-adam")
# what --full adds to the line: each from a run of its own behind the timed steps
LEGS = ("ms_per_step_eager", "host_enqueue_ms_per_step_eager", "roofline", "ms_per_step_torch_adam", "parity",
        "cpu_baseline")


def _bench(out, *extra, narrow=NARROW):
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    env.pop("RANK", None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--patch", "32", "--pools", "2", "--features",
           "32"] + list(narrow) + ["--dump-outputs", out] + list(extra)
    p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)
    assert p.returncode == 0, p.stderr.decode("utf-8", "replace")[-4000:]
    lines = [l for l in p.stdout.decode().splitlines() if l.startswith("{")]
    assert len(lines) == 1, lines
    assert sorted(os.listdir(out)) == sorted(n + ".npy" for n in NAMES)
    assert sum(os.path.getsize(os.path.join(out, f)) for f in os.listdir(out)) <= 64 * 10 ** 6
    arrays = {n: np.load(os.path.join(out, n + ".npy")) for n in NAMES}
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in arrays.values())
    return json.loads(lines[0]), arrays


def test_dump_outputs_repeats_bit_for_bit_and_eager_equals_replay(tmp_path):
    rec_a, a = _bench(str(tmp_path / "a"), "--steps", "2", "--warmup", "1")
    rec_b, b = _bench(str(tmp_path / "b"), "--steps", "2", "--warmup", "1")
    assert rec_a["steps"] == 2 and "hipGraph" in rec_a["step_launch"]
    assert a["logits"].shape == (2, 3, 32, 32, 32) and a["loss"][0] == np.float32(rec_a["final_loss"])
    assert np.abs(a["grads"]).max() > 0 and np.abs(a["logits"]).max() > 0
    for n in NAMES:
        assert np.array_equal(a[n], b[n]), n
    # the graphed loop takes one more step than --warmup before the timed ones (the captured step's first replay):
    # two steps in front of the two timed ones either way
    rec_e, e = _bench(str(tmp_path / "e"), "--steps", "2", "--warmup", "2", "--launch", "eager")
    assert rec_e["step_launch"].startswith("eager")
    for n in NAMES:
        assert np.array_equal(a[n], e[n]), n
    # one more timed step is one more Adam update
    rec_c, c = _bench(str(tmp_path / "c"), "--steps", "3", "--warmup", "1")
    assert rec_c["steps"] == 3 and not np.array_equal(a["params"], c["params"])


def test_plain_run_prints_the_headline_alone_and_full_adds_the_other_legs_behind_the_same_steps(tmp_path):
    rec_p, p = _bench(str(tmp_path / "p"), "--steps", "2", "--warmup", "1", narrow=())
    rec_f, f = _bench(str(tmp_path / "f"), "--steps", "2", "--warmup", "1", "--full", narrow=())
    for rec in (rec_p, rec_f):
        assert rec["metric"].startswith("train voxels/sec (32^3 patch, bs=2 per GPU)") and rec["unit"] == "voxels/s"
        assert rec["higher_is_better"] is True and rec["dtype"] == "bf16" and rec["steps"] == 2 and rec["warmup"] == 1
        assert rec["ms_per_step"] > 0 and abs(rec["value"] * rec["ms_per_step"] - 2 * 32 ** 3 * 1e3) < 1e-3 * 2 * 32 ** 3
        assert "hipGraph" in rec["step_launch"] and rec["roofline_step"]["alg_flops"] > 0
    assert not [k for k in LEGS if k in rec_p], rec_p
    assert not [k for k in LEGS if k not in rec_f], rec_f
    assert rec_f["ms_per_step_eager"] > 0 and rec_f["ms_per_step_torch_adam"] > 0
    assert rec_f["roofline"]["launches"] > 0 and rec_f["roofline"]["avg_ms"] > 0
    assert "error" not in rec_f["parity"] and all(len(rec_f["parity"][k]["dice_vs_cpu_ref"]) == 3 for k in ("bf16", "fp32"))
    assert rec_f["cpu_baseline"]["value"] > 0
    # the legs run behind the timed steps and the dump: both runs took the same steps
    assert rec_p["final_loss"] == rec_f["final_loss"]
    for n in NAMES:
        assert np.array_equal(p[n], f[n]), n
    # the options that narrow --full still do
    rec_n, _ = _bench(str(tmp_path / "n"), "--steps", "2", "--warmup", "1", "--full")
    assert [k for k in LEGS if k in rec_n] == ["ms_per_step_eager", "host_enqueue_ms_per_step_eager"], rec_n
