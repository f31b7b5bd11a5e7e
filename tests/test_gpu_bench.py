"""bench.py --dump-outputs on a real MI355X: the files of two runs with the same arguments are equal bit for bit (same
seeded inputs, deterministic bf16 kernels), and the eager loop writes what the hipGraph replay writes for the same
number of training steps.  Small model (2 levels, 32 features, 32^3 patches); run with `-m gpu`."""
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


def _bench(out, *extra):
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    env.pop("RANK", None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--patch", "32", "--pools", "2", "--features",
           "32", "--no-probe", "--no-cpu-baseline", "--no-parity", "--no-torch-adam", "--dump-outputs", out] + list(extra)
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
