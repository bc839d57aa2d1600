"""The bench's plain run and its ``--dump-outputs``: one small run (64x64 crops, batch 4) must print
the headline line without the ``--full`` legs, honour ``--steps``, and write the last timed step's
output, which is the forward of the same seeded inputs through the façade's context (bit for bit)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_prints_headline_and_dumps_outputs(tmp_path, mp):
    n, crop, T = 4, 64, 8
    dump = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3",
                        "--warmup", "1", "--batch", str(n), "--crop", str(crop), "--dump-outputs", str(dump)],
                       cwd=ROOT, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    rec = json.loads(lines[0])
    assert rec["steps"] == 3 and rec["warmup"] == 1 and rec["n_gpus"] == 1
    assert rec["unit"] == "crops/s" and rec["higher_is_better"] is True and rec["dtype"].startswith("f32")
    assert rec["ms_per_step"] > 0
    # value is crops over the timed steps: batch / (ms_per_step rounded to a microsecond)
    assert rec["value"] == pytest.approx(n / (rec["ms_per_step"] * 1e-3), rel=1e-2)
    for leg in ("roofline", "fft_kernels", "cpu_baseline", "parity", "extras", "breakdown_ms_per_step"):
        assert leg not in rec, leg
    assert sorted(os.listdir(dump)) == ["pose.npy"]
    got = np.load(dump / "pose.npy")
    assert got.shape == (n, 69) and got.dtype == np.float32 and np.isfinite(got).all()
    # the same seeded weights / crops / O0 through a context of the same dtype in this process
    W = mp.weights
    dev = torch.device("cuda", 0)
    ctx = mp._lib.Context(mp._lib.MP_MODEL_HGRU_POSE, dev.index)
    for v in W.hgru_pose_vars(output_shape=69, timesteps=T, crop=crop):
        ctx.set_weight(v.name, W.synth_value(v, 1234, T))
    ctx.finalize(mp._lib.dtype_code("f32_fft"))
    depth = torch.from_numpy(W.synth_crops(n, seed=42, size=crop)).to(dev)
    o0 = torch.from_numpy(W.synth_hidden((n, crop // 2, crop // 2, 64), seed=7)).to(dev)
    out = torch.empty((n, 69), dtype=torch.float32, device=dev)
    ctx.pose_fwd(depth, o0, out, mp._lib.current_stream(dev))
    torch.cuda.synchronize()
    want = out.cpu().numpy()
    ctx.close()
    assert np.array_equal(got, want)
