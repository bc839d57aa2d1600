"""The per-launch profile contract of the pose forward (mp_profile_enable / mp_profile_read), which
bench.py and tools/ read: with profiling on, one forward records every launch of the hGRU loop under
its scope name, once, on one stream.  The counts follow from the loop structure:

  four-step loop (fp32_fft)    row_init 1; per step col_gemm, row_a, col_gemm, row_b (the last: row_final)
  six-launch loop (MP_FFT4=0)  per step fft_fwd, spec_gemm, inv_a_fwd, spec_gemm, fft_inv, epi_b
  direct convs (fp32_split)    per step conv15_a, conv15_b

and the outer scopes conv15_a / conv15_b wrap the two half-steps of every loop (row_init counts as an
A half-step).  Golden case pose_c64_t8: crop 64, a 32 x 32 map, T = 8, batch 2."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import MG, golden_meta, pkg

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 8
FOUR_STEP = ("row_init", "col_gemm", "row_a", "row_b", "row_final")
SIX_LAUNCH = ("fft_fwd", "spec_gemm", "inv_a_fwd", "fft_inv", "epi_b")
NAMES = FOUR_STEP + SIX_LAUNCH + ("conv15_a", "conv15_b", "backbone", "fc1", "fc_out")


def profile_counts(dtype):
    """launches per scope name of one profiled forward of pose_c64_t8"""
    m = golden_meta()["pose_c64_t8"]
    assert (m["n"], m["crop"], m["timesteps"]) == (2, 64, T)
    wts, depth, O0 = MG.pose_inputs(m["n"], m["crop"], T, m["weight_seed"], m["crop_seed"], m["o0_seed"])
    model = pkg().hgru_pose.model()
    model.compute_dtype = dtype
    model.load_weights(wts)
    x, o0 = torch.from_numpy(depth).cuda(), torch.from_numpy(O0).cuda()
    model.build(x, m["output_shape"], train_mode=False, h2_init=o0)   # the context; unprofiled
    model.profile(True)
    out = model.forward(x, h2_init=o0)
    model.profile(False)
    assert np.isfinite(out.cpu().numpy()).all()
    counts = {}
    for name in NAMES:
        ms, n = model.profile_read(name)
        assert n == 0 or ms > 0, name
        counts[name] = n
    return counts


def test_four_step_loop_scopes():
    c = profile_counts("fp32_fft")
    print(c)
    want = {"row_init": 1, "col_gemm": 2 * T, "row_a": T, "row_b": T - 1, "row_final": 1, "backbone": 1, "fc1": 1,
            "fc_out": 1, "conv15_a": T + 1, "conv15_b": T, **{k: 0 for k in SIX_LAUNCH}}
    assert c == want


def test_six_launch_loop_scopes():
    """MP_FFT4 is read once per process: a fresh child"""
    code = (f"import json, sys\nsys.path.insert(0, {os.path.join(ROOT, 'tests')!r})\n"
            "import test_gpu_profile_scopes as t\nprint(json.dumps(t.profile_counts('fp32_fft')))\n")
    r = subprocess.run([sys.executable, "-c", code], env={**os.environ, "MP_FFT4": "0"}, capture_output=True,
                       text=True, timeout=110)
    assert r.returncode == 0, r.stderr[-2000:]
    c = json.loads(r.stdout.strip().splitlines()[-1])
    print(c)
    want = {"fft_fwd": T, "spec_gemm": 2 * T, "inv_a_fwd": T, "fft_inv": T, "epi_b": T, "backbone": 1, "fc1": 1,
            "fc_out": 1, "conv15_a": T, "conv15_b": T, **{k: 0 for k in FOUR_STEP}}
    assert c == want


def test_direct_loop_scopes():
    c = profile_counts("fp32_split")
    print(c)
    want = {"conv15_a": T, "conv15_b": T, "backbone": 1, "fc1": 1, "fc_out": 1,
            **{k: 0 for k in FOUR_STEP + SIX_LAUNCH}}
    assert c == want
