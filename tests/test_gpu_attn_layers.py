"""The attention net's kernels, one layer at a time, against float64 of that layer computed from the GPU's
own input to it (tests/attn_layer_cases.py: tables, inputs, references, gates): the fused aconv_1 + pool +
BN kernel, aconv_2 .. aconv_4 on the unpooled TALL halo kernel with 2, 4 and 8 rows per tile, aconv_5 on the
wide im2col kernel at K = 12,800, pool2_kernel's BN epilogue on gammas of both signs, afc_1 with its folded BN
and afc_out, at batches 1 / 3 / 11 / 130 in fp32_split, fp32 and bf16, and the 424 x 512 resize.

Every row asserts the kernel each conv took (mp_info attn_path:<scope>), G1 per element and G2 per region
(the lost-plane gate on conv3, conv4, conv5 and relu1), that every buffer keeps the sentinel past its last
image, and that the tapped call's output is the plain call's bit for bit.  Every test prints its worst
err / bound and err / gate; the measured figures are in profiles/attn_layers/README.md.

Measured maxima on an MI355X (err / bound; err / gate where G2 applies), over batches 1, 3, 11, 130:
  tap     fp32_split         fp32      bf16
  pool1   0.3353             0.3353    0.3353
  conv2   0.0023             0.0095    0.1252
  pool2   0.8453             0.8657    0.8626
  conv3   0.0011 / 0.0306    0.0051    0.0886 / 0.5000
  pool3   0.8198             0.7933    0.8403
  conv4   0.0006 / 0.0477    0.0033    0.0582 / 0.5000
  pool4   0.8766             0.9255    0.9147
  conv5   0.0001 / 0.0928    0.0005    0.0207 / 0.5000
  pool5   0.9337             0.8774    0.8896
  relu1   0.0000 / 0.0220    0.0000    0.0072 / 0.5000
  out     0.0003             0.0005    0.6342
The 424 x 512 row, the three switch rows and B = 256 (rel_inf 2.1e-6 against float64) are in the README.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import attn_layer_cases as A
from helpers import FP32_REL_TOL, rel_inf
from oracle import regressors_ref as RR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _report(res, setting=""):
    tag = f"[{res['dtype']}] n={res['n']}" + (" 424x512" if res["big"] else "") + (f" {setting}" if setting else "")
    for layer, d in res["layers"].items():
        print(f"attn {tag} {layer}: err/bound {d['g1']:.4f}  err/gate {d['g2']:.4f} ({d['g2_region']})"
              f"  positive {d['positive']:.3f}")
    for scope, p in res["paths"].items():
        print(f"attn {tag} {scope}: {p}")
    bad = A.path_mismatches(res["paths"], res["dtype"], setting)
    assert not bad, bad
    assert res["g1"] <= 1.0, res
    assert res["g2"] <= 1.0, res
    assert all(res["same"].values()), res["same"]


_ROWS = A.params()


@pytest.mark.parametrize("dtype,n", _ROWS, ids=[f"{d}-n{n}" for d, n in _ROWS])
def test_layer_row(dtype, n):
    _report(A.run_row(dtype, n))


def test_layer_row_424x512_resized():
    """the resize on the way in: the resized tap equals TF1's bilinear kernel bit for bit, and every layer
    behind it holds its gate"""
    res = A.run_row(*A.BIG_ROW, big=True)
    assert "resized" in res["same"]
    _report(res)


@pytest.mark.parametrize("dtype", A.DTYPES)
def test_one_frame_after_a_batch_of_130(dtype):
    """the workspace of a batch of 130 reused by a single frame: the same bits as the frame's row in the batch"""
    ctx = A.context(dtype)
    big = A.forward(ctx, A.attn_frames(130))["out"]
    one = A.forward(ctx, A.attn_frames(1))["out"]
    print(f"attn [{dtype}] frame 0 alone after n=130: max |difference| from its row "
          f"{float(np.abs(one[0].astype(np.float64) - big[0]).max()):.3e}")
    assert np.array_equal(one[0], big[0])
    p1 = A.paths_of(ctx)
    assert not A.path_mismatches(p1, dtype), p1           # a property of the layer, never of the batch


@pytest.mark.parametrize("setting", A.SWITCHES)
def test_row_under_a_dispatch_switch(setting):
    """The switches are cached in statics, so each setting runs in one child process: the n = 3 fp32_split
    row under the same gates and the setting's own expected kernels."""
    dtype, n = A.SWITCH_ROW
    var, val = setting.split("=")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "attn_layer_cases.py"), f"{dtype}:{n}"],
                       env={**os.environ, var: val}, capture_output=True, text=True, timeout=170)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    res = [json.loads(l) for l in r.stdout.strip().splitlines() if l.startswith("{")]
    assert [(d["dtype"], d["n"]) for d in res] == [(dtype, n)]
    _report(res[0], setting)


def test_benchmarked_batch_of_256():
    """B = 256 frames of 424 x 512, the batch bench.py times (attn_b256): eight distinct frames repeated, so
    every frame differs from its neighbours.  Frames 3, 130 and 255 against the float64 oracle, a second run
    bit-identical, and each sampled frame alone bit-identical to its row."""
    import torch
    B, sample = 256, (3, 130, 255)
    distinct = A.pkg().weights.synth_frames(8, seed=A.BIG_FRAME_SEED + 1) * A.FRAME_GAIN
    src = np.arange(B) % 8
    ref = RR.attn_forward(distinct[src[list(sample)]], A.attn_weights())
    ctx = A.context("fp32_split")
    L = A.pkg()._lib
    frames = torch.from_numpy(distinct).cuda()[torch.from_numpy(src).cuda()].contiguous()
    outs = []
    for _ in range(2):
        out = torch.full((B, A.NOUT), float("nan"), device="cuda")
        ctx.attn_fwd(frames, out, L.current_stream())
        torch.cuda.synchronize()
        outs.append(out.cpu().numpy())
    err = rel_inf(outs[0][list(sample)], ref)
    print(f"attn B=256 424x512 fp32_split: frames {sample} rel_inf vs float64 {err:.3e}")
    # the sampled frames' neighbours are other frames, by far more than the tolerance
    for i in sample:
        for j in (i - 1, i + 1):
            if 0 <= j < B:
                assert rel_inf(outs[0][j], outs[0][i]) > 100 * FP32_REL_TOL, (i, j)
    assert err <= FP32_REL_TOL
    assert np.array_equal(outs[0], outs[1])
    assert np.array_equal(outs[0][8:], outs[0][:-8])            # the same frame gives the same bits in any tile
    for i in sample:
        one = torch.full((1, A.NOUT), float("nan"), device="cuda")
        ctx.attn_fwd(frames[i:i + 1].contiguous(), one, L.current_stream())
        torch.cuda.synchronize()
        assert np.array_equal(one.cpu().numpy()[0], outs[0][i]), i
