"""The pose model's own kernels, one layer at a time, against float64 of that layer computed from the
GPU's own input to it (tests/pose_layer_cases.py: tables, references, split models, gates):
conv_1 + pool (pool1), conv_2 and conv_3 with the backbone epilogue in every tile form, fc_1 on the
pre-split planes and with the in-loop split at every row tile, its reduce with the folded BN, and fc_out.

Two gates per layer.  G1, per element: |got - ref| <= bound(kind, K, S, A).  G2, per region (whole
tensor, image border, tile seams, last image of the batch and of each hGRU slice; for fc layers the rows
at every tile edge): rms(got - ref) <= 1/16 of what the emulated f16 split gives when it loses either lo
product (bf16: twice the one-product model's error).  Every output and tap buffer is one image / row too
long and must keep its sentinel; `out` must be the same bits with no taps, the backbone taps and the head
taps.  Every test prints its worst err/bound (G1) and err/gate (G2); the measured figures are in
profiles/pose_layers/README.md.
"""
import json
import os
import subprocess
import sys

import pytest

import pose_layer_cases as P

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _report(res):
    for layer, d in res["layers"].items():
        print(f"{res['row']} [{res['dtype']}] n={res['n']} {layer}: err/bound {d['g1']:.4f}  err/gate {d['g2']:.4f}"
              f" ({d['g2_region']})")
    assert res["g1"] <= 1.0, res
    assert res["g2"] <= 1.0, res
    assert all(res["same"].values()), res["same"]


_BB = P.params(P.BACKBONE_ROWS)
_HEAD = P.params(P.HEAD_ROWS)


@pytest.mark.parametrize("name,dtype,n", _BB, ids=[f"{a}-{d}-n{n}" for a, d, n in _BB])
def test_backbone_row(name, dtype, n):
    _report(P.run_backbone_row(name, dtype, n))


@pytest.mark.parametrize("name,dtype,n", _HEAD, ids=[f"{a}-{d}-n{n}" for a, d, n in _HEAD])
def test_head_row(name, dtype, n):
    res = P.run_head_row(name, dtype, n)
    assert res["positive"] >= 0.25
    _report(res)


@pytest.mark.parametrize("setting", sorted(P.SWITCH_ROWS))
def test_rows_under_a_dispatch_switch(setting):
    """The switches are cached in statics, so each setting runs in one child process: two backbone and two
    head rows of the tables under the same two gates."""
    rows = P.SWITCH_ROWS[setting]
    var, val = setting.split("=")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "pose_layer_cases.py"),
                        ",".join(f"{a}:{d}:{n}" for a, d, n in rows)],
                       env={**os.environ, var: val}, capture_output=True, text=True, timeout=170)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    res = [json.loads(l) for l in r.stdout.strip().splitlines() if l.startswith("{")]
    assert [(d["row"], d["dtype"], d["n"]) for d in res] == [tuple(x) for x in rows]
    for d in res:
        print(setting, end=" ")
        _report(d)
