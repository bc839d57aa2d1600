"""Every f16-split kernel across the window of magnitudes its scale gives it (tests/magnitude_cases.py: tables,
inputs, bounds; the windows themselves are in include/monkeypose.h).

Part 1, weight rescaling: a layer's weights and bias times 2^j, j in {-20, -7, 7, 20}, must give
ldexp(baseline, j) bit for bit on every dtype the row supports -- the per-tensor weight scale absorbs the
factor, `unscale` carries it, and the fp32 and bf16 roundings are homogeneous.  For the pose model's convs the
folded BN behind the relu takes the factor out again and the tap keeps the baseline's bits; for the hGRU loops
beta, nu and gamma do, and every stored O_t and I_t keeps them.

Part 2, activation sweeps: input and bias times 2^j below 1 (j = -6, -12, -24) and at the top of the path's
window, each op per element against float64 of the GPU's own input to it under the row's bound (3K + 16) u S +
A / s; at j = -24 that floor is the whole bound.  The `fp32` dtype with zero bias must scale bit for bit.

Every test prints its err / bound per sweep point; the measured figures are in profiles/magnitude/README.md.
"""
import json
import os
import subprocess
import sys

import pytest

import magnitude_cases as M
import pose_layer_cases as P

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNITS = M.graph_units()
EDGES = M.edge_units()


# -------------------------------------------------------------------------------- graph runtime
_RESCALE = [(u.name, d) for u in UNITS.values() for d in u.dtypes]
_SWEEP = [(u.name, d) for u in UNITS.values() for d in M.GRAPH_SWEEP_DTYPES if d in u.dtypes]


@pytest.mark.parametrize("name,dtype", _RESCALE, ids=[f"{n}-{d}" for n, d in _RESCALE])
def test_graph_weight_rescaling_is_bit_exact(name, dtype):
    bad = M.graph_rescale_mismatches(UNITS[name], dtype)
    assert not bad, bad


@pytest.mark.parametrize("name,dtype", _SWEEP, ids=[f"{n}-{d}" for n, d in _SWEEP])
def test_graph_activation_sweep(name, dtype):
    u = UNITS[name]
    worst = {}
    for j in M.graph_sweep_points(u, dtype):
        worst[j] = M.graph_sweep_ratio(u, dtype, j)
        print(f"err/bound {name} [{dtype}] j={j}: {worst[j]:.4f}")
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize("name", sorted(UNITS))
def test_graph_fp32_dtype_scales_bit_for_bit(name):
    """no f16 staging hides in the exact path: with zero bias the output at input 2^j is ldexp(baseline, j)"""
    bad = M.graph_fp32_mismatches(UNITS[name])
    assert not bad, bad


@pytest.mark.parametrize("dtype", M.GRAPH_SWEEP_DTYPES)
@pytest.mark.parametrize("name", sorted(EDGES))
def test_graph_edge_tensors(name, dtype):
    """max |w| exactly 2^-3, the maximum held by a negative element (the row's ordinary bound), and one weight
    2^20 above the rest (the bound with magnitude_cases' OUTLIER_TERM)"""
    u = EDGES[name]
    r = M.graph_sweep_ratio(u, dtype, 0, outlier=u.edge == "outlier")      # the term applies under fp32_split only
    print(f"err/bound {name} [{dtype}]: {r:.4f}")
    assert r <= 1.0, r


# ----------------------------------------------------------------------------------- pose model
_POSE = [(l, d) for l in M.POSE_LAYERS
         for d in P.ROWS[M.POSE_HEAD_ROW if l == "fc_1" else M.POSE_BB_ROW].dtypes]


@pytest.mark.parametrize("layer,dtype", _POSE, ids=[f"{l}-{d}" for l, d in _POSE])
def test_pose_weight_rescaling_is_bit_exact(layer, dtype):
    bad = M.pose_rescale_mismatches(layer, dtype)
    assert not bad, bad


@pytest.mark.parametrize("dtype", M.POSE_SWEEP_DTYPES)
@pytest.mark.parametrize("path", ["backbone", "fc_1"])
def test_pose_activation_sweep(path, dtype):
    """conv_2 (split at BB_ASCALE) and fc_1 (split unscaled) under G1 with the floor A / s at every sweep point,
    and under G2 -- the result at least 16 times nearer than either dropped-plane model -- at the top and at -6"""
    res = {}
    for j in M.pose_sweep_points(path, dtype):
        res[j] = M.pose_sweep(path, dtype, j)
        print(f"{path} [{dtype}] j={j}: err/bound {res[j]['g1']:.4f}  err/gate {res[j]['g2']:.4f}  "
              f"max|input| {res[j]['xmax']:.4g}")
    assert max(r["g1"] for r in res.values()) <= 1.0, res
    assert max(r["g2"] for r in res.values()) <= 1.0, res
    if dtype != "bf16":   # the top point is the last octave of the window on the GPU's own input
        top = M.pose_top(path)
        scale = P.BB_ASCALE if path == "backbone" else 1.0
        assert res[top]["xmax"] * scale <= 2.0 ** M.TOP_LOG2 < 2 * res[top]["xmax"] * scale, res[top]


# ----------------------------------------------------------------------------------- hGRU loops
@pytest.mark.parametrize("name", [c.name for c in M.LOOPS])
def test_loop_weight_rescaling_is_bit_exact(name):
    bad = M.loop_rescale_mismatches(name)
    assert not bad, bad


def test_six_launch_loop_weight_rescaling_is_bit_exact():
    """MP_FFT4=0 (read once at library load: one child process for both dtypes)"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "magnitude_cases.py"), ",".join(M.SIX_LAUNCH)],
                       env={**os.environ, "MP_FFT4": "0"}, capture_output=True, text=True, timeout=110)
    assert r.returncode == 0, r.stderr[-2000:]
    res = [json.loads(l) for l in r.stdout.strip().splitlines() if l.startswith("{")]
    assert [d["row"] for d in res] == list(M.SIX_LAUNCH)
    for d in res:
        assert d["fft_loop"] == 6 and not d["bad"], d


# ---------------------------------------------------------------- hGRU loops: the first half-step
def _check_i1(what, got, ref, e32, ssf, dtype):
    import circuit_shape_cases as S
    assert got.shape == ref.shape
    return S.check(what, got, ref, ssf, dtype, e32)


@pytest.mark.parametrize("name", [t.name for t in M.TWINS])
def test_loop_first_half_step_across_its_window(name):
    """the rescaled twin (O0 2^j; i_r, p_r, beta 2^-j) at the points its split model reaches below 1 and at the top
    of the path's window, I_1 against the float64 oracle of the twin under the fp32-class rule; and once with
    hidden_init='identity', X scaled to the top.  Nothing can take the factor out of the drive X, so on the two tanh
    paths that run is saturated and checks range and finiteness only; on the relu path it is as sensitive as the twin
    (test_magnitude_cases_cpu.py pins both)."""
    c = M.TWIN_LOOPS[M.TWINS_BY_NAME[name].loop]
    for j in M.twin_points(name):
        ref, e32 = M.twin_reference(name, j)
        _check_i1(f"{name} j={j} I_1", M.twin_run(name, j), ref, e32, c.shape[3], c.dtype)
    j = M.twin_top(name, identity=True)
    ref, e32 = M.twin_reference(name, j, True)
    _check_i1(f"{name} identity j={j} I_1", M.twin_run(name, j, True), ref, e32, c.shape[3], c.dtype)


@pytest.mark.parametrize("conv", sorted(M.CNF_CASES))
def test_channel_general_fft_conv_at_its_ceiling(conv):
    """a constant-sign conv input with min(h, 64) min(w, 64) max|v| / 64 = 2^15.9 (the header's range sentence):
    finite, and I_1 within the bounds of circuit_fft_cases (the project gate and max(10 e32, 1e-5))"""
    ref, e32 = M.cnf_reference(conv)
    _check_i1(f"cnf {conv} I_1", M.cnf_run(conv), ref, e32, M.CNF_SSF, "fp32_split")


@pytest.mark.parametrize("edge", M.EDGE_TENSORS)
def test_circuit_edge_tensors(edge):
    """p_r with max |w| = 2^-3, with a negative maximum and with one tap 2^20 above the rest, on the fused
    fp32_fft loop: O_T under the fp32-class rule.  (What the path packs is p_r's spectrum, and the spectrum of one
    large tap has the same magnitude at every frequency: no packed value is pushed towards the subnormals.)"""
    ref, e32 = M.circuit_edge_reference(edge)
    _check_i1(f"fp32_fft p_r {edge} O_T", M.circuit_edge_run(edge), ref, e32, 5, "fp32_fft")
