"""CPU: the conditions the GPU time-axis tests (tests/test_gpu_circuit_time.py) rest on, from the case
table (tests/circuit_time_cases.py) and the float64 oracle alone: every loop and dtype is there at
timesteps = 1, and the four-step loop (fp32_fft and bf16), the general loop and the channel-general loop
(direct and 'fft' conv) are there below len(rho) as well; the oracle itself does not
depend on len(rho) (prefix property); and on every case a run of one step more or fewer, a run that
returned O0, or a rho taken from the wrong end of the vector differs from the expected result by at
least SENSITIVITY_MARGIN times the bound the GPU test applies, so that no such kernel can pass."""
import numpy as np
import pytest

import circuit_shape_cases as S
import circuit_time_cases as T
from helpers import rel_inf

CASES = T.ALL_CASES
ORACLE_KEYS = sorted({(T._key(c), c.t_run) for c in CASES}, key=str)
ONE_PER_KEY = [next(c for c in CASES if (T._key(c), c.t_run) == k) for k in ORACLE_KEYS]


def test_every_loop_and_dtype_runs_one_step():
    t1 = {(c.loop, c.dtype) for c in T.T1 if c.t_run == 1}
    assert t1 >= {(T.FUSED, "fp32_fft"), (T.FUSED, "bf16"), (T.DIRECT, "fp32"), (T.DIRECT, "fp32_split"),
                  (T.SIX, "fp32_fft"), (T.SIX, "bf16"), (T.GENERAL, "fp32_fft"), (T.GENERAL, "fp32"),
                  (T.NHWC, "fp32_split"), (T.POSE, "fp32_fft"), (T.POSE, "bf16"), (T.POSE, "fp32")}
    assert all(c.t_run == 1 for c in T.T1)
    assert {c.n for c in T.T1_FUSED if c.dtype == "fp32_fft" and (c.h, c.ssf) == (9, 5)} >= {2, 9, 66, 130}
    assert {(c.h, c.w, c.ssf) for c in T.T1_FUSED if c.dtype == "fp32_fft"} >= {(9, 32, 5), (7, 32, 15), (17, 64, 3)}
    assert {c.n for c in T.T1_FUSED if c.dtype == "bf16"} == {2, 9, 66}
    assert {(c.dtype, c.n) for c in T.T1_DIRECT} == {("fp32", 1), ("fp32", 2), ("fp32_split", 1), ("fp32_split", 2)}
    assert {(c.dtype, c.n) for c in T.T1_SIX} == {(d, n) for d in ("fp32_fft", "bf16") for n in (2, 66)}
    assert {(c.dtype, c.variant) for c in T.T1_GENERAL} == {(d, v) for d in ("fp32_fft", "fp32")
                                                           for v in ("pose", "defaults", T.NO_ADAPT)}
    assert {(c.k, c.conv) for c in T.T1_NHWC} >= {(8, "direct"), (25, "direct"), (64, "direct"), (8, "fft"), (4, "fft_tiled")}
    assert {c.variant for c in T.T1_NHWC} == {"pose", "defaults"}
    assert {(c.dtype, c.n) for c in T.T1_POSE} == {(d, n) for d in ("fp32_fft", "bf16", "fp32") for n in T.POSE_NS}
    assert len({T.case_id(c) for c in CASES}) == len(CASES) and all(T.BY_ID[T.case_id(c)] == c for c in CASES + T.REUSE)


def test_short_and_long_cases_are_the_ones_named():
    short = {(c.loop, c.dtype, c.variant, c.conv, c.n) for c in T.SHORT}
    assert short >= {(T.FUSED, "fp32_fft", "pose", None, 2), (T.FUSED, "fp32_fft", "pose", None, 9),
                     (T.GENERAL, "fp32_fft", "pose", None, 2), (T.GENERAL, "fp32_fft", "defaults", None, 2),
                     (T.NHWC, "fp32_split", "pose", "direct", 2), (T.NHWC, "fp32_split", "pose", "fft", 2)}
    assert any(c.loop == T.FUSED and c.dtype == "bf16" for c in T.SHORT)
    for c in T.SHORT:
        assert c.len_rho == T.LEN_RHO == 3 and 1 <= c.t_run < c.len_rho
        assert c._replace(t_run=3 - c.t_run) in T.SHORT            # both 1 and 2
        if T.adapts(c):
            rho = T.rho_of(c)
            assert rho.shape == (3,) and len(set(rho.tolist())) == 3       # non-constant
    assert {c.loop for c in T.LONG} == {T.GENERAL, T.NHWC}
    for c in T.LONG:
        assert not T.adapts(c) and T.rho_of(c) is None and c.t_run == 4 > c.len_rho
    assert not T.CC.aux_of(T.NO_ADAPT)['adapation'] and not T.CC.aux_of("defaults")['adapation']
    assert T.CC.aux_of("adapt")['adapation'] and T.CC.aux_of("pose")['adapation']
    assert all(T.adapts(c) and c.len_rho == 3 for c in T.REJECT)
    assert {(T.uses_var_entry(c), c.loop) for c in T.REJECT} == {(False, T.FUSED), (False, T.DIRECT), (False, T.NHWC),
                                                                 (True, T.GENERAL), (True, T.NHWC)}
    assert T.REUSE_STEPS == (3, 1, 2, 1, 3) and all(c.len_rho == 3 and T.adapts(c) for c in T.REUSE)
    assert {(c.loop, c.dtype) for c in T.REUSE} == {(T.FUSED, "fp32_fft"), (T.FUSED, "bf16"), (T.GENERAL, "fp32_fft"),
                                                   (T.NHWC, "fp32_split")}


def test_every_case_fits_its_path():
    from pose_layer_cases import shape_ok
    L = T.pkg()._lib
    for c in CASES + T.REUSE + T.REJECT:
        assert c.ssf in (3, 5, 15) and c.n >= 1 and c.t_run >= 1
        if c.loop == T.NHWC:
            assert c.k != 64 or T.nhwc_loop_flag(c)
            if c.conv != "direct":
                assert L.resolve_nhwc_conv(c.conv, c.dtype, c.h, c.w, c.k, T.nhwc_loop_flag(c)) == L.NHWC_CONVS[c.conv]
            assert (c.h > 64) == (c.conv == "fft_tiled")
        elif c.loop == T.POSE:
            assert shape_ok(c.h, c.w, c.dtype) and not shape_ok(c.h // 2, c.w, c.dtype)     # the smallest
        else:
            assert c.k == 64 and S.map_ok(c.dtype, c.h, c.w), c
        if c.loop in (T.FUSED, T.SIX):
            assert c.dtype in ("fp32_fft", "bf16")
    # the batch dispatch the fused cases name (mp_abi.hip run_circuit): 66 = 64 + 2 on two streams
    assert S.first_slice(66) == 64 and S.first_slice(130) == 96 and S.first_slice(12) == 12
    assert S.sampled_images(66) == [0, 63, 64, 65]


@pytest.mark.parametrize("c", ONE_PER_KEY, ids=T.case_id)
def test_one_step_stacks_and_finite_regions(c):
    """the stored-state stacks hold t_run maps of the case's shape (one at T = 1), the stacked last O is the
    returned O, and every error region carries values of the map's scale"""
    o = T.oracle(c)
    shape = (c.n, c.h, c.w, c.k)
    assert len(o["O_t"]) == len(o["I_t"]) == c.t_run
    assert np.stack(o["O_t"], 1).shape == np.stack(o["I_t"], 1).shape == (c.n, c.t_run) + shape[1:]
    assert np.array_equal(o["O_t"][-1], o["O"]) and np.array_equal(o["I_t"][-1], o["I"])
    reg = S.regions(c.h, c.w, c.ssf)
    for a in (o["O"], o["I"]):
        assert a.dtype == np.float64 and a.shape == shape and np.isfinite(a).all()
        top = np.abs(a).max()
        assert top > 1e-2
        for k in S.METRICS:
            assert reg[k].any() and np.abs(a[:, reg[k]]).max() >= 0.5 * top, (T.case_id(c), k)
    if c.loop == T.POSE:
        assert o["out"].shape == (c.n, 69) and np.abs(o["out"]).max() > 1e-2


@pytest.mark.parametrize("c", ONE_PER_KEY, ids=T.case_id)
def test_float32_oracle_error_leaves_the_floor_operative(c):
    e = T.e32(c)
    rows = [e["O"], e["I"], *e["O_t"], *e["I_t"]]
    print(f"e32 {T.case_id(c)}: O_T " + " ".join(f"{v:.2e}" for v in e["O"]) + f"  max {max(max(r) for r in rows):.2e}")
    for r in rows:
        for v in r:
            assert 0 < v <= 1e-6 and T.bound(c._replace(dtype="fp32"), v) == S.FP32_CLASS_FLOOR


@pytest.mark.parametrize("c", [c for c in ONE_PER_KEY if not T.adapts(c) or c.t_run < c.len_rho], ids=T.case_id)
def test_prefix_property(c):
    """the oracle's states after t_run steps are the first t_run states of its longer run on the same
    weights, exactly: the oracle reads rho[t] and nothing that depends on len(rho)"""
    longer = max(c.len_rho, c.t_run + 1)        # without adaptation there is no rho to run out of
    a, b = T.oracle(c), T.oracle(c, longer)
    for t in range(c.t_run):
        assert np.array_equal(a["O_t"][t], b["O_t"][t]) and np.array_equal(a["I_t"][t], b["I_t"][t]), t
    assert np.array_equal(a["O"], b["O_t"][c.t_run - 1])


def _margin(c):
    return T.BF16_MARGIN if c.dtype == "bf16" else T.SENSITIVITY_MARGIN


@pytest.mark.parametrize("c", CASES, ids=T.case_id)
def test_step_count_sensitivity(c):
    """O after t_run steps differs from O0, from O after t_run - 1 steps and (where rho allows) from O after
    t_run + 1 steps by >= margin * bound on the whole-map metric, and rho[t_run - 1] from rho[len - 1]"""
    o = T.oracle(c)
    need = _margin(c) * T.bound(c, T.e32(c)["O"][0])
    if c.dtype == "bf16":       # its fp32_fft twin carries the 100-bound condition on the same inputs
        twin = c._replace(dtype="fp32_fft")
        assert twin in CASES and T._key(twin) == T._key(c)
    others = {"O0": T.initial_state(c)}
    if c.t_run > 1:
        others["t_run - 1"] = T.oracle(c, c.t_run - 1)["O"]
    if not T.adapts(c) or c.t_run < c.len_rho:
        others["t_run + 1"] = T.oracle(c, c.t_run + 1)["O"]
    for what, a in others.items():
        d = S.metrics(a, o["O"], c.ssf)[0]
        print(f"{T.case_id(c)}: O_T against {what}: {d:.3e} (needs {need:.1e})")
        assert d >= need, (what, d, need)
    if T.adapts(c) and c.t_run < c.len_rho:
        rho = T.rho_of(c).astype(np.float64)
        d = abs(rho[c.t_run - 1] - rho[c.len_rho - 1]) / np.abs(rho).max()
        print(f"{T.case_id(c)}: |rho[{c.t_run - 1}] - rho[{c.len_rho - 1}]| / |rho|_inf = {d:.3e} (needs {need:.1e})")
        assert d >= need, (d, need)
        # and the gain reaches the output: the run with rho read from the wrong end
        wrong = o["O"] * (rho[c.len_rho - 1] / rho[c.t_run - 1]) if c.t_run == 1 else None
        if wrong is not None:
            assert S.metrics(wrong, o["O"], c.ssf)[0] >= need


@pytest.mark.parametrize("hidden_init", ["zeros", "identity"])
def test_hidden_init_oracles_at_one_step(hidden_init):
    """the initial state reaches O_1 on every loop the GPU test runs hidden_init on"""
    assert len(T.HIDDEN_CASES) == 5
    for c in T.HIDDEN_CASES + [c for c in T.T1_POSE if c.n == 2]:
        o = T.oracle(c, None, "float64", hidden_init)
        assert np.isfinite(o["O"]).all() and rel_inf(o["O"], T.oracle(c)["O"]) >= 1e-2, T.case_id(c)
        e = T.e32(c, None, hidden_init)
        assert max(max(r) for r in [e["O"], e["I"]]) <= 1e-6


def test_second_input_set_differs():
    for c in T.REUSE:
        a, b = T.inputs(c), T.inputs(c, second=True)
        assert a[0] is b[0] or all(np.array_equal(a[0][k], b[0][k]) for k in a[0])        # one weight set
        assert b[1].shape == (T.REUSE_SECOND_N, c.h, c.w, c.k) and b[1].shape[0] != a[1].shape[0]
        assert rel_inf(b[1][:2], a[1][:2]) >= 0.5 and rel_inf(b[2][:2], a[2][:2]) >= 0.5
        o = T.oracle(c, T.REUSE_SECOND, second=True)["O"]
        assert o.shape == b[1].shape and np.isfinite(o).all()
