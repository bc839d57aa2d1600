"""GPU: the time axis of every hGRU loop (tests/circuit_time_cases.py) -- timesteps = 1, the module's
default, where the first step is also the last; fewer steps than rho holds; more, without adaptation --
against the float64 oracle run at the same step count, on the three error metrics of circuit_shape_cases
at the project gate and, for the fp32-class paths, at max(10 * e32, 1e-5).  At T = 1 the four-step loop's
step 0 reads O0 as NHWC, gets no C8 map to write unless states are stored, and is ROW_FINAL (mode 2,
fc_1's planes, on the pose model); each other loop's `t == T - 1` branch meets its `t == 0` one.  One
context runs several step counts in turn (a stale state map would show), and the switches that change
those paths are run in child processes, four in all, beside the in-process tests (the `children` fixture)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import circuit_fft_tiled_cases as FT
import circuit_shape_cases as S
import circuit_time_cases as T
from helpers import pkg, rel_inf

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IN_PROCESS = [c for c in T.T1 if c.loop not in (T.SIX, T.POSE)]
STATE_CASES = [c for c in IN_PROCESS if c.n <= 12]                              # every loop
SHORT_PAIRS = [c for c in T.SHORT if c.t_run == 1]                              # with its t_run = 2 twin


def _check(what, c, got, ref, e, key, t=None):
    """circuit_shape_cases.check on one state map; the tiled FFT conv's own check adds its seam band"""
    e32 = e[key] if t is None else e[key][t]
    if c.conv == "fft_tiled":
        r32 = T.oracle(c, None, "float32")
        ref32 = r32[key] if t is None else r32[key][t]
        return FT.check(what, got, ref, c.ssf, e32, ref32)
    return S.check(what, got, ref, c.ssf, c.dtype, None if c.dtype == "bf16" else e32)


@pytest.mark.parametrize("c", IN_PROCESS, ids=T.case_id)
def test_parity_at_one_step(c):
    """O_1 (and I_1 where the entry point returns it) against float64; from 64 images on also the images at
    the batch-slice edges, each on its own"""
    ref, e = T.oracle(c), T.e32(c)
    r = T.run(c)
    assert r["O"].shape == (c.n, c.h, c.w, c.k)
    _check(f"{T.case_id(c)} O_1", c, r["O"], ref["O"], e, "O")
    if "I" in r:
        _check(f"{T.case_id(c)} I_1", c, r["I"], ref["I"], e, "I")
    else:
        assert not T.uses_var_entry(c)
    if c.n >= 64:
        r32 = T.oracle(c, None, "float32")["O"]
        for i in S.sampled_images(c.n):
            S.check(f"{T.case_id(c)} image {i}", r["O"][i:i + 1], ref["O"][i:i + 1], c.ssf, c.dtype,
                    None if c.dtype == "bf16" else S.metrics(r32[i:i + 1], ref["O"][i:i + 1], c.ssf))


@pytest.mark.parametrize("c", STATE_CASES, ids=T.case_id)
def test_store_states_at_one_step(c):
    """the stacks are [n, 1, h, w, k], O_1 and I_1 within the bounds, and the plain call's output is
    stack[:, 0] bit for bit (bf16: to the rounding of the bf16 state map the stack is read from, as
    test_gpu_circuit_shapes has it).  On the four-step loop this is the one configuration where ROW_FINAL at
    step 0 writes the C8 O map from an NHWC O0."""
    ref, e = T.oracle(c), T.e32(c)
    r = T.run(c, store_states=True)
    assert r["sO"].shape == r["sI"].shape == (c.n, 1, c.h, c.w, c.k)
    _check(f"{T.case_id(c)} stored O_1", c, r["sO"][:, 0], ref["O_t"][0], e, "O_t", 0)
    _check(f"{T.case_id(c)} stored I_1", c, r["sI"][:, 0], ref["I_t"][0], e, "I_t", 0)
    plain = T.run(c)
    _check(f"{T.case_id(c)} O_1", c, plain["O"], ref["O"], e, "O")
    if c.dtype == "bf16":
        assert np.all(np.abs(r["sO"][:, 0] - plain["O"]) <= 2.0 ** -8 * np.abs(plain["O"]))
    else:
        assert np.array_equal(r["sO"][:, 0], plain["O"])
    if "I" in plain:
        assert np.array_equal(r["sI"][:, 0], plain["I"]) and np.array_equal(r["I"], plain["I"])


@pytest.mark.parametrize("hidden_init", ["zeros", "identity"])
@pytest.mark.parametrize("c", T.HIDDEN_CASES, ids=T.case_id)
def test_hidden_init_at_one_step(c, hidden_init):
    ref, e = T.oracle(c, None, "float64", hidden_init), T.e32(c, None, hidden_init)
    r = T.run(c, hidden_init=hidden_init)
    S.check(f"{T.case_id(c)} {hidden_init} O_1", r["O"], ref["O"], c.ssf, c.dtype, e["O"])
    if "I" in r:
        S.check(f"{T.case_id(c)} {hidden_init} I_1", r["I"], ref["I"], c.ssf, c.dtype, e["I"])


@pytest.mark.parametrize("c", SHORT_PAIRS, ids=T.case_id)
def test_fewer_steps_than_rho_holds(c):
    """1 and 2 steps on weights whose rho holds 3: O, the final I where the entry point returns it and every
    stored O_t and I_t against the oracle at that step count, then len(rho) steps on the same context (through
    the C ABI: one context for all three), and the facade at 1 and 2 steps on the same weights.

    On the general and the channel-general loop the short run's output is also the longer run's stack entry
    bit for bit: every step's O is computed by the one instantiation of circuit_out_kernel<PC4, NL>
    (k_circuit_var.hip:115; the last step only adds the store under the run-time `if (a.out)` at :155) and
    of circuit_nhwc_out_kernel<NL, VW> (k_circuit_nhwc.hip:85, `if (a.out)` at :103), and the stack is a
    copy of the map that kernel writes in place; the I_t entries follow, the input half being launched with the
    same arguments at every step (`a.out = nullptr`, mp_abi.hip var_circuit / nhwc_circuit).  The four-step loop's ROW_B and ROW_FINAL are different
    instantiations: there the oracle alone is the reference."""
    wts, X, O0, I0 = T.inputs(c)
    ctx = T.context(c)
    outs = {}
    for t in (1, 2, c.len_rho):
        ct = c._replace(t_run=t)
        ref = T.oracle(ct)
        e = T.e32(ct)
        r = T.ctx_forward(ctx, c, X, O0, I0, t, states=True)
        assert r["sO"].shape == r["sI"].shape == (c.n, t, c.h, c.w, c.k)
        _check(f"{T.case_id(ct)} O_T", ct, r["O"], ref["O"], e, "O")
        for s in range(t):
            _check(f"{T.case_id(ct)} stored O_{s + 1}", ct, r["sO"][:, s], ref["O_t"][s], e, "O_t", s)
            _check(f"{T.case_id(ct)} stored I_{s + 1}", ct, r["sI"][:, s], ref["I_t"][s], e, "I_t", s)
        plain = T.ctx_forward(ctx, c, X, O0, I0, t)
        if c.dtype != "bf16":
            assert np.array_equal(plain["O"], r["O"]) and np.array_equal(r["sO"][:, -1], r["O"])
        else:
            _check(f"{T.case_id(ct)} O_T (no states)", ct, plain["O"], ref["O"], e, "O")
        if "I" in r:
            _check(f"{T.case_id(ct)} I_T", ct, r["I"], ref["I"], e, "I")
            assert np.array_equal(r["I"], r["sI"][:, -1]) and np.array_equal(plain["I"], r["I"])
        else:
            assert not T.uses_var_entry(c)
        outs[t] = (plain["O"], r["sO"], r["sI"])
    ctx.close()
    if c.loop in (T.GENERAL, T.NHWC):
        for t in (1, 2):
            assert np.array_equal(outs[t][0], outs[c.len_rho][1][:, t - 1]), t
            assert np.array_equal(outs[t][2][:, t - 1], outs[c.len_rho][2][:, t - 1]), t
        assert np.array_equal(outs[1][0], outs[2][1][:, 0])
    for t in (1, 2):        # the facade passes timesteps through with the longer rho
        ct = c._replace(t_run=t)
        f = T.run(ct)
        _check(f"{T.case_id(ct)} facade O_T", ct, f["O"], T.oracle(ct)["O"], T.e32(ct), "O")
        if c.dtype != "bf16":
            assert np.array_equal(f["O"], outs[t][0]), t


@pytest.mark.parametrize("c", T.LONG, ids=T.case_id)
def test_more_steps_than_rho_without_adaptation(c):
    """an aux without adaptation reads no rho: 4 steps on weights that hold none"""
    ref, e = T.oracle(c), T.e32(c)
    r = T.run(c, store_states=True)
    assert r["sO"].shape == (c.n, c.t_run, c.h, c.w, c.k)
    for s in range(c.t_run):
        _check(f"{T.case_id(c)} O_{s + 1}", c, r["sO"][:, s], ref["O_t"][s], e, "O_t", s)
        _check(f"{T.case_id(c)} I_{s + 1}", c, r["sI"][:, s], ref["I_t"][s], e, "I_t", s)
    plain = T.run(c)
    _check(f"{T.case_id(c)} O_T", c, plain["O"], ref["O"], e, "O")
    assert np.array_equal(plain["O"], r["sO"][:, -1])


@pytest.mark.parametrize("c", T.REUSE, ids=T.case_id)
def test_one_context_runs_several_step_counts(c):
    """timesteps 3, 1, 2, 1, 3 on one context and the same inputs, then one step on a second input set: each
    output is a fresh context's bit for bit and within the bounds, and the last 3-step output is the first.
    At T = 1 the four-step loop never writes its C8 O map: a kernel that read the map instead of O0 would
    read the previous call's here."""
    wts, X, O0, I0 = T.inputs(c)
    ctx = T.context(c)
    outs = []
    calls = [(t, (X, O0, I0), False) for t in T.REUSE_STEPS] + [(T.REUSE_SECOND, T.inputs(c, True)[1:], True)]
    for t, (x, o0, i0), second in calls:
        out = T.ctx_forward(ctx, c, x, o0, i0, t)["O"]
        fresh = T.context(c)
        want = T.ctx_forward(fresh, c, x, o0, i0, t)["O"]
        fresh.close()
        assert np.array_equal(out, want), (len(outs), t)
        ct = c._replace(t_run=t)
        ref = T.oracle(ct, second=second)["O"]
        e = None if c.dtype == "bf16" else S.metrics(T.oracle(ct, None, "float32", second=second)["O"], ref, c.ssf)
        S.check(f"{T.case_id(c)} call {len(outs)} T={t}", out, ref, c.ssf, c.dtype, e)
        outs.append(out)
    ctx.close()
    assert np.array_equal(outs[0], outs[4]) and np.array_equal(outs[1], outs[3])
    assert not np.array_equal(outs[0], outs[1]) and not np.array_equal(outs[1], outs[2])


@pytest.mark.parametrize("c", T.T1_POSE, ids=T.case_id)
def test_pose_model_at_one_step(c):
    """the pose model on weights whose rho holds one entry: fc_1's pre-split planes come from a step-0
    ROW_FINAL (rowq_a at n = 2, row8 at 12, two slices at 66).  The output against hgru_pose_forward at one
    step, at the model-output gate; the same bytes with store_states, whose states are within the state
    bounds; at n = 2 and 12 hidden_init 'zeros' and 'identity' (the C8 drive converted to NHWC, read as the
    o_nhwc input)."""
    ctx = T.context(c)
    assert ctx.info("timesteps") == 1
    gate = T.output_gate(c)
    ref, e = T.oracle(c), T.e32(c)
    plain = T.pose_forward(ctx, c)
    err = rel_inf(plain["out"], ref["out"])
    print(f"{T.case_id(c)} out: rel_inf {err:.3e} (gate {gate:.0e})")
    assert np.isfinite(plain["out"]).all() and err <= gate
    st = T.pose_forward(ctx, c, store_states=True)
    assert st["sO"].shape == st["sI"].shape == (c.n, 1, c.h, c.w, 64)
    assert np.array_equal(st["out"], plain["out"])
    _check(f"{T.case_id(c)} stored O_1", c, st["sO"][:, 0], ref["O_t"][0], e, "O_t", 0)
    _check(f"{T.case_id(c)} stored I_1", c, st["sI"][:, 0], ref["I_t"][0], e, "I_t", 0)
    for hi in ("zeros", "identity") if c.n <= 12 else ():
        rh = T.oracle(c, None, "float64", hi)
        got = T.pose_forward(ctx, c, store_states=True, hidden_init=hi)
        err = rel_inf(got["out"], rh["out"])
        print(f"{T.case_id(c)} {hi} out: rel_inf {err:.3e} (gate {gate:.0e})")
        assert err <= gate
        _check(f"{T.case_id(c)} {hi} stored O_1", c, got["sO"][:, 0], rh["O_t"][0], T.e32(c, None, hi), "O_t", 0)
        assert np.array_equal(T.pose_forward(ctx, c, hidden_init=hi)["out"], got["out"])
    again = T.pose_forward(ctx, c)      # after the other initial states: the given one again, the same bytes
    assert np.array_equal(again["out"], plain["out"])
    ctx.close()


@pytest.mark.parametrize("c", T.REJECT, ids=T.case_id)
def test_bad_step_counts_are_rejected_before_any_launch(c):
    """timesteps = 0, and len(rho) + 1 with adaptation, fail with MP_ERR_ARG on mp_hgru_circuit_fwd (the
    fused loop and the channel-general one behind it) and on mp_hgru_circuit_fwd_var (the general loop and
    the channel-general one), and the output keeps its sentinel"""
    L = pkg()._lib
    wts, X, O0, I0 = T.inputs(c)
    ctx = T.context(c)
    assert T.adapts(c)
    for t in (0, -1, c.len_rho + 1):
        out = torch.full(X.shape, 7.0, device="cuda")
        with pytest.raises(L.MonkeyPoseError) as e:
            T.ctx_forward(ctx, c, X, O0, I0, t, out=out)
        assert e.value.code == T.MP_ERR_ARG, str(e.value)
        torch.cuda.synchronize()
        assert bool((out == 7.0).all())
    O = T.ctx_forward(ctx, c, X, O0, I0, c.len_rho)["O"]     # and the context still runs
    ct = c._replace(t_run=c.len_rho)
    _check(f"{T.case_id(ct)} after the rejections", ct, O, T.oracle(ct)["O"], T.e32(ct), "O")
    ctx.close()


@pytest.mark.parametrize("c", T.LONG, ids=T.case_id)
def test_zero_steps_are_rejected_without_adaptation_too(c):
    L = pkg()._lib
    wts, X, O0, I0 = T.inputs(c)
    ctx = T.context(c)
    out = torch.full(X.shape, 7.0, device="cuda")
    with pytest.raises(L.MonkeyPoseError) as e:
        T.ctx_forward(ctx, c, X, O0, I0, 0, out=out)
    assert e.value.code == T.MP_ERR_ARG
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    ctx.close()


SIX_CASES = {d: [c for c in T.T1_SIX if c.dtype == d] for d in ("fp32_fft", "bf16")}
PRESPLIT_CASES = [c for c in T.T1_POSE if c.dtype != "fp32"]
# one child process per setting (the switches are read once at library load): environment, (mode, cases)...
CHILDREN = {
    "MP_O0_DIRECT=0": ({"MP_O0_DIRECT": "0"}, ("both", T.O0_DIRECT)),
    "MP_O0_DIRECT=1": ({"MP_O0_DIRECT": "1"}, ("both", T.O0_DIRECT)),
    "MP_FFT4=0": ({"MP_FFT4": "0"}, ("both", T.T1_SIX)),
    "MP_FC_PRESPLIT=0": ({"MP_FC_PRESPLIT": "0"}, ("plain", PRESPLIT_CASES)),
}


@pytest.fixture(scope="module", autouse=True)
def children():
    """The four child processes.  They start together when the file's first test begins, so that they run
    beside the in-process tests (five processes on the GPU for the first seconds; the file's and each test's
    time are measured that way), and the switch tests at the end of the file read what they printed.  A run
    that selects other tests of the file only starts them all the same and waits for them at teardown."""
    procs = {}
    for name, (env, *groups) in CHILDREN.items():
        args = [a for mode, cases in groups for a in (mode, ",".join(T.case_id(c) for c in cases))]
        procs[name] = subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "circuit_time_cases.py"), *args],
                                       env={**os.environ, **env}, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    done = {}

    def result(name):
        """{(mode, case id): record} of one child"""
        if name not in done:
            out, err = procs[name].communicate(timeout=170)
            assert procs[name].returncode == 0, err[-2000:]
            recs = [json.loads(line) for line in out.strip().splitlines() if line.startswith("{")]
            want = [(mode, T.case_id(c)) for mode, cases in CHILDREN[name][1:] for c in cases]
            assert [(x["mode"], x["id"]) for x in recs] == want
            assert all(x["finite"] for x in recs)
            done[name] = {(x["mode"], x["id"]): x for x in recs}
        return done[name]

    yield result
    for p in procs.values():        # let a child that nobody read run to its end: none is killed in mid-launch
        try:
            p.communicate(timeout=170)
        except subprocess.TimeoutExpired:
            p.kill()
            p.communicate()


def _hold(what, c, errs, e32_metrics):
    """a child's metrics against the bounds of circuit_shape_cases.check"""
    print(f"{what}: rel_inf " + "  ".join(f"{k} {v:.3e}" for k, v in zip(S.METRICS, errs)))
    for k, v, r in zip(S.METRICS, errs, e32_metrics):
        assert v <= T.bound(c, r), (what, k, v, T.bound(c, r))


def _hold_both(tag, c, r):
    """a 'both' record: the call's own output, the stacks, and stack[:, 0] against the output"""
    cid, e = T.case_id(c), T.e32(c)
    assert r["shape"] == [c.n, 1, c.h, c.w, c.k]
    _hold(f"{tag} {cid} O_1", c, r["O"], e["O"])
    _hold(f"{tag} {cid} stored O_1", c, r["O_1"], e["O_t"][0])
    _hold(f"{tag} {cid} stored I_1", c, r["I_1"], e["I_t"][0])
    if c.n >= 64:
        ref, r32 = T.oracle(c)["O"], T.oracle(c, None, "float32")["O"]
        assert sorted(r["images"]) == sorted(str(i) for i in S.sampled_images(c.n))
        for i in S.sampled_images(c.n):
            _hold(f"{tag} {cid} image {i}", c, r["images"][str(i)], S.metrics(r32[i:i + 1], ref[i:i + 1], c.ssf))
    if c.dtype == "bf16":       # the stack reads the bf16 state map: half an ulp of 7 stored mantissa bits
        assert r["close"], cid
    else:
        assert r["same"] and r["sha"] == r["stack_sha"], cid


def test_o0_direct_switch_at_one_step(children):
    """MP_O0_DIRECT 0 against 1 on the four-step fp32_fft loop at T = 1, n = 2 (rowq_a) and 12 (row8), with
    and without stored states: row(INIT) copying O0 into the C8 map, or ROW_A and ROW_FINAL reading it as
    NHWC, give the same bytes, within the bounds of the oracle"""
    recs = {v: children(f"MP_O0_DIRECT={v}") for v in ("0", "1")}
    for c in T.O0_DIRECT:
        cid = T.case_id(c)
        for v in ("0", "1"):
            assert recs[v]["both", cid]["fft_loop"] == 4
            _hold_both(f"MP_O0_DIRECT={v}", c, recs[v]["both", cid])
        for k in ("sha", "stack_sha"):
            assert recs["0"]["both", cid][k] == recs["1"]["both", cid][k], (cid, k)


@pytest.mark.parametrize("dtype", ["fp32_fft", "bf16"])
def test_six_launch_loop_at_one_step(children, dtype):
    """MP_FFT4=0 at T = 1: the six-launch loop on one stream (n = 2) and on two (n = 66), whose
    `t == T - 1 -> final_out` (mode 1: the NHWC result) is then also their first step.  The call's own
    output -- at n = 66 also the images at the slice edges -- and the stored states against the oracle;
    stack[:, 0] is the output (bf16: to the rounding of the bf16 state map)"""
    recs = children("MP_FFT4=0")
    for c in SIX_CASES[dtype]:
        assert recs["both", T.case_id(c)]["fft_loop"] == 6
        _hold_both("MP_FFT4=0", c, recs["both", T.case_id(c)])


def test_fc_presplit_switch_on_the_one_step_pose_model(children):
    """MP_FC_PRESPLIT=0: the step-0 ROW_FINAL writes the fp32 NHWC map (mode 1) and fc_1 splits it in its K
    loop; within the model-output gate"""
    recs = children("MP_FC_PRESPLIT=0")
    for c in PRESPLIT_CASES:
        err = recs["plain", T.case_id(c)]["out"]
        print(f"MP_FC_PRESPLIT=0 {T.case_id(c)} out: rel_inf {err:.3e} (gate {T.output_gate(c):.0e})")
        assert err <= T.output_gate(c)
