"""The time axis of every hGRU loop (CPU and GPU): the case table per loop at ``timesteps = 1`` -- the
module's own default, where the first step is also the last -- at fewer steps than ``rho`` holds and,
without adaptation, at more; the inputs (regenerated from fixed seeds, read-only), the float64 and
float32 oracle runs (once per process, never modified) and the bound each case is held to.

Nothing is restated: weights and inputs are ``MG.circuit_inputs`` (the 64-channel fused loops),
``circuit_channel_cases.variant_weights`` / ``inputs`` (the general and the channel-general loop) and
``pose_layer_cases.pose_weights`` (the pose model) with ``rho`` cut to the case's ``len_rho``; the
oracles are ``oracle.hgru_ref.hgru_forward`` / ``hgru_pose_forward`` and
``hgru_variants_ref.variant_forward`` run with ``timesteps = t_run`` on those weights; metrics and
bounds are ``circuit_shape_cases``'.

``python circuit_time_cases.py [plain|states|both ID,ID,...]...`` runs cases in a child process (the dispatch
switches are read once at library load) and prints one JSON line per case and mode."""
import collections
import functools
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import circuit_channel_cases as CC  # noqa: E402
import circuit_shape_cases as S  # noqa: E402
import hgru_variant_cases as HV  # noqa: E402
import hgru_variants_ref as V  # noqa: E402
from helpers import BF16_REL_TOL, BF16_STATE_REL_TOL, FP32_REL_TOL, HGRU_POSE_AUX, MG, pkg  # noqa: E402

# the loops of mp_abi.hip, by the name the table gives them
FUSED = "fused"          # circuit_range's four-step loop (k_fft4.hip), fp32_fft and bf16
DIRECT = "direct"        # circuit_range's direct-conv loop (k_conv64.hip, k_conv64x3.hip)
SIX = "six"              # MP_FFT4=0: circuit_range's six-launch loop (k_fft.hip), on one stream or two
GENERAL = "general"      # var_circuit, k_circuit_var.hip
NHWC = "nhwc"            # nhwc_circuit, k_circuit_nhwc.hip
POSE = "pose"            # the pose model: backbone, the fused loop at len(rho) steps, the head
LOOPS = (FUSED, DIRECT, SIX, GENERAL, NHWC, POSE)
POSE_AUX_LOOPS = (FUSED, DIRECT, SIX)       # 64 channels, the pose aux, MG.circuit_inputs' weights

# len_rho: the entries of the weights' rho (an aux without adaptation has no rho at all: there it only names
# the step count of the longer run a short one is compared with); t_run: the steps the case runs;
# conv: the channel-general loop's association-field conv (None elsewhere)
Case = collections.namedtuple("Case", "loop dtype n h w ssf variant k len_rho t_run conv",
                              defaults=("pose", 64, 1, 1, None))
SCOPE_RHO = {True: f"{S.SCOPE}/rho", False: f"{CC.SCOPE}/rho"}

# ---- timesteps = 1 -------------------------------------------------------------------------------
T1_FUSED = (
    [Case(FUSED, "fp32_fft", n, 9, 32, 5) for n in (2,      # rowq_a_kernel
                                                    9,      # row8_kernel
                                                    12,     # the MP_O0_DIRECT pair's second batch
                                                    66,     # two batch slices, 64 + 2, on two streams
                                                    130)]   # ntot >= 128: non-temporal maps, col8p on slice one
    + [Case(FUSED, "fp32_fft", 2, 7, 32, 15), Case(FUSED, "fp32_fft", 2, 17, 64, 3)]
    + [Case(FUSED, "bf16", n, 9, 32, 5) for n in (2, 9, 66)])
T1_DIRECT = ([Case(DIRECT, "fp32", n, 16, 32, 3) for n in (1, 2)]
             + [Case(DIRECT, "fp32_split", n, 32, 32, 5) for n in (1, 2)])
T1_SIX = [Case(SIX, d, n, 9, 32, 5) for d in ("fp32_fft", "bf16") for n in (2, 66)]
NO_ADAPT = "output_gru_gates"           # a variant without adaptation (and with a gated B_in)
T1_GENERAL = [Case(GENERAL, d, 2, h, 32, ssf, v) for d, h, ssf in (("fp32_fft", 7, 15), ("fp32", 16, 5))
              for v in ("pose", "defaults", NO_ADAPT)]
T1_NHWC = [
    Case(NHWC, "fp32_split", 2, 7, 9, 5, "pose", 8, conv="direct"),
    Case(NHWC, "fp32_split", 2, 7, 9, 15, "pose", 25, conv="direct"),       # odd k, map smaller than the filter
    Case(NHWC, "fp32_split", 2, 16, 32, 5, "pose", 64, conv="direct"),      # nhwc_loop=True
    Case(NHWC, "fp32_split", 2, 7, 9, 5, "pose", 8, conv="fft"),
    Case(NHWC, "fp32_split", 2, 65, 9, 3, "pose", 4, conv="fft_tiled"),     # two windows
    Case(NHWC, "fp32_split", 2, 7, 9, 5, "defaults", 8, conv="direct"),     # reads I0
]
POSE_MAP = (16, 32)     # the smallest map pose_fwd takes (crop / 2 a multiple of 16 rows and 32 columns)
POSE_WIDTH = 160        # fc_1 outputs, pose_layer_cases' head_32x32_w160
POSE_NS = (2, 12, 66)
T1_POSE = [Case(POSE, d, n, *POSE_MAP, 15) for d in ("fp32_fft", "bf16", "fp32") for n in POSE_NS]
T1 = T1_FUSED + T1_DIRECT + T1_SIX + T1_GENERAL + T1_NHWC + T1_POSE

# ---- fewer steps than rho holds: len(rho) = 3, the non-constant rho of the helpers ------------------
LEN_RHO = 3
SHORT = [c._replace(len_rho=LEN_RHO, t_run=t) for t in (1, 2) for c in (
    Case(FUSED, "fp32_fft", 2, 9, 32, 5), Case(FUSED, "fp32_fft", 9, 9, 32, 5),
    Case(FUSED, "bf16", 9, 9, 32, 5),       # n = 9: its rho draw spreads widest (BF16_MARGIN below)
    Case(GENERAL, "fp32_fft", 2, 7, 32, 15, "pose"), Case(GENERAL, "fp32_fft", 2, 7, 32, 15, "defaults"),
    Case(GENERAL, "fp32_fft", 2, 7, 32, 15, "adapt"),      # 'defaults' holds no rho: this one reads I0 and adapts
    Case(NHWC, "fp32_split", 2, 7, 9, 5, "pose", 8, conv="direct"),
    Case(NHWC, "fp32_split", 2, 7, 9, 5, "pose", 8, conv="fft"))]
# ---- more steps than rho: a variant without adaptation reads no rho ---------------------------------
LONG_T = 4
LONG = [Case(GENERAL, "fp32_fft", 2, 7, 32, 15, "defaults", len_rho=0, t_run=LONG_T),
        Case(NHWC, "fp32_split", 2, 7, 9, 5, "defaults", 8, len_rho=0, t_run=LONG_T, conv="direct")]

ALL_CASES = T1 + SHORT + LONG
# one context at these step counts in turn, then REUSE_SECOND steps on a second input set
REUSE_STEPS = (3, 1, 2, 1, 3)
REUSE_SECOND = 1
REUSE = [Case(FUSED, "fp32_fft", 2, 9, 32, 5, len_rho=LEN_RHO), Case(FUSED, "bf16", 2, 9, 32, 5, len_rho=LEN_RHO),
         Case(GENERAL, "fp32_fft", 2, 7, 32, 15, "adapt", len_rho=LEN_RHO),
         Case(NHWC, "fp32_split", 2, 7, 9, 5, "pose", 8, len_rho=LEN_RHO, conv="direct")]
REUSE_SECOND_N = 3      # the second input set: another batch (other seeds), the same map
O0_DIRECT = [c for c in T1_FUSED if c.dtype == "fp32_fft" and c.n in (2, 12) and (c.h, c.ssf) == (9, 5)]
# bad step counts, per entry point and the loops behind it: mp_hgru_circuit_fwd -> the four-step loop (both
# dtypes), the direct-conv loop, the channel-general loop; mp_hgru_circuit_fwd_var -> the general loop, the
# channel-general loop.  Every one adapts, with len(rho) = 3
REJECT = [Case(FUSED, "fp32_fft", 2, 9, 32, 5, len_rho=LEN_RHO), Case(FUSED, "bf16", 2, 9, 32, 5, len_rho=LEN_RHO),
          Case(DIRECT, "fp32", 1, 16, 32, 3, len_rho=LEN_RHO),
          Case(NHWC, "fp32_split", 2, 7, 9, 5, "pose", 8, len_rho=LEN_RHO, conv="direct"),
          Case(GENERAL, "fp32_fft", 2, 7, 32, 15, "adapt", len_rho=LEN_RHO),
          Case(NHWC, "fp32_split", 2, 7, 9, 5, "adapt", 8, len_rho=LEN_RHO, conv="direct")]
# Step-count sensitivity (tests/test_circuit_time_cases_cpu.py): a run of one step more or fewer, or with rho
# taken from the wrong end, differs from the oracle by at least this many bounds.  The fp32-class bound is
# 1e-5, so the margin asks 1e-3.  The bf16 gate is 2e-2 and 100 gates are 2: between tanh-bounded states
# (|O| <= max|rho|) rel_inf reaches 2 only for a sign flip of the largest entry, and rho = 1 +- 0.1 differs by
# 0.2 / 1.1 at the most, so no input meets it.  A bf16 case is therefore held to two things: its inputs are
# those of an fp32_fft case of the same loop, n, map and step counts, which meets the margin (the loops'
# host code -- the step count, rho[t], the last-step branch -- is shared by both dtypes), and its own
# differences clear BF16_MARGIN gates: a wrong step count then stays >= 2 gates from the oracle after the full
# error a bf16 run is allowed.
SENSITIVITY_MARGIN = 100.0
BF16_MARGIN = 3.0
MP_ERR_ARG = -1         # include/monkeypose.h
# hidden_init 'zeros' / 'identity' at one step (the pose model's n = 2 cases as well)
HIDDEN_CASES = [c for c in T1 if c.n == 2 and (
    (c.loop == FUSED and c.dtype == "fp32_fft" and c.h == 9)
    or (c.loop == GENERAL and c.dtype == "fp32_fft" and c.variant in ("pose", "defaults"))
    or (c.loop == NHWC and c.k == 8 and c.conv == "direct"))]


def case_id(c):
    s = f"{c.loop}-{c.dtype}-n{c.n}-{c.h}x{c.w}-ssf{c.ssf}"
    if c.loop in (GENERAL, NHWC):
        s += f"-{c.variant}"
    if c.loop == NHWC:
        s += f"-k{c.k}-{c.conv}"
    return s + f"-rho{c.len_rho}-t{c.t_run}"


BY_ID = {case_id(c): c for c in ALL_CASES + REUSE}


def adapts(c):
    return c.loop not in (GENERAL, NHWC) or bool(CC.aux_of(c.variant)['adapation'])


def nhwc_loop_flag(c):
    return c.loop == NHWC and c.k == 64


def state_gate(c):
    """the project gate of a state map"""
    return BF16_STATE_REL_TOL if c.dtype == "bf16" else FP32_REL_TOL


def output_gate(c):
    """the project gate of the pose model's output"""
    return BF16_REL_TOL if c.dtype == "bf16" else FP32_REL_TOL


def bound(c, e32_metric):
    """what circuit_shape_cases.check holds one metric of a state map of this case to"""
    return state_gate(c) if c.dtype == "bf16" else min(FP32_REL_TOL, S.fp32_class_bound(e32_metric))


def pose_bucket(n):
    """the pose model's inputs and oracle runs are made once for 12 images and once for 66: a case takes
    the first n of the smallest set that holds it"""
    return min(m for m in (12, max(POSE_NS)) if m >= n)


def _freeze(a):
    a.setflags(write=False)
    return a


# ------------------------------------------------------------------------------------------ inputs
def _key(c):
    """what the inputs and the oracle of a case depend on"""
    fam = "pose" if c.loop == POSE else ("aux64" if c.loop in POSE_AUX_LOOPS else "variant")
    n = pose_bucket(c.n) if c.loop == POSE else c.n
    return fam, c.k, n, c.h, c.w, c.ssf, c.variant if fam == "variant" else "pose", c.len_rho


@functools.lru_cache(maxsize=None)
def _inputs(key):
    fam, k, n, h, w, ssf, variant, len_rho = key
    if fam == "aux64":
        wts, X, O0 = MG.circuit_inputs(n, h, w, ssf, len_rho, *S.seeds(n, h, w, ssf))
        return {nm: _freeze(a) for nm, a in wts.items()}, _freeze(X), _freeze(O0), None
    if fam == "variant":
        X, O0, I0 = CC.inputs(k, n, h, w)
        wts = dict(CC.variant_weights(variant, k, ssf))
        nm = SCOPE_RHO[False]
        if nm in wts:       # an aux without adaptation creates no rho: len_rho is then the longer run's step count only
            assert len_rho > 0, (variant, len_rho)
            wts[nm] = _freeze(CC.RHO[:len_rho].copy())
        return wts, X, O0, I0
    import pose_layer_cases as PL
    Wt = pkg().weights
    wts = dict(PL.pose_weights(h, w, POSE_WIDTH))
    wts[SCOPE_RHO[True]] = _freeze(HV.RHO[:len_rho].copy())     # hgru_pose_vars' rho is ones: a gain that shows
    depth = np.ascontiguousarray(Wt.synth_crops(n, seed=PL.SEED + 11, size=2 * max(h, w))[:, :2 * h, :2 * w])
    return wts, _freeze(depth), _freeze(Wt.synth_hidden((n, h, w, 64), seed=PL.SEED + 12)), None


@functools.lru_cache(maxsize=None)
def _second(key):
    """REUSE_SECOND_N other images on the weights of ``key``"""
    fam, k, n, h, w, ssf, variant, len_rho = key
    wts, m = _inputs(key)[0], REUSE_SECOND_N
    if fam == "aux64":
        ws, xs, os_ = S.seeds(n, h, w, ssf)
        _, X, O0 = MG.circuit_inputs(m, h, w, ssf, len_rho, ws, xs + 50, os_ + 50)
        return wts, _freeze(X), _freeze(O0), None
    assert fam == "variant"     # circuit_channel_cases' draw of a taller map, cut to this one
    return (wts,) + tuple(_freeze(np.ascontiguousarray(a[:, 1:h + 1])) for a in CC.inputs(k, m, h + 2, w))


def inputs(c, second=False):
    """(weights, X or the depth crops, O0, I0 or None) of a case.  ``second``: another input set on the same weights (REUSE_SECOND_N images)."""
    if second:
        return _second(_key(c))
    wts, X, O0, I0 = _inputs(_key(c))
    if c.loop == POSE:
        return wts, X[:c.n], O0[:c.n], None
    return wts, X, O0, I0


def rho_of(c):
    """the rho the case's loop indexes, or None where its aux does not adapt"""
    return np.asarray(inputs(c)[0][SCOPE_RHO[c.loop in POSE_AUX_LOOPS + (POSE,)]]) if adapts(c) else None


# ------------------------------------------------------------------------------------------ oracle
def _chunks(n):
    return [slice(i, min(n, i + S.ORACLE_CHUNK)) for i in range(0, n, S.ORACLE_CHUNK)]


@functools.lru_cache(maxsize=None)
def _oracle(key, t, precision, hidden_init, second=False):
    from oracle import hgru_ref as R
    fam = key[0]
    wts, X, O0, I0 = _second(key) if second else _inputs(key)
    dt = np.dtype(precision).type
    parts = []
    for s in _chunks(X.shape[0]):       # images are independent (pinned on the CPU): 32 at a time stay in cache
        if fam == "pose":
            o0 = None if hidden_init != "random" else O0[s].astype(dt)
            out, inter = R.hgru_pose_forward(X[s], wts, o0, t, dt, keep=True, hidden_init=hidden_init)
            parts.append((inter["hgru_steps"][-1], inter["hgru_isteps"][-1], inter["hgru_steps"], inter["hgru_isteps"], out))
            continue
        Xp = X[s].astype(dt)
        o0, i0 = ((O0[s], I0[s] if I0 is not None else None) if hidden_init == "random" else
                  (X[s], X[s]) if hidden_init == "identity" else (np.zeros_like(X[s]),) * 2)
        if fam == "aux64":
            O, so, si = R.hgru_forward(Xp, o0.astype(dt), wts, t, keep_inputs=True)
            parts.append((O, si[-1], so, si))
        else:
            w = {nm: a.astype(dt) for nm, a in wts.items()}
            parts.append(V.variant_forward(Xp, o0.astype(dt), i0.astype(dt), w, CC.aux_of(key[6]), t, scope=CC.SCOPE,
                                           keep_steps=True))
    cat = lambda j: _freeze(np.concatenate([p[j] for p in parts]))
    res = dict(O=cat(0), I=cat(1), O_t=[_freeze(np.concatenate([p[2][i] for p in parts])) for i in range(t)],
               I_t=[_freeze(np.concatenate([p[3][i] for p in parts])) for i in range(t)])
    if fam == "pose":
        res["out"] = cat(4)
    return res


def oracle(c, t=None, precision="float64", hidden_init="random", second=False):
    """{'O', 'I', 'O_t': [...], 'I_t': [...]} (and 'out' of the pose model) after ``t`` steps (default
    t_run) on the case's weights, whose rho holds len_rho entries"""
    if second:
        return _oracle(_key(c), c.t_run if t is None else t, precision, hidden_init, True)
    r = _oracle(_key(c), c.t_run if t is None else t, precision, hidden_init)
    if c.loop == POSE and c.n != pose_bucket(c.n):
        r = {k: ([a[:c.n] for a in v] if isinstance(v, list) else v[:c.n]) for k, v in r.items()}
    return r


def e32(c, t=None, hidden_init="random"):
    """the three metrics of the float32 oracle against the float64 one, per output"""
    a, b = oracle(c, t, "float64", hidden_init), oracle(c, t, "float32", hidden_init)
    return {"O": S.metrics(b["O"], a["O"], c.ssf), "I": S.metrics(b["I"], a["I"], c.ssf),
            "O_t": [S.metrics(y, x, c.ssf) for x, y in zip(a["O_t"], b["O_t"])],
            "I_t": [S.metrics(y, x, c.ssf) for x, y in zip(a["I_t"], b["I_t"])]}


def initial_state(c):
    """O0 as the oracle takes it: the given draw, or the pose model's (no map of its own on the host)"""
    return np.asarray(inputs(c)[2], np.float64)


# ----------------------------------------------------------------------------------- running the GPU
def cuda(a):
    import torch
    return torch.from_numpy(np.array(a, dtype=np.float32)).cuda()      # a copy: the shared inputs are read-only


def aux_of_case(c):
    return dict(HGRU_POSE_AUX) if c.loop in POSE_AUX_LOOPS else dict(HV.VARIANTS[c.variant])


def uses_var_entry(c):
    """mp_hgru_circuit_fwd_var (the general loop, and the channel-general loop for every aux but the pose
    one) or mp_hgru_circuit_fwd (the fused loops, and the channel-general loop on the pose aux)"""
    return c.loop == GENERAL or (c.loop == NHWC and c.variant != "pose")


def run(c, t=None, store_states=False, hidden_init="random"):
    """the facade on the case's inputs at ``t`` steps (default t_run) -> {'O' (without store_states), 'I'
    (where the entry point returns it), 'sO', 'sI' (store_states)} as numpy"""
    assert c.loop != POSE
    wts, X, O0, I0 = inputs(c)
    gl = uses_var_entry(c)
    aux = aux_of_case(c)
    aux.update(store_states=store_states, hidden_init=hidden_init)
    cc = pkg().hgru_module.ContextualCircuit(cuda(X), timesteps=c.t_run if t is None else t, SRF=1, SSN=c.ssf,
                                             SSF=c.ssf, aux=aux)
    kw = dict(compute_dtype=c.dtype, general_loop=gl, nhwc_loop=nhwc_loop_flag(c))
    if c.conv:
        kw["nhwc_conv"] = c.conv
    if hidden_init == "random":
        kw["h2_init"] = cuda(O0)
        if gl:
            kw["h1_init"] = cuda(I0)
    out, w, _ = cc.build(weights=wts, **kw)
    res = {}
    if store_states:
        res["sO"], res["sI"] = out.cpu().numpy(), w["store_I"].cpu().numpy()    # (the facade drops the call's O)
    else:
        res["O"] = out.cpu().numpy()
    if "I" in w:
        res["I"] = w["I"].cpu().numpy()
    return res


def context(c):
    """a finalized C-ABI context of the case's loop (the caller closes it)"""
    L = pkg()._lib
    ctx = L.Context(L.MP_MODEL_HGRU_POSE if c.loop == POSE else L.MP_MODEL_HGRU_CIRCUIT, 0)
    if uses_var_entry(c):
        M = pkg().hgru_module
        ctx.set_circuit_variant(L.circuit_variant(M.merged_aux(aux_of_case(c))))
    if nhwc_loop_flag(c):
        ctx.set_nhwc_loop(True)
    if c.conv and c.conv != "direct":
        ctx.set_nhwc_conv(L.NHWC_CONVS[c.conv])
    for nm, v in inputs(c)[0].items():
        ctx.set_weight(nm, v)
    ctx.finalize(L.dtype_code(c.dtype))
    return ctx


def ctx_forward(ctx, c, X, O0, I0, t, out=None, states=False):
    """one call of the case's entry point on the context -> {'O', 'I' (mp_hgru_circuit_fwd_var's i_out), 'sO',
    'sI' (``states``)} as numpy; ``out``: the caller's output tensor (a rejection test's sentinel)"""
    import torch
    L = pkg()._lib
    x, o0 = cuda(X), cuda(O0)
    out = torch.empty_like(x) if out is None else out
    sO = torch.empty((x.shape[0], t) + tuple(x.shape[1:]), device="cuda") if states else None
    sI = torch.empty_like(sO) if states else None
    st = L.current_stream(x.device)
    if uses_var_entry(c):
        var = L.circuit_variant(pkg().hgru_module.merged_aux(aux_of_case(c)))
        i_out = torch.empty_like(x)
        ctx.circuit_fwd_var(x, o0, cuda(I0), out, i_out, t, st, var, 0, sO, sI)
    else:
        i_out = None
        ctx.circuit_fwd(x, o0, out, t, st, 0, sO, sI)
    torch.cuda.synchronize()
    res = {"O": out.cpu().numpy()}
    if i_out is not None:
        res["I"] = i_out.cpu().numpy()
    if states:
        res["sO"], res["sI"] = sO.cpu().numpy(), sI.cpu().numpy()
    return res


def pose_forward(ctx, c, store_states=False, hidden_init="random"):
    """one forward of the pose model -> {'out', 'sO', 'sI'} as numpy"""
    import torch
    L = pkg()._lib
    _, depth, O0, _ = inputs(c)
    out = torch.empty((c.n, 69), device="cuda")
    taps = {}
    if store_states:
        T = ctx.info("timesteps")
        taps = {k: torch.empty((c.n, T, c.h, c.w, 64), device="cuda") for k in ("states_O", "states_I")}
    o0 = cuda(O0) if hidden_init == "random" else None
    ctx.pose_fwd_taps(cuda(depth), o0, out, taps, L.current_stream(), L.MP_HIDDEN[hidden_init])
    torch.cuda.synchronize()
    res = {"out": out.cpu().numpy()}
    if store_states:
        res["sO"], res["sI"] = taps["states_O"].cpu().numpy(), taps["states_I"].cpu().numpy()
    return res


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


CHILD_MODES = ("plain", "states", "both")


def child_record(c, mode):
    """what a child process reports of one case: hashes of the output bytes and the metrics against float64
    (the parent holds them to the bounds).  'plain': the call's own output (from 64 images on also the images
    at the batch-slice edges, each on its own); 'states': the store_states call's stacks; 'both': the two,
    and whether stack[:, 0] is the plain output bit for bit ('same') and to the rounding of a bf16 state map
    ('close', 2^-8 of the value)"""
    assert mode in CHILD_MODES
    ref, rec, got = oracle(c), {}, []
    if c.loop == POSE:
        assert mode == "plain"
        ctx = context(c)
        r = pose_forward(ctx, c)
        ctx.close()
        return dict(sha=sha(r["out"]), out=S.rel_inf(r["out"], ref["out"]), finite=bool(np.isfinite(r["out"]).all()))
    if mode != "states":
        plain = run(c)["O"]
        got.append(plain)
        rec.update(sha=sha(plain), O=S.metrics(plain, ref["O"], c.ssf))
        if c.n >= 64:
            rec["images"] = {str(i): S.metrics(plain[i:i + 1], ref["O"][i:i + 1], c.ssf) for i in S.sampled_images(c.n)}
    if mode != "plain":
        r = run(c, store_states=True)
        got += [r["sO"], r["sI"]]
        rec.update(shape=list(r["sO"].shape), stack_sha=sha(r["sO"][:, -1]),
                   O_1=S.metrics(r["sO"][:, -1], ref["O_t"][-1], c.ssf), I_1=S.metrics(r["sI"][:, -1], ref["I_t"][-1], c.ssf))
    if mode == "both":
        rec["same"] = bool(np.array_equal(r["sO"][:, -1], plain))
        rec["close"] = bool(np.all(np.abs(r["sO"][:, -1] - plain) <= 2.0 ** -8 * np.abs(plain)))
    ctx = context(c)
    rec["fft_loop"] = ctx.info("fft_loop") if c.loop in (FUSED, SIX) else 0
    ctx.close()
    rec["finite"] = all(bool(np.isfinite(a).all()) for a in got)
    return rec


if __name__ == "__main__":
    for mode, ids in zip(sys.argv[1::2], sys.argv[2::2]):
        for cid in ids.split(","):
            print(json.dumps({"id": cid, "mode": mode, **child_record(BY_ID[cid], mode)}), flush=True)
