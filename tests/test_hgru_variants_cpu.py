"""CPU: the ContextualCircuit variant family -- the variant oracle against the pose oracle, the
facade's acceptance matrix, and the library's host evaluation of the epilogue kernels' rule
(csrc/circuit_var.hpp, the same code the kernels compile) against the oracle."""
import itertools

import numpy as np
import pytest

import hgru_variant_cases as C
import hgru_variants_ref as V
from helpers import HGRU_POSE_AUX, pkg, rel_inf
from oracle import hgru_ref as R


def test_pose_aux_oracle_equals_hgru_ref_exactly():
    shape = C.SHAPES["fp32"]
    X, O0, I0, _ = (a.astype(np.float64) for a in C.inputs(shape))
    w = {k: v.astype(np.float64) for k, v in C.weights(shape[3]).items()}
    O, I, so, si = V.variant_forward(X, O0, I0, w, V.POSE_AUX, C.T, scope=C.SCOPE, keep_steps=True)
    ref, steps, isteps = R.hgru_forward(X, O0, w, C.T, scope=C.SCOPE, keep_inputs=True)
    assert np.array_equal(O, ref)
    for t in range(C.T):
        assert np.array_equal(so[t], steps[t]) and np.array_equal(si[t], isteps[t])
    # the facade's idea of the pose aux is the helpers' (hgru_pose.py:20-39)
    M = pkg().hgru_module
    assert M.is_pose_aux(M.merged_aux(HGRU_POSE_AUX)) and not M.is_pose_aux(M.merged_aux({}))


@pytest.mark.parametrize("name", [n for n in C.VARIANTS if n != "pose"])
def test_named_variants_differ_from_the_pose_aux(name):
    """a GPU test of a named variant cannot pass with its flag ignored: on the shared inputs the
    variant's oracle output is at least 1e-2 (rel_inf) from the pose aux's"""
    for shape in sorted(set(C.SHAPES.values())) + [C.SHAPE_SSF15]:
        pose = C.oracle("pose", shape)[0]
        assert rel_inf(C.oracle(name, shape)[0], pose) >= 1e-2, (name, shape)


@pytest.mark.parametrize("name", list(C.VARIANTS))
def test_live_initial_i(name):
    """two different I0 move O_T by >= 1e-2 exactly for the variants that read the previous I"""
    shape = C.SHAPES["fp32"]
    a, b = C.oracle(name, shape)[0], C.oracle(name, shape, alt_i0=True)[0]
    M = pkg().hgru_module
    live = M.reads_previous_i(M.merged_aux(C.VARIANTS[name]))
    assert live == V.reads_previous_i(C.VARIANTS[name])
    assert live == (name in ("defaults", "output_gru_gates", "additive", "zeta_xi", "no_gamma_beta_nu",
                             "lesion_beta_nu", "lesion_kappa_omega", "rectify", "mely", "mely_gru", "relu",
                             "hard_tanh", "selu", "leaky_relu", "adapt"))
    if live:
        assert rel_inf(b, a) >= 1e-2
    else:
        assert np.array_equal(a, b)


# ---------------------------------------------------------------------------------------------
# facade matrix
# ---------------------------------------------------------------------------------------------
def _x():
    import torch
    return torch.zeros((1, 16, 32, 64))


@pytest.mark.parametrize("name", list(C.VARIANTS))
def test_accepted_aux_constructs(name):
    M = pkg().hgru_module
    cc = M.ContextualCircuit(_x(), timesteps=C.T, SSF=5, aux=dict(C.VARIANTS[name]))
    assert cc.SSF_ext == 5 and cc.p_shape == [5, 5, 64, 64]
    names = [v.name.split("/")[-1] for v in cc.variable_table()]
    aux = C.aux_of(name)
    assert ("rho" in names) == bool(aux['adapation'])
    assert ("zeta" in names) == bool(aux['zeta']) and ("xi" in names) == bool(aux['xi'])
    assert ("beta" in names) == (bool(aux['beta']) and not aux['lesion_beta'])
    assert ("kappa" in names) == (bool(aux['multiplicative_excitation']) and not aux['lesion_kappa'])
    with pytest.raises(TypeError):
        cc.build()                                         # CPU tensor: no CPU fallback


def test_every_flag_combination_constructs():
    M = pkg().hgru_module
    for nl, it, gg, og in itertools.product(("tanh", "relu", "selu", "leaky_relu", "hard_tanh"),
                                            ("alternate", "mely", "control"), (False, True), (False, True)):
        M.ContextualCircuit(_x(), timesteps=2, SSF=15, aux={'recurrent_nl': nl, 'integration_type': it,
                                                            'gru_gates': gg, 'output_gru_gates': og})


REJECTED = [
    ({'rectify_weights': True}, {}, "rectify_weights"),
    ({'gate_filter': 3}, {}, "gate_filter"),
    ({'association_field': False}, {}, "association_field"),
    ({'batch_norm': True}, {}, "batch_norm"),
    ({'dense_connections': True}, {}, "dense_connections"),
    ({'atrous_convolutions': 2}, {}, "atrous_convolutions"),
    ({'dropout': 0.5}, {}, "dropout"),
    ({'recurrent_nl': np.tanh}, {}, "recurrent_nl"),
    ({'recurrent_nl': 'softplus'}, {}, "recurrent_nl"),
    ({'integration_type': 'other'}, {}, "integration_type"),
    ({'hidden_init': 'ones'}, {}, "hidden_init"),
    ({}, {'SSF': [3, 5]}, "SSF"),
    ({}, {'SSF': 29}, "SSF"),
    ({}, {'SSF': 7}, "SSF"),
    ({}, {'strides': [1, 2, 2, 1]}, "strides"),
]


@pytest.mark.parametrize("aux,kw,word", REJECTED, ids=[f"{r[2]}-{i}" for i, r in enumerate(REJECTED)])
def test_rejected_options_raise_naming_the_option(aux, kw, word):
    M = pkg().hgru_module
    args = dict(timesteps=2, SSF=15, aux=aux)
    args.update(kw)
    with pytest.raises(NotImplementedError, match=word):
        M.ContextualCircuit(_x(), **args)


def test_default_ssf_still_raises():
    M = pkg().hgru_module
    with pytest.raises(NotImplementedError, match="SSF"):
        M.ContextualCircuit(_x(), timesteps=2)             # SSF = 29


def test_train_mode_still_raises():
    import torch
    with pytest.raises(NotImplementedError, match="train_mode"):
        pkg().hgru_pose.model().build(torch.zeros((1, 128, 128, 1)), 69, train_mode=True)


def test_pose_model_accepts_only_its_own_aux():
    m = pkg().hgru_pose.model()
    assert m._hidden_init() == "random"                    # the aux check build() makes before any work
    m.aux['integration_type'] = 'mely'
    with pytest.raises(NotImplementedError, match="own aux"):
        m._hidden_init()


def test_default_variable_table_is_unchanged():
    W = pkg().weights
    names = [v.name.split("/")[-1] for v in W.hgru_circuit_vars()]
    assert names == ["p_r", "i_r", "i_b", "o_r", "o_b", "beta", "nu", "gamma", "kappa", "omega", "rho",
                     "lateral_bias"]


# ---------------------------------------------------------------------------------------------
# the host evaluation of the kernels' rule
# ---------------------------------------------------------------------------------------------
RULE_RHO = 1.25


def _rule_case(aux, rng):
    """(library I', library O', oracle I', oracle O') for one aux on random per-pixel inputs, all of
    them float32 values, so that the only difference is the rule's own float32 arithmetic"""
    L = pkg()._lib
    npix = 96
    u = lambda *s: rng.uniform(-1.0, 1.0, s).astype(np.float32)   # noqa: E731
    P, X, O, I, I2, G1, G2 = (u(npix, 64) for _ in range(7))
    names = L.RULE_CONSTS
    wts = {f"s/{nm}": u(64) for nm in names}
    full = V.full_aux(aux)
    c = V.constants({k: v.astype(np.float64) for k, v in wts.items()}, full, "s", np.float64)
    c["lateral_bias"] = wts["s/lateral_bias"].astype(np.float64)
    consts = np.stack([np.broadcast_to(np.asarray(c[nm], np.float64), (64,)) for nm in names]).astype(np.float32)
    d = lambda a: a.astype(np.float64)   # noqa: E731
    rI = V.input_rule(d(P) + c["lateral_bias"], d(X), d(O), d(I), R.sigmoid(d(G1)), c, full)
    rO = V.output_rule(d(P) + c["lateral_bias"], d(I2), d(O), R.sigmoid(d(G2)), c, full, RULE_RHO)
    v = L.circuit_variant(full)
    gI = L.circuit_var_rule_host(v, 0, P, X, O, I, G1, consts)
    gO = L.circuit_var_rule_host(v, 1, P, X, O, I2, G2, consts, rho=RULE_RHO)
    return gI, gO, rI, rO


def test_variant_struct_size_is_checked():
    """mp_circuit_variant carries struct_size like mp_fwd_opts: a struct smaller than the first
    layout, or an enum out of range, is rejected before anything else is read"""
    import ctypes
    L = pkg()._lib
    lib = L.load()
    assert ctypes.sizeof(L.CircuitVariant) == 72                       # the header's layout
    v = L.circuit_variant(V.full_aux({}))
    z = np.zeros((1, 64), np.float32)
    args = [z.ctypes.data_as(ctypes.c_void_p)] * 6
    v.struct_size = 16
    rc = lib.mp_circuit_var_rule_host(ctypes.byref(v), 0, 1, *args, ctypes.c_float(1.0), args[0])
    assert rc == -1 and b"struct_size" in lib.mp_last_error()
    v = L.circuit_variant(V.full_aux({}))
    v.recurrent_nl = 9
    rc = lib.mp_circuit_var_rule_host(ctypes.byref(v), 0, 1, *args, ctypes.c_float(1.0), args[0])
    assert rc == -1 and b"recurrent_nl" in lib.mp_last_error()
    assert lib.mp_circuit_set_variant(None, ctypes.byref(v)) == -1


def test_host_rule_matches_the_oracle():
    """The float32 rule against the oracle's float64 per-pixel expressions, rel_inf <= 1e-6, for
    every nl x integration x gate combination.  Inputs: every map and constant uniform in [-1, 1]
    (inside [-2, 2], nothing overflows), as float32 values on both sides.  The bounded
    nonlinearities set the range: their output is at most 1, so 1e-6 of it allows about 8 float32
    roundings of an argument of magnitude <= 4 (half an ulp there is 1.2e-7), and with maps and
    constants in [-1, 1] the largest argument, kappa (zeta I + gamma P) + omega (zeta I gamma P), is
    at most 3 + 2 after four roundings; at [-2, 2] the same sum reaches 52, where one rounding alone
    is 1.9e-6."""
    rng = np.random.default_rng(5)
    worst = {}
    for nl, it, gg, og, mult, rect in itertools.product(
            ("tanh", "relu", "selu", "leaky_relu", "hard_tanh"), ("alternate", "mely", "control"),
            (False, True), (False, True), (False, True), (None, False)):
        aux = {'recurrent_nl': nl, 'integration_type': it, 'gru_gates': gg, 'output_gru_gates': og,
               'multiplicative_excitation': mult, 'rectify_weights': rect, 'adapation': og != gg,
               'zeta': True, 'xi': True, 'lesion_nu': mult and og}
        gI, gO, rI, rO = _rule_case(aux, rng)
        worst[(nl, it, gg, og, mult, rect)] = (rel_inf(gI, rI), rel_inf(gO, rO))
    bad = {k: v for k, v in worst.items() if max(v) > 1e-6}
    print("worst rel_inf (I', O'):", max(v[0] for v in worst.values()), max(v[1] for v in worst.values()))
    assert not bad, bad
