"""CPU ORACLE of the ContextualCircuit variants -- test infrastructure only.

A float64 NumPy restatement, line by line, of one ``full`` iteration
(``/root/reference/hgru_module.py:825-857``) for every aux the facade accepts
(``monkey-pose_amd/hgru_module.py``): ``circuit_input`` 692-724, ``circuit_output`` 726-756, the
three integration pairs 758-823, the constants of ``prepare_tensors`` 404-497 and the
nonlinearities of ``interpret_nl`` 130-143.  The conv and sigmoid primitives are
``oracle.hgru_ref``'s (looked up at call time, so the structural test can swap symbolic ones in).
With the hgru_pose aux it computes exactly what ``oracle.hgru_ref.hgru_forward`` computes
(``np.array_equal``, tests/test_hgru_variants_cpu.py).

``selu`` / ``leaky_relu``: TensorFlow's documented definitions (scale 1.0507009873554805, alpha
1.6732632423543772; leaky alpha 0.2, ``tf.nn.leaky_relu``'s default).  The reference only names
them (136-139), so their numerics are restated from TF's documentation and unpinned; where they
are applied is pinned structurally (tests/test_hgru_variants_structure.py).
"""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import hgru_ref as R  # noqa: E402

# auxilliary_variables() (hgru_module.py:13-51), the keys that change the forward values
DEFAULT_AUX = {
    'recurrent_nl': 'tanh', 'rectify_weights': None, 'xi': False, 'zeta': False, 'gamma': True,
    'beta': True, 'nu': True, 'output_gru_gates': False, 'multiplicative_excitation': True,
    'gru_gates': False, 'adapation': False, 'integration_type': 'alternate', 'lesion_beta': False,
    'lesion_nu': False, 'lesion_omega': False, 'lesion_kappa': False,
}
# hgru_pose.py:20-39 over the defaults
POSE_AUX = dict(DEFAULT_AUX, gru_gates=True, adapation=True)

SELU_SCALE, SELU_ALPHA, LEAKY_ALPHA = 1.0507009873554805, 1.6732632423543772, 0.2


def full_aux(aux=None):
    a = dict(DEFAULT_AUX)
    a.update(aux or {})
    return a


def _is_sym(x):
    return type(x).__name__ == "Sym"


def recurrent_nl(name):
    """interpret_nl (130-143)"""
    if name == 'tanh':
        return np.tanh                                                        # 132-133
    if name == 'relu':
        return lambda x: np.maximum(x, 0)                                     # 134-135
    if name == 'selu':                                                        # 136-137
        def selu(x):
            if _is_sym(x):
                return type(x)("selu", [x], x.shape)
            return SELU_SCALE * np.where(x > 0, x, SELU_ALPHA * np.expm1(np.minimum(x, 0)))
        return selu
    if name == 'leaky_relu':                                                  # 138-139
        def leaky(x):
            if _is_sym(x):
                return type(x)("leaky_relu", [x, LEAKY_ALPHA], x.shape)
            return np.where(x > 0, x, LEAKY_ALPHA * x)
        return leaky
    if name == 'hard_tanh':
        return lambda x: np.maximum(np.minimum(x, 1), 0)                      # 140-141
    raise NotImplementedError(name)                                           # 142-143


def constants(wts, aux, scope, dt):
    """the degree-of-freedom vectors of prepare_tensors (404-497): a weight, or the constant"""
    def vec(nm):
        return wts[f"{scope}/{nm}"].astype(dt).reshape(-1)
    c = {}
    for nm in ("beta", "nu"):                                                 # 405-429
        if aux[nm] and not aux['lesion_' + nm]:
            c[nm] = vec(nm)
        else:
            c[nm] = 0.0 if aux['lesion_' + nm] else 1.0
    for nm in ("zeta", "gamma", "xi"):                                        # 430-464
        c[nm] = vec(nm) if aux[nm] else 1.0
    for nm in ("kappa", "omega"):                                             # 465-497
        if aux['lesion_' + nm]:
            c[nm] = 0.0
        else:
            c[nm] = vec(nm) if aux['multiplicative_excitation'] else 1.0
    return c


def input_rule(P1, X, O, I, g1, c, aux):
    """the per-pixel part of the input half: P1 = conv + lateral_bias (657), g1 the input gate
    (696-707), O the caller's un-gated output state -> I'"""
    nl = recurrent_nl(aux['recurrent_nl'])
    integ = aux['integration_type']
    if aux['rectify_weights'] is False:
        P1 = np.minimum(P1, 0)                                    # 721-722
    if integ == 'mely':                                           # 758-767
        s = nl(c['xi'] * X - (c['beta'] * I + c['nu']) * P1)
        return s if aux['gru_gates'] else g1 * I + (1 - g1) * s
    if integ == 'control':                                        # 775-780
        return nl(c['xi'] * X - (c['beta'] * O + c['nu']) * P1)
    if integ == 'alternate':                                      # 795-804
        s = nl(c['xi'] * X - (c['beta'] * O + c['nu']) * P1)
        return s if aux['gru_gates'] else g1 * I + (1 - g1) * s
    raise NotImplementedError(integ)                              # 155-157


def output_rule(P2, In, O, g2, c, aux, rho_t=None):
    """the per-pixel part of the output half: P2 = conv + lateral_bias, g2 the output gate
    (729-740), In the un-gated I' -> O' (after the rho gain with adaptation)"""
    nl = recurrent_nl(aux['recurrent_nl'])
    integ = aux['integration_type']
    if aux['rectify_weights'] is False:
        P2 = np.maximum(P2, 0)                                    # 753-754
    e = c['gamma'] * P2
    if integ == 'mely':                                           # 769-773
        s = nl(c['zeta'] * In + e)
        On = g2 * O + (1 - g2) * s
    else:                                                         # 782-793, 806-823
        if aux['multiplicative_excitation']:
            a = c['kappa'] * (c['zeta'] * In + e)
            m = c['omega'] * (c['zeta'] * In * e)
            s = nl(a + m)
        else:
            s = nl(c['zeta'] * In + e)
        if integ == 'control' or aux['output_gru_gates']:
            On = s
        else:
            On = g2 * O + (1 - g2) * s
    if aux['adapation']:                                          # 847-849
        On = On * rho_t
    return On


def variant_step(X, O, I, t, wts, aux, scope="cnn/contextual_circuit"):
    """One ``full`` iteration (825-857) -> (O', I')."""
    aux = full_aux(aux)
    dt = X.dtype
    p_r = wts[f"{scope}/p_r"].astype(dt)
    i_r = wts[f"{scope}/i_r"].astype(dt)
    o_r = wts[f"{scope}/o_r"].astype(dt)
    i_b = wts[f"{scope}/i_b"].astype(dt).reshape(-1)
    o_b = wts[f"{scope}/o_b"].astype(dt).reshape(-1)
    lat = wts[f"{scope}/lateral_bias"].astype(dt).reshape(-1)
    c = constants(wts, aux, scope, dt)

    # circuit_input (692-724)
    g1 = R.sigmoid(R.conv2d_same(O, i_r) + i_b)                   # 696-707
    A_in = O * g1 if aux['gru_gates'] else O                      # 709-711: rebinds the local O only
    P1 = R.conv2d_same(A_in, p_r) + lat                           # 714-718 -> process_p 657
    In = input_rule(P1, X, O, I, g1, c, aux)                      # self.ii, 831-835: the un-gated O

    # circuit_output (726-756)
    g2 = R.sigmoid(R.conv2d_same(In, o_r) + o_b)                  # 729-740
    B_in = In * g2 if aux['output_gru_gates'] else In             # 742-743: local rebinding again
    P2 = R.conv2d_same(B_in, p_r) + lat                           # 746-750
    rho_t = wts[f"{scope}/rho"].astype(dt).reshape(-1)[t] if aux['adapation'] else None
    On = output_rule(P2, In, O, g2, c, aux, rho_t)                # self.oi, 841-849: the un-gated I'
    return On, In


def reads_previous_i(aux):
    """the previous I is read by the forget gate on the input state (765, 802) and by mely's
    beta * I (762)"""
    aux = full_aux(aux)
    return aux['integration_type'] == 'mely' or (aux['integration_type'] == 'alternate' and not aux['gru_gates'])


def variant_forward(X, O0, I0, wts, aux, timesteps, scope="cnn/contextual_circuit", keep_steps=False):
    """``ContextualCircuit.build`` (872-954) with both initial states explicit -> (O_T, I_T), and
    with ``keep_steps`` also the per-step lists (O_t after the rho gain, I_t) as store_states
    writes them (851-853)."""
    O = O0.astype(X.dtype)
    I = I0.astype(X.dtype)
    so, si = [], []
    for t in range(timesteps):
        O, I = variant_step(X, O, I, t, wts, aux, scope)
        if keep_steps:
            so.append(O.copy())
            si.append(I.copy())
    return (O, I, so, si) if keep_steps else (O, I)
