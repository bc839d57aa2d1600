"""The named ContextualCircuit variants the variant tests share (CPU and GPU), their inputs and
their float64 oracle results (computed once per process and never modified)."""
import functools

import numpy as np

import hgru_variants_ref as V
from helpers import pkg

# aux overrides over the module's own defaults (auxilliary_variables, hgru_module.py:9-51)
VARIANTS = {
    "defaults": {},
    "pose": {'gru_gates': True, 'adapation': True},
    "output_gru_gates": {'output_gru_gates': True},
    "additive": {'multiplicative_excitation': False},
    "zeta_xi": {'zeta': True, 'xi': True},
    "no_gamma_beta_nu": {'gamma': False, 'beta': False, 'nu': False},
    "lesion_beta_nu": {'lesion_beta': True, 'lesion_nu': True},
    "lesion_kappa_omega": {'lesion_kappa': True, 'lesion_omega': True},
    "rectify": {'rectify_weights': False},
    "mely": {'integration_type': 'mely'},
    "mely_gru": {'integration_type': 'mely', 'gru_gates': True},
    "control": {'integration_type': 'control'},
    "relu": {'recurrent_nl': 'relu'},
    "hard_tanh": {'recurrent_nl': 'hard_tanh'},
    "selu": {'recurrent_nl': 'selu'},
    "leaky_relu": {'recurrent_nl': 'leaky_relu'},
    "adapt": {'adapation': True},
}
FFT_ONLY = ("selu", "leaky_relu")
T = 3
RHO = np.array([0.8, 1.15, 0.9], np.float32)      # adapation with a non-constant rho
SEED = 1234
SCOPE = "contextual_circuit"
# (n, h, w, ssf) per compute dtype: the smallest maps the tilings allow
SHAPES = {"fp32_fft": (2, 16, 32, 5), "fp32": (2, 16, 32, 5), "fp32_split": (2, 32, 32, 5)}
SHAPE_SSF15 = (3, 16, 32, 15)                      # one ssf = 15, n = 3 case (fp32_fft)


def aux_of(name):
    return V.full_aux(VARIANTS[name])


@functools.lru_cache(maxsize=None)
def weights(ssf, seed=SEED):
    """every variable any variant reads, float32 (each variant takes the subset its aux creates)"""
    W = pkg().weights
    table = W.hgru_circuit_vars(k=64, ssf=ssf, timesteps=T, scope=SCOPE, zeta=True, xi=True)
    w = {v.name: W.synth_value(v, seed, T) for v in table}
    w[f"{SCOPE}/rho"] = RHO.copy()
    for a in w.values():
        a.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def inputs(shape, seed=SEED):
    """X, O0, I0 and a second I0 [n, h, w, 64] float32"""
    W = pkg().weights
    n, h, w, _ = shape
    out = tuple(W.synth_hidden((n, h, w, 64), seed=seed + j, name=nm, limit=1.0)
                for j, nm in enumerate(("X", "O0", "I0", "I0b")))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def oracle(name, shape, alt_i0=False):
    """float64 (O_T, I_T, [O_t], [I_t]) of the named variant on the shape's inputs"""
    X, O0, I0, I0b = inputs(shape)
    w64 = {k: v.astype(np.float64) for k, v in weights(shape[3]).items()}
    out = V.variant_forward(X.astype(np.float64), O0.astype(np.float64), (I0b if alt_i0 else I0).astype(np.float64),
                            w64, aux_of(name), T, scope=SCOPE, keep_steps=True)
    for a in (out[0], out[1], *out[2], *out[3]):
        a.setflags(write=False)
    return out


def variant_weights(name, ssf):
    """the weights the facade's table names for this aux, from the shared set"""
    M = pkg().hgru_module
    W = pkg().weights
    table = W.hgru_circuit_vars(k=64, ssf=ssf, timesteps=T, scope=SCOPE, **M.variable_flags(M.merged_aux(VARIANTS[name])))
    return {v.name: weights(ssf)[v.name] for v in table}
