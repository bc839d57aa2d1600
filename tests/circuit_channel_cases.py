"""The ContextualCircuit channel counts the channel-general loop is tested at (CPU and GPU): the case
table, the inputs (regenerated from fixed seeds, read-only) and the float64 / float32 oracle runs
(``hgru_variants_ref.variant_forward``, computed once per process and never modified).

Each case is the smallest shape at which the thing it names can go wrong; metrics and bounds are
``circuit_shape_cases``' (the project gate 1e-4 and the fp32-class rule max(10 * e32, 1e-5))."""
import collections
import functools

import numpy as np

import circuit_shape_cases as S
import hgru_variant_cases as HV
import hgru_variants_ref as V
from helpers import pkg

T = 3
RHO = HV.RHO                            # a non-constant rho where the aux adapts
SEED = 4321
SCOPE = "contextual_circuit"
ORACLE_CHUNK = S.ORACLE_CHUNK

# variant: a name of hgru_variant_cases.VARIANTS; nhwc_loop: 64 channels sent through the new loop
Case = collections.namedtuple("Case", "dtype k n h w ssf variant nhwc_loop", defaults=(False,))

CASES = [
    # odd k (no 16-byte pixel alignment, padded Cin), map smaller than the filter, gated A_in
    Case("fp32_split", 25, 2, 7, 9, 15, "pose"),
    # k below one channel chunk, reads I0, n = 3, widths that are no multiple of 32
    Case("fp32_split", 8, 3, 20, 28, 5, "defaults"),
    Case("fp32_split", 24, 2, 16, 32, 5, "mely"),                 # 24 -> 32 Cin padding, mely's beta * I
    Case("fp32_split", 32, 1, 33, 17, 3, "relu"),                 # unbounded states
    Case("fp32_split", 96, 2, 12, 40, 5, "pose"),                 # Cout > 64
    Case("fp32_split", 128, 1, 16, 32, 15, "defaults"),           # widest tested, K = 28800
    Case("fp32_split", 4, 2, 1, 1, 3, "pose"),                    # smallest k, one pixel
    Case("fp32_split", 48, 2, 9, 32, 5, "output_gru_gates"),      # gated B_in
    Case("fp32", 25, 2, 7, 9, 15, "pose"),                        # the exact-fp32 convs
    Case("fp32", 96, 2, 12, 40, 5, "output_gru_gates"),
    Case("fp32", 8, 3, 20, 28, 5, "rectify"),
    # 64 channels on a map the 64-channel tilings reject
    Case("fp32_split", 64, 2, 20, 28, 15, "output_gru_gates", True),
]
STATES = (24, 2, 16, 32, 5)             # k, n, h, w, ssf: per-step state, hidden_init, the device draw
STATES_VARIANTS = ("pose", "defaults")
BATCH = (8, 9, 32, 5, "pose")           # k, h, w, ssf, variant at n = 1, 3 and 66
BATCH_NS = (1, 3, 66)
BATCH_ODD = (25, 9, 32, 5, "pose")      # n = 1 against n = 3
REUSE_K, REUSE_SSF = 24, 5
REUSE_SEQUENCE = [(2, 16, 32), (1, 7, 9), (3, 20, 28), (2, 16, 32)]     # one context, in turn
BOTH_LOOPS = (64, 2, 16, 32, 5)         # k, n, h, w, ssf: today's general loop against the new one
BOTH_VARIANTS = ("defaults", "pose")
# (what, k of the weights, dtype, the weight to replace or None, its shape, MP_ERR_* status)
MP_ERR_WEIGHT, MP_ERR_UNSUPPORTED = -4, -6
REJECTED = [
    ("k25-fp32_fft", 25, "fp32_fft", None, None, MP_ERR_UNSUPPORTED),
    ("k25-bf16", 25, "bf16", None, None, MP_ERR_UNSUPPORTED),
    ("k3", 3, "fp32_split", None, None, MP_ERR_WEIGHT),
    ("k260", 260, "fp32_split", None, None, MP_ERR_WEIGHT),
    ("p_r-24x32", 24, "fp32_split", "p_r", (5, 5, 24, 32), MP_ERR_WEIGHT),
    ("i_r-64x64", 24, "fp32_split", "i_r", (1, 1, 64, 64), MP_ERR_WEIGHT),
]


def case_id(c):
    return f"{c.dtype}-k{c.k}-n{c.n}-{c.h}x{c.w}-ssf{c.ssf}-{c.variant}" + ("-nhwc" if c.nhwc_loop else "")


def shape_of(c):
    return c.k, c.n, c.h, c.w, c.ssf


def aux_of(variant):
    return V.full_aux(HV.VARIANTS[variant])


def derived_flags(variant):
    """circuit_var.hpp make_variant, restated: the flags the epilogue kernels branch on"""
    a = aux_of(variant)
    it = a['integration_type']
    return dict(gru_gates=bool(a['gru_gates']), out_gates=bool(a['output_gru_gates']),
                blend_in=it != 'control' and not a['gru_gates'],
                blend_out=it == 'mely' or (it == 'alternate' and not a['output_gru_gates']),
                rectify=a['rectify_weights'] is False,
                mult=bool(a['multiplicative_excitation']) and it != 'mely', adapt=bool(a['adapation']))


def _freeze(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def weights(k, ssf):
    """every variable any variant reads at k channels, float32"""
    W = pkg().weights
    table = W.hgru_circuit_vars(k=k, ssf=ssf, timesteps=T, scope=SCOPE, zeta=True, xi=True)
    w = {v.name: W.synth_value(v, SEED + k, T) for v in table}
    w[f"{SCOPE}/rho"] = RHO.copy()
    return {n: _freeze(a) for n, a in w.items()}


def variant_weights(variant, k, ssf):
    """the weights the facade's table names for this aux"""
    M = pkg().hgru_module
    W = pkg().weights
    table = W.hgru_circuit_vars(k=k, ssf=ssf, timesteps=T, scope=SCOPE,
                                **M.variable_flags(M.merged_aux(HV.VARIANTS[variant])))
    return {v.name: weights(k, ssf)[v.name] for v in table}


@functools.lru_cache(maxsize=None)
def inputs(k, n, h, w):
    """X, O0, I0 [n, h, w, k] float32; image i is the same at every n"""
    W = pkg().weights
    s = SEED + 17 * k + 7 * h + 3 * w
    out = []
    for j, nm in enumerate(("X", "O0", "I0")):
        imgs = [W.synth_hidden((1, h, w, k), seed=s + 100 * j + 1000 * i, name=nm, limit=1.0) for i in range(n)]
        out.append(_freeze(np.concatenate(imgs)))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def oracle(k, n, h, w, ssf, variant, precision="float64", hidden_init="random"):
    """(O_T, I_T, [O_t], [I_t]) in ``precision``; batches above ORACLE_CHUNK in chunks (images are
    independent, pinned on the CPU); hidden_init 'zeros' / 'identity' replace both initial states"""
    dt = np.dtype(precision).type
    X, O0, I0 = inputs(k, n, h, w)
    if hidden_init != "random":
        O0 = I0 = X if hidden_init == "identity" else np.zeros_like(X)
    wts = {nm: a.astype(dt) for nm, a in weights(k, ssf).items()}
    parts = [V.variant_forward(X[i:i + ORACLE_CHUNK].astype(dt), O0[i:i + ORACLE_CHUNK].astype(dt),
                               I0[i:i + ORACLE_CHUNK].astype(dt), wts, aux_of(variant), T, scope=SCOPE, keep_steps=True)
             for i in range(0, n, ORACLE_CHUNK)]
    O = _freeze(np.concatenate([p[0] for p in parts]))
    I = _freeze(np.concatenate([p[1] for p in parts]))
    so = [_freeze(np.concatenate([p[2][t] for p in parts])) for t in range(T)]
    si = [_freeze(np.concatenate([p[3][t] for p in parts])) for t in range(T)]
    return O, I, so, si


@functools.lru_cache(maxsize=None)
def e32(k, n, h, w, ssf, variant, hidden_init="random"):
    """the three metrics of the float32 oracle against the float64 one, per output"""
    a = oracle(k, n, h, w, ssf, variant, "float64", hidden_init)
    b = oracle(k, n, h, w, ssf, variant, "float32", hidden_init)
    return {"O": S.metrics(b[0], a[0], ssf), "I": S.metrics(b[1], a[1], ssf),
            "O_t": [S.metrics(y, x, ssf) for x, y in zip(a[2], b[2])],
            "I_t": [S.metrics(y, x, ssf) for x, y in zip(a[3], b[3])]}
