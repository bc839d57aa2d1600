"""The ContextualCircuit map shapes, filter sizes and batches the shape tests share (CPU and GPU):
the case table per kernel path, the inputs (regenerated from fixed seeds, read-only), the float64
oracle results (computed once per process and never modified), the three error metrics and the
bounds they are held to.

The map rule of each path is restated here (``map_ok``) next to ``_lib.resolve_dtype`` and pinned by
tests/test_circuit_shape_cases_cpu.py against the case table."""
import collections
import functools

import numpy as np

import hgru_variants_ref as V
from helpers import BF16_STATE_REL_TOL, FP32_REL_TOL, MG, pkg, rel_inf

T = 3                                   # two state hand-overs, a non-constant rho
SCOPE = "cnn/contextual_circuit"        # MG.circuit_inputs' weight names
ORACLE_CHUNK = 32                       # images per oracle run of a larger batch
FP32_CLASS_FLOOR = 1e-5                 # test_fft_precision_is_fp32_class: err <= max(10 * e32, 1e-5)

# n, h, w, ssf, and the loop: None = the fused pose loop, else the general loop's variant name
Case = collections.namedtuple("Case", "dtype n h w ssf variant", defaults=(None,))

FFT_FUSED = [
    Case("fp32_fft", 2, 1, 32, 3),      # a single live row
    Case("fp32_fft", 2, 7, 32, 15),     # fewer rows than the 8 row classes
    Case("fp32_fft", 2, 9, 32, 5),      # one row into the second wave
    Case("fp32_fft", 9, 17, 64, 3),     # B > 8: row8 for row A; full width, short map
    Case("fp32_fft", 2, 33, 64, 5),
    Case("fp32_fft", 2, 63, 32, 5),     # only the last row dead
    Case("fp32_fft", 1, 63, 64, 15),
    Case("fp32_fft", 2, 64, 32, 15),
    Case("fp32_fft", 2, 16, 64, 15),
]
# 9 x 32, ssf 5: rowq (n <= 8); row8 with the ntot <= 32 policies; ntot in 33..63; two slices 64 + 2;
# slices 160 + 98 (col8p on the first, col8 on the second, map_nt on).  One input set of BATCH_MAX
# images; batch n is its first n images
BATCH_SHAPE = (9, 32, 5)
BATCH_NS = (1, 9, 40, 66, 258)
BATCH_MAX = max(BATCH_NS)
BF16 = [
    Case("bf16", 2, 9, 32, 5),
    Case("bf16", 9, 17, 64, 3),
    Case("bf16", 2, 63, 32, 5),
    Case("bf16", 2, 64, 32, 15),
]
GENERAL = [
    Case("fp32_fft", 2, 7, 32, 15, "pose"),
    Case("fp32_fft", 9, 17, 64, 3, "pose"),
    Case("fp32_fft", 2, 63, 32, 5, "pose"),
    Case("fp32_fft", 2, 64, 32, 15, "pose"),
    Case("fp32_fft", 2, 63, 32, 5, "defaults"),    # reads I0
]
DIRECT = [
    Case("fp32", 2, 16, 32, 3),
    Case("fp32", 1, 16, 96, 5),
    Case("fp32", 1, 48, 96, 15),
    Case("fp32_split", 1, 64, 32, 3),
    Case("fp32_split", 1, 96, 64, 5),
    Case("fp32_split", 1, 32, 96, 15),
]
STATES = Case("fp32_fft", 2, 63, 32, 5)            # store_states and hidden_init
SIX_LAUNCH = [(2, 7, 32, 15), (9, 17, 64, 3), (2, 63, 32, 5)]     # MP_FFT4=0, fp32_fft and bf16
REUSE_SSF = 5
REUSE_SEQUENCE = [(2, 64, 64), (2, 9, 32), (9, 17, 64), (1, 1, 32), (2, 64, 64)]   # one context, in turn
DEFAULT_DTYPE_SHAPE = (2, 20, 32, 5)
# (dtype, h, w): MP_ERR_SHAPE before any launch
REJECTED = [("fp32_fft", 65, 32), ("fp32_fft", 32, 96), ("fp32_fft", 32, 16),
            ("bf16", 65, 32), ("bf16", 32, 96), ("bf16", 32, 16),
            ("fp32", 17, 32), ("fp32_split", 48, 32)]

ALL_CASES = (FFT_FUSED + BF16 + GENERAL + DIRECT + [STATES] +
             [Case("fp32_fft", BATCH_MAX, *BATCH_SHAPE)] +
             [Case(d, *s) for s in SIX_LAUNCH for d in ("fp32_fft", "bf16")] +
             [Case(d, n, h, w, REUSE_SSF) for n, h, w in REUSE_SEQUENCE for d in ("fp32_fft", "bf16")] +
             [Case("fp32_fft", *DEFAULT_DTYPE_SHAPE)])


def case_id(c):
    return f"{c.dtype}-n{c.n}-{c.h}x{c.w}-ssf{c.ssf}" + (f"-{c.variant}" if c.variant else "")


def first_slice(n):
    """images of the first batch slice (mp_abi.hip run_circuit): two streams from 64 images on, slices
    of whole 32-image GEMM groups, the first slice takes the larger half"""
    groups = (n + 31) // 32
    return min(n, ((groups + 1) // 2) * 32) if n >= 64 else n


def sampled_images(n):
    """image 0, the last of the first slice, the first of the second slice, n - 1"""
    f = first_slice(n)
    return sorted({0, f - 1, f % n, n - 1})


def map_ok(dtype, h, w):
    """mp_abi.hip check_map: the map sizes each compute dtype's association-field conv takes"""
    if dtype in ("fp32_fft", "bf16"):
        return 1 <= h <= 64 and w in (32, 64)
    if dtype == "fp32_split":
        return h >= 32 and h % 32 == 0 and w >= 32 and w % 32 == 0
    return h >= 16 and h % 16 == 0 and w >= 32 and w % 32 == 0      # 'fp32'


def seeds(n, h, w, ssf):
    """fixed (weight, X, O0) seeds of a shape"""
    s = 7 * h + 3 * w + 11 * ssf + n
    return 5000 + s, 6000 + s, 7000 + s


def _freeze(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def inputs(n, h, w, ssf):
    """(weights, X, O0, I0): MG.circuit_inputs on the shape's seeds, and a second state draw"""
    ws, xs, os_ = seeds(n, h, w, ssf)
    wts, X, O0 = MG.circuit_inputs(n, h, w, ssf, T, ws, xs, os_)
    I0 = pkg().weights.sym_uniform(os_ + 1000, "I0", (n, h, w, 64), 0.5)
    for a in wts.values():
        _freeze(a)
    return wts, _freeze(X), _freeze(O0), _freeze(I0)


def aux_of(variant):
    """the facade's aux of a general-loop variant name (tests/hgru_variant_cases.py VARIANTS)"""
    import hgru_variant_cases as HV
    return dict(HV.VARIANTS[variant])


def oracle(n, h, w, ssf, variant=None, precision="float64", hidden_init="random"):
    return _oracle(n, h, w, ssf, None if variant == "pose" else variant, precision, hidden_init)


@functools.lru_cache(maxsize=None)
def _oracle(n, h, w, ssf, variant, precision, hidden_init):
    """(O_T, [O_t], [I_t]) of the shape's inputs in ``precision``.  The fused loop's pose aux through
    oracle.hgru_ref.hgru_forward, a general-loop variant through hgru_variants_ref.variant_forward;
    hidden_init 'zeros' / 'identity' replace O0 (hgru_module.py:875-892)."""
    from oracle import hgru_ref as R
    if n > ORACLE_CHUNK:   # images are independent (pinned on the CPU): 32 at a time stay in cache
        assert variant is None and hidden_init == "random"
        wts, X, O0, _ = inputs(n, h, w, ssf)
        dt = np.dtype(precision).type
        parts = [R.hgru_forward(X[i:i + ORACLE_CHUNK].astype(dt), O0[i:i + ORACLE_CHUNK], wts, T, keep_inputs=True)
                 for i in range(0, n, ORACLE_CHUNK)]
        O = _freeze(np.concatenate([p[0] for p in parts]))
        so = [_freeze(np.concatenate([p[1][t] for p in parts])) for t in range(T)]
        si = [_freeze(np.concatenate([p[2][t] for p in parts])) for t in range(T)]
        return O, so, si
    wts, X, O0, I0 = inputs(n, h, w, ssf)
    dt = np.dtype(precision).type
    Xp = X.astype(dt)
    O0p = {"random": O0, "zeros": np.zeros_like(X), "identity": X}[hidden_init].astype(dt)
    if variant in (None, "pose"):
        O, so, si = R.hgru_forward(Xp, O0p, wts, T, keep_inputs=True)
    else:
        O, _, so, si = V.variant_forward(Xp, O0p, I0.astype(dt), {k: v.astype(dt) for k, v in wts.items()},
                                         V.full_aux(aux_of(variant)), T, scope=SCOPE, keep_steps=True)
    for a in (O, *so, *si):
        _freeze(a)
    return O, so, si


def regions(h, w, ssf):
    """boolean [h, w] masks: the whole map; the border band of the filter's radius; the last live row
    together with the last column"""
    r = ssf // 2
    y = np.arange(h)[:, None]
    x = np.arange(w)[None, :]
    whole = np.ones((h, w), bool)
    border = (y < r) | (y >= h - r) | (x < r) | (x >= w - r)
    last = (y == h - 1) | (x == w - 1)
    return {"whole": whole, "border": border, "last": last}


METRICS = ("whole", "border", "last")


def metrics(got, ref, ssf):
    """rel_inf of [n, h, w, k] maps on the three regions, each relative to max|ref| of its own region"""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    m = regions(ref.shape[1], ref.shape[2], ssf)
    return tuple(rel_inf(got[:, m[k]], ref[:, m[k]]) for k in METRICS)


def e32(n, h, w, ssf, variant=None, hidden_init="random"):
    return _e32(n, h, w, ssf, None if variant == "pose" else variant, hidden_init)


@functools.lru_cache(maxsize=None)
def _e32(n, h, w, ssf, variant, hidden_init):
    """the three metrics of the oracle run in float32 against its float64 run, per output:
    {'O': ..., 'I': ..., 'O_t': [...], 'I_t': [...]} -- the reference's own single-precision error"""
    a = oracle(n, h, w, ssf, variant, "float64", hidden_init)
    b = oracle(n, h, w, ssf, variant, "float32", hidden_init)
    return {"O": metrics(b[0], a[0], ssf), "I": metrics(b[2][-1], a[2][-1], ssf),
            "O_t": [metrics(y, x, ssf) for x, y in zip(a[1], b[1])],
            "I_t": [metrics(y, x, ssf) for x, y in zip(a[2], b[2])]}


def fp32_class_bound(e):
    """the project's fp32-class rule on one metric, e the float32 oracle's error on that metric"""
    return max(10 * e, FP32_CLASS_FLOOR)


def check(what, got, ref, ssf, dtype, e32_metrics=None, gate_only=False):
    """print the three metrics and hold them to the dtype's bounds: the project gate always, and for
    the fp32-class paths max(10 * e32, 1e-5) (gate_only: a documented exception); returns them"""
    errs = metrics(got, ref, ssf)
    print(f"{what}: rel_inf " + "  ".join(f"{k} {e:.3e}" for k, e in zip(METRICS, errs)))
    assert np.isfinite(np.asarray(got)).all(), what
    gate = BF16_STATE_REL_TOL if dtype == "bf16" else FP32_REL_TOL
    for k, e in zip(METRICS, errs):
        assert e <= gate, (what, k, e)
    if dtype != "bf16" and not gate_only:
        assert e32_metrics is not None
        for k, e, r in zip(METRICS, errs, e32_metrics):
            assert e <= fp32_class_bound(r), (what, k, e, fp32_class_bound(r))
    return errs
