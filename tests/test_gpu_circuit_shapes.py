"""GPU: the ContextualCircuit kernels at every map shape, filter size and batch dispatch the library
accepts (tests/circuit_shape_cases.py), against the float64 oracle on three error metrics -- the
whole map, the border band of the filter's radius, and the last live row with the last column -- at
the project gate and, for the fp32-class paths, at max(10 * e32, 1e-5) with e32 the float32 oracle's
own error on the same metric.  Heights that are no multiple of 8 run the dead-row branches of the row
kernels, ssf 3 the 3-tap weight builds, the batch cases every row / column kernel choice and cache
policy of the four-step loop, and one context serves maps of different sizes in turn."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import circuit_shape_cases as C
from helpers import HGRU_POSE_AUX, pkg

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cuda(a):
    return torch.from_numpy(np.array(a, dtype=np.float32)).cuda()      # a copy: the shared inputs are read-only


def _shape(c):
    return c.n, c.h, c.w, c.ssf


def _build(X, O0, wts, ssf, dtype, variant=None, I0=None, general_loop=False, store_states=False,
           hidden_init="random"):
    """the facade on the given arrays -> (O or the O_t stack, weights dict) as numpy / as returned"""
    M = pkg().hgru_module
    aux = dict(HGRU_POSE_AUX) if variant in (None, "pose") else C.aux_of(variant)
    aux.update(store_states=store_states, hidden_init=hidden_init)
    cc = M.ContextualCircuit(_cuda(X), timesteps=C.T, SRF=1, SSN=ssf, SSF=ssf, aux=aux)
    kw = {}
    if dtype is not None:
        kw["compute_dtype"] = dtype
    if hidden_init == "random":
        kw["h2_init"] = _cuda(O0)
        if I0 is not None:
            kw["h1_init"] = _cuda(I0)
    out, w, _ = cc.build(weights=wts, general_loop=general_loop, **kw)
    return out.cpu().numpy(), w


def _fused(c, dtype=None):
    wts, X, O0, _ = C.inputs(*_shape(c))
    return _build(X, O0, wts, c.ssf, dtype or c.dtype)[0]


def _context(dtype, wts):
    L = pkg()._lib
    ctx = L.Context(L.MP_MODEL_HGRU_CIRCUIT, 0)
    for k, v in wts.items():
        ctx.set_weight(k, v)
    ctx.finalize(L.dtype_code(dtype))
    return ctx


def _ctx_fwd(ctx, X, O0):
    L = pkg()._lib
    x, o0 = _cuda(X), _cuda(O0)
    out = torch.empty_like(x)
    ctx.circuit_fwd(x, o0, out, C.T, L.current_stream(x.device))
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("c", C.FFT_FUSED, ids=C.case_id)
def test_fft_fused_loop(c):
    """the four-step loop (k_fft4.hip) at heights 1 .. 64, both widths, ssf 3 / 5 / 15"""
    O = _fused(c)
    C.check(C.case_id(c), O, C.oracle(*_shape(c))[0], c.ssf, c.dtype, C.e32(*_shape(c))["O"])


@pytest.mark.parametrize("n", C.BATCH_NS)
def test_batch_dispatch(n):
    """9 x 32, ssf 5 at batches 1 (rowq), 9 (row8, cache-resident policies), 40, 66 (slices 64 + 2 on
    two streams) and 258 (160 + 98: col8p and col8, streamed maps): every image against the oracle,
    and the images at the slice edges bit-identical to their own n = 1 run (batch invariance)"""
    h, w, ssf = C.BATCH_SHAPE
    wts, X, O0, _ = C.inputs(C.BATCH_MAX, h, w, ssf)
    ref = C.oracle(C.BATCH_MAX, h, w, ssf)[0][:n]
    r32 = C.oracle(C.BATCH_MAX, h, w, ssf, None, "float32")[0][:n]
    O = _build(X[:n], O0[:n], wts, ssf, "fp32_fft")[0]
    C.check(f"n={n}", O, ref, ssf, "fp32_fft", C.metrics(r32, ref, ssf))
    worst = max(range(n), key=lambda i: np.abs(O[i] - ref[i]).max())
    C.check(f"n={n} image {worst}", O[worst:worst + 1], ref[worst:worst + 1], ssf, "fp32_fft",
            C.metrics(r32[worst:worst + 1], ref[worst:worst + 1], ssf))
    for i in C.sampled_images(n):
        one = _build(X[i:i + 1], O0[i:i + 1], wts, ssf, "fp32_fft")[0]
        assert np.array_equal(one[0], O[i]), (n, i)


@pytest.mark.parametrize("c", C.BF16, ids=C.case_id)
def test_bf16(c):
    C.check(C.case_id(c), _fused(c), C.oracle(*_shape(c))[0], c.ssf, "bf16")


@pytest.mark.parametrize("c", C.GENERAL, ids=C.case_id)
def test_general_loop(c):
    """launch_fft_fwd / spec_gemm / fft_inv per half-step (the lfft forms for B <= 8, the batched ones
    above) with the epilogue kernels of k_circuit_var.hip: O_T and I_T"""
    wts, X, O0, I0 = C.inputs(*_shape(c))
    ref_O, _, ref_si = C.oracle(*_shape(c), c.variant)
    e = C.e32(*_shape(c), c.variant)
    O, w = _build(X, O0, wts, c.ssf, c.dtype, c.variant, I0 if c.variant == "defaults" else None, general_loop=True)
    C.check(f"{C.case_id(c)} O_T", O, ref_O, c.ssf, c.dtype, e["O"])
    C.check(f"{C.case_id(c)} I_T", w['I'].cpu().numpy(), ref_si[-1], c.ssf, c.dtype, e["I"])


@pytest.mark.parametrize("c", C.DIRECT, ids=C.case_id)
def test_direct_paths(c):
    """the exact fp32 conv (k_conv64.hip) and the f16x3 split conv (k_conv64x3.hip) at ssf 3 / 5 / 15,
    maps wider than 64 included; where the FFT path takes the shape too, its error is within
    max(10 * the exact path's, 1e-5) (test_fft_precision_is_fp32_class's rule)"""
    ref = C.oracle(*_shape(c))[0]
    e = C.e32(*_shape(c))["O"]
    errs = C.check(C.case_id(c), _fused(c), ref, c.ssf, c.dtype, e)
    if C.map_ok("fp32_fft", c.h, c.w):
        if c.dtype != "fp32":
            errs = C.check(f"{C.case_id(c)} as fp32", _fused(c, "fp32"), ref, c.ssf, "fp32", e)
        fft = C.check(f"{C.case_id(c)} as fp32_fft", _fused(c, "fp32_fft"), ref, c.ssf, "fp32_fft", e)
        for k, a, b in zip(C.METRICS, fft, errs):
            assert a <= max(10 * b, C.FP32_CLASS_FLOOR), (k, a, b)


@pytest.mark.parametrize("dtype,hidden_init", [("fp32_fft", "given"), ("fp32_fft", "zeros"), ("fp32_fft", "identity"),
                                               ("bf16", "given")])
def test_store_states_and_hidden_init(dtype, hidden_init):
    """every step's O_t and I_t at 63 x 32 (one dead row), for a given, a zero and an identity initial
    state (and the bf16 maps' stacks for a given one); the last stack entry is the plain call's output
    bit for bit (bf16: to the rounding of the bf16 state map the stack is read from)"""
    c = C.STATES._replace(dtype=dtype)
    wts, X, O0, _ = C.inputs(*_shape(c))
    hi = "random" if hidden_init == "given" else hidden_init
    ref_O, ref_so, ref_si = C.oracle(*_shape(c), None, "float64", hi)
    e = C.e32(*_shape(c), None, hi)
    sO, w = _build(X, O0, wts, c.ssf, c.dtype, store_states=True, hidden_init=hi)
    sI = w['store_I'].cpu().numpy()
    assert sO.shape == sI.shape == (c.n, C.T, c.h, c.w, 64)
    for t in range(C.T):
        C.check(f"{dtype} {hidden_init} O_{t + 1}", sO[:, t], ref_so[t], c.ssf, c.dtype, e["O_t"][t])
        C.check(f"{dtype} {hidden_init} I_{t + 1}", sI[:, t], ref_si[t], c.ssf, c.dtype, e["I_t"][t])
    plain, _ = _build(X, O0, wts, c.ssf, c.dtype, hidden_init=hi)
    C.check(f"{dtype} {hidden_init} O_T", plain, ref_O, c.ssf, c.dtype, e["O"])
    if dtype == "bf16":   # the stack reads the bf16 state map (7 stored mantissa bits, half an ulp <= 2^-8 |v|)
        assert np.all(np.abs(sO[:, -1] - plain) <= 2.0 ** -8 * np.abs(plain))
    else:
        assert np.array_equal(sO[:, -1], plain)


@pytest.mark.parametrize("dtype", ["fp32_fft", "bf16"])
def test_one_context_serves_maps_of_different_sizes(dtype):
    """64 x 64 -> 9 x 32 -> 17 x 64 (a larger batch) -> 1 x 32 -> 64 x 64 on one context: the workspace
    keeps its largest size, and no stale row of Z or of the maps reaches a smaller call -- each output
    is the same call's on a fresh context bit for bit, and the first and last are equal"""
    from oracle import hgru_ref as R
    n0, h0, w0 = C.REUSE_SEQUENCE[0]
    wts = C.inputs(n0, h0, w0, C.REUSE_SSF)[0]      # one weight set for every map of the sequence
    ctx = _context(dtype, wts)
    assert ctx.info("fft_loop") == 4 and ctx.info("ssf") == C.REUSE_SSF
    outs = []
    for n, h, w in C.REUSE_SEQUENCE:
        _, X, O0, _ = C.inputs(n, h, w, C.REUSE_SSF)
        outs.append(_ctx_fwd(ctx, X, O0))
        fresh = _context(dtype, wts)
        want = _ctx_fwd(fresh, X, O0)
        fresh.close()
        assert np.array_equal(outs[-1], want), (n, h, w)
        if len(outs) < len(C.REUSE_SEQUENCE):       # (the last call repeats the first)
            ref = R.hgru_forward(X.astype(np.float64), O0, wts, C.T)
            e = None if dtype == "bf16" else C.metrics(R.hgru_forward(X.astype(np.float32), O0, wts, C.T), ref, C.REUSE_SSF)
            C.check(f"{dtype} call {len(outs)} n{n} {h}x{w}", outs[-1], ref, C.REUSE_SSF, dtype, e)
    ctx.close()
    assert np.array_equal(outs[0], outs[-1])


@pytest.mark.parametrize("dtype,h,w", C.REJECTED, ids=[f"{d}-{h}x{w}" for d, h, w in C.REJECTED])
def test_unsupported_maps_are_rejected_before_any_launch(dtype, h, w):
    L = pkg()._lib
    ctx = _context(dtype, C.inputs(*_shape(C.STATES))[0])
    x = torch.zeros((1, h, w, 64), device="cuda")
    out = torch.full_like(x, 7.0)
    with pytest.raises(L.MonkeyPoseError) as e:
        ctx.circuit_fwd(x, x, out, C.T, L.current_stream(x.device))
    assert e.value.code == -5      # MP_ERR_SHAPE
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    ctx.close()


def test_ssf_7_is_rejected_by_the_facade():
    with pytest.raises(NotImplementedError, match="SSF"):
        pkg().hgru_module.ContextualCircuit(torch.zeros((1, 16, 32, 64), device="cuda"), timesteps=C.T, SSF=7,
                                            aux=HGRU_POSE_AUX)


def test_default_dtype_takes_a_20_row_map():
    """build() with the default compute_dtype: 'auto' sends 20 x 32 to the FFT path"""
    n, h, w, ssf = C.DEFAULT_DTYPE_SHAPE
    wts, X, O0, _ = C.inputs(n, h, w, ssf)
    assert pkg()._lib.resolve_dtype('auto', h, w) == 'fp32_fft'
    O = _build(X, O0, wts, ssf, None)[0]
    C.check(f"auto {h}x{w}", O, C.oracle(n, h, w, ssf)[0], ssf, "fp32_fft", C.e32(n, h, w, ssf)["O"])
    assert np.array_equal(O, _build(X, O0, wts, ssf, "fp32_fft")[0])


_CHILD = r"""
import json, sys
sys.path.insert(0, {tests!r})
import numpy as np, torch
import circuit_shape_cases as C
from helpers import HGRU_POSE_AUX, pkg
P = pkg()
L = P._lib
dtype = {dtype!r}
res = {{}}
for n, h, w, ssf in C.SIX_LAUNCH:
    wts, X, O0, _ = C.inputs(n, h, w, ssf)
    cc = P.hgru_module.ContextualCircuit(torch.from_numpy(np.array(X)).cuda(), timesteps=C.T, SRF=1, SSN=ssf,
                                         SSF=ssf, aux=HGRU_POSE_AUX)
    O, _, _ = cc.build(weights=wts, h2_init=torch.from_numpy(np.array(O0)).cuda(), compute_dtype=dtype)
    O = O.cpu().numpy()
    assert np.isfinite(O).all()
    res[f"{{n}}-{{h}}x{{w}}-{{ssf}}"] = C.metrics(O, C.oracle(n, h, w, ssf)[0], ssf)
ctx = L.Context(L.MP_MODEL_HGRU_CIRCUIT, 0)
for k, v in wts.items():
    ctx.set_weight(k, v)
ctx.finalize(L.dtype_code(dtype))
res["fft_loop"] = ctx.info("fft_loop")
ctx.close()
print(json.dumps(res))
"""


@pytest.mark.parametrize("dtype", ["fp32_fft", "bf16"])
def test_six_launch_loop(dtype):
    """MP_FFT4=0 (read once at library load: a fresh child process): fft_fwd / spec_gemm / inv_a_fwd /
    spec_gemm / fft_inv / epi_b (k_fft.hip) with their clamped loads at 7, 17 and 63 rows"""
    code = _CHILD.format(tests=os.path.join(ROOT, "tests"), dtype=dtype)
    r = subprocess.run([sys.executable, "-c", code], env={**os.environ, "MP_FFT4": "0"}, capture_output=True,
                       text=True, timeout=110)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["fft_loop"] == 6
    gate = C.BF16_STATE_REL_TOL if dtype == "bf16" else C.FP32_REL_TOL
    for n, h, w, ssf in C.SIX_LAUNCH:
        errs = res[f"{n}-{h}x{w}-{ssf}"]
        print(f"MP_FFT4=0 {dtype} n{n} {h}x{w} ssf{ssf}: rel_inf " + "  ".join(f"{k} {e:.3e}" for k, e in zip(C.METRICS, errs)))
        for k, e, e32 in zip(C.METRICS, errs, C.e32(n, h, w, ssf)["O"]):
            assert e <= gate, (k, e)
            if dtype != "bf16":
                assert e <= C.fp32_class_bound(e32), (k, e)
