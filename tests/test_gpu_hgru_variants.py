"""GPU: the general ContextualCircuit loop (conv -> P map -> epilogue kernel per half-step) for
every named variant and compute dtype against the float64 variant oracle
(tests/hgru_variants_ref.py), at the project's fp32 gate; T = 3, so two state hand-overs exercise
the forget gates, the rho[t] indexing and the state buffers.  Inputs and oracle results are shared
(tests/hgru_variant_cases.py)."""
import ctypes

import numpy as np
import pytest

import hgru_variant_cases as C
from helpers import FP32_REL_TOL, pkg, rel_inf

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

CASES = [(name, dt) for name in C.VARIANTS for dt in C.SHAPES if dt == "fp32_fft" or name not in C.FFT_ONLY]


def _cuda(a):
    return torch.from_numpy(np.array(a)).cuda()      # a copy: the shared inputs are read-only


def _circuit(name, shape, store_states=False, hidden_init="random"):
    M = pkg().hgru_module
    aux = dict(C.VARIANTS[name], store_states=store_states, hidden_init=hidden_init)
    X = C.inputs(shape)[0]
    cc = M.ContextualCircuit(_cuda(X), timesteps=C.T, SSF=shape[3], aux=aux)
    cc.weights = C.variant_weights(name, shape[3])
    return cc


def _build(name, dtype, shape, store_states=False, alt_i0=False, general_loop=True):
    _, O0, I0, I0b = C.inputs(shape)
    cc = _circuit(name, shape, store_states)
    h1 = _cuda(I0b if alt_i0 else I0) if general_loop else None    # the fused pose loop takes no I0
    out, w, _ = cc.build(h2_init=_cuda(O0), h1_init=h1, compute_dtype=dtype, general_loop=general_loop)
    return out.cpu().numpy(), w


def _check(got, ref, what):
    r = rel_inf(got, ref)
    print(f"{what}: rel_inf {r:.3e}")
    assert r <= FP32_REL_TOL, (what, r)


@pytest.mark.parametrize("name,dtype", CASES, ids=[f"{n}-{d}" for n, d in CASES])
def test_variant_matches_oracle(name, dtype):
    shape = C.SHAPES[dtype]
    ref_O, ref_I, ref_so, ref_si = C.oracle(name, shape)
    if name != "pose":   # the test cannot pass with the variant's flag ignored
        assert rel_inf(ref_O, C.oracle("pose", shape)[0]) >= 1e-2
    O, w = _build(name, dtype, shape)
    _check(O, ref_O, "O_T")
    _check(w['I'].cpu().numpy(), ref_I, "I_T")
    sO, w = _build(name, dtype, shape, store_states=True)
    sI = w['store_I'].cpu().numpy()
    assert sO.shape == (shape[0], C.T) + O.shape[1:]
    for t in range(C.T):
        _check(sO[:, t], ref_so[t], f"O_{t + 1}")
        _check(sI[:, t], ref_si[t], f"I_{t + 1}")
    assert np.array_equal(sO[:, -1], O)
    if name == "pose":   # the same aux through the fused loop: both inside the gate of the oracle
        fused, _ = _build(name, dtype, shape, general_loop=False)
        _check(fused, ref_O, "fused O_T")
        print(f"general vs fused: rel_inf {rel_inf(O, fused):.3e}")


def test_module_defaults_ssf15():
    """ContextualCircuit(X, T, SSF=15).build() with no aux, n = 3, on the FFT path"""
    M = pkg().hgru_module
    shape = C.SHAPE_SSF15
    X, O0, I0, _ = C.inputs(shape)
    ref_O, ref_I, _, _ = C.oracle("defaults", shape)
    assert rel_inf(ref_O, C.oracle("pose", shape)[0]) >= 1e-2
    cc = M.ContextualCircuit(_cuda(X), C.T, SSF=15)
    cc.weights = C.variant_weights("defaults", 15)
    O, w, _ = cc.build(h2_init=_cuda(O0), h1_init=_cuda(I0), compute_dtype="fp32_fft")
    _check(O.cpu().numpy(), ref_O, "O_T")
    _check(w['I'].cpu().numpy(), ref_I, "I_T")
    assert sorted(k for k in w if k not in ("I", "p_t")) == sorted(
        ["p_r", "i_r", "i_b", "o_r", "o_b", "beta", "nu", "gamma", "kappa", "omega", "lateral_bias"])


@pytest.mark.parametrize("name", ["defaults", "mely_gru", "pose", "control"])
def test_initial_i_is_live_exactly_where_it_is_read(name):
    shape = C.SHAPES["fp32_fft"]
    live = pkg().hgru_module.reads_previous_i(pkg().hgru_module.merged_aux(C.VARIANTS[name]))
    a, _ = _build(name, "fp32_fft", shape)
    b, _ = _build(name, "fp32_fft", shape, alt_i0=True)
    ra, rb = C.oracle(name, shape)[0], C.oracle(name, shape, alt_i0=True)[0]
    if live:
        assert rel_inf(rb, ra) >= 1e-2          # the two I0 move the oracle's O_T
        _check(a, ra, "O_T (I0)")
        _check(b, rb, "O_T (second I0)")
    else:
        assert np.array_equal(ra, rb) and np.array_equal(a, b)


@pytest.mark.parametrize("hidden_init", ["zeros", "identity"])
def test_hidden_init_sets_both_states(hidden_init):
    import hgru_variants_ref as V
    shape = C.SHAPES["fp32_fft"]
    X = C.inputs(shape)[0].astype(np.float64)
    h0 = X if hidden_init == "identity" else np.zeros_like(X)
    w64 = {k: v.astype(np.float64) for k, v in C.weights(shape[3]).items()}
    ref_O, ref_I = V.variant_forward(X, h0, h0, w64, C.aux_of("defaults"), C.T, scope=C.SCOPE)
    cc = _circuit("defaults", shape, hidden_init=hidden_init)
    O, w, _ = cc.build(compute_dtype="fp32_fft")
    _check(O.cpu().numpy(), ref_O, "O_T")
    _check(w['I'].cpu().numpy(), ref_I, "I_T")
    with pytest.raises(ValueError):
        cc.build(h1_init=_cuda(C.inputs(shape)[2]))


def test_random_hidden_draws_reproduce_on_the_host():
    """hidden_init='random' without h1_init / h2_init: call c draws O0 and I0 on the device as
    weights.synth_hidden(seed=hidden_seed + c) and (seed=hidden_seed_i + c), bit for bit"""
    W = pkg().weights
    shape = C.SHAPES["fp32_fft"]
    cc = _circuit("defaults", shape)
    outs = [cc.build(compute_dtype="fp32_fft")[0].cpu().numpy() for _ in range(2)]
    assert not np.array_equal(outs[0], outs[1])
    for c in range(2):
        o0 = W.synth_hidden(cc.X.shape, seed=cc.hidden_seed + c)
        i0 = W.synth_hidden(cc.X.shape, seed=cc.hidden_seed_i + c)
        assert not np.array_equal(o0, i0)
        want = _circuit("defaults", shape).build(h2_init=_cuda(o0), h1_init=_cuda(i0),
                                                 compute_dtype="fp32_fft")[0].cpu().numpy()
        assert np.array_equal(outs[c], want)


@pytest.mark.parametrize("dtype", ["fp32_fft", "fp32", "fp32_split", "bf16"])
def test_pose_aux_without_general_loop_is_the_old_call(dtype):
    """the pose aux keeps its fused path: build() equals a context driven through
    mp_hgru_circuit_fwd_ex on the same inputs, bit for bit"""
    P = pkg()
    L = P._lib
    shape = C.SHAPES["fp32_split"] if dtype in ("fp32_split", "bf16") else C.SHAPES[dtype]
    X, O0, _, _ = C.inputs(shape)
    got, _ = _build("pose", dtype, shape, general_loop=False)
    ctx = L.Context(L.MP_MODEL_HGRU_CIRCUIT, 0)
    for k, v in C.variant_weights("pose", shape[3]).items():
        ctx.set_weight(k, v)
    ctx.finalize(L.dtype_code(dtype))
    x, o0 = _cuda(X), _cuda(O0)
    out = torch.empty_like(x)
    n, h, w, k = x.shape
    L.check(ctx.lib.mp_hgru_circuit_fwd_ex(ctx.h, x.data_ptr(), o0.data_ptr(), n, h, w, k, C.T, L.MP_HIDDEN_GIVEN,
                                           out.data_ptr(), None, None,
                                           ctypes.c_void_p(L.current_stream(x.device))))
    torch.cuda.synchronize()
    ctx.close()
    assert np.array_equal(got, out.cpu().numpy())


def test_bf16_and_mismatched_calls_are_rejected():
    P = pkg()
    L = P._lib
    shape = C.SHAPES["fp32_fft"]
    with pytest.raises(NotImplementedError, match="bf16"):
        _build("defaults", "bf16", shape)
    ctx = L.Context(L.MP_MODEL_HGRU_CIRCUIT, 0)
    v = L.circuit_variant(C.aux_of("defaults"))
    ctx.set_circuit_variant(v)
    for k, a in C.variant_weights("defaults", shape[3]).items():
        ctx.set_weight(k, a)
    with pytest.raises(L.MonkeyPoseError) as e:
        ctx.finalize(L.MP_DTYPE_BF16)
    assert e.value.code == -6
    ctx.finalize(L.MP_DTYPE_F32_FFT)
    x = _cuda(C.inputs(shape)[0])
    out = torch.empty_like(x)
    with pytest.raises(L.MonkeyPoseError) as e:      # the fused entry on a variant context
        ctx.circuit_fwd(x, x, out, C.T, L.current_stream(x.device))
    assert e.value.code == -2
    other = L.circuit_variant(C.aux_of("mely"))
    with pytest.raises(L.MonkeyPoseError) as e:      # another variant than the finalized one
        ctx.circuit_fwd_var(x, x, x, out, None, C.T, L.current_stream(x.device), other)
    assert e.value.code == -2
    ctx.close()
