"""GPU: ContextualCircuit at channel counts other than 64 -- the channel-general loop (NHWC maps, the
graph runtime's implicit-GEMM convs, the epilogue kernels of k_circuit_nhwc.hip) at every case of
tests/circuit_channel_cases.py against the float64 oracle, on the three error metrics of
circuit_shape_cases, held to the project gate and to max(10 * e32, 1e-5); per-step states, the three
hidden_init forms and the device draw; batch invariance and determinism; one context serving several
maps; 64 channels through both loops; and the rejections, before any launch."""
import numpy as np
import pytest

import circuit_channel_cases as C
import circuit_shape_cases as S
import hgru_variant_cases as HV
from helpers import pkg

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def _cuda(a):
    return torch.from_numpy(np.array(a, dtype=np.float32)).cuda()      # a copy: the shared inputs are read-only


def _circuit(X, k, ssf, variant, **aux):
    cc = pkg().hgru_module.ContextualCircuit(_cuda(X), timesteps=C.T, SSF=ssf, aux=dict(HV.VARIANTS[variant], **aux))
    cc.weights = C.variant_weights(variant, k, ssf)
    return cc


def _build(k, n, h, w, ssf, variant, dtype, images=None, general_loop=None, nhwc_loop=False, store_states=False):
    """the facade on the case's inputs (``images``: a slice of the batch) -> (O or the O_t stack, weights);
    the pose aux takes the fused entry point unless ``general_loop``, every other aux the variant one"""
    X, O0, I0 = (a[images] if images is not None else a for a in C.inputs(k, n, h, w))
    cc = _circuit(X, k, ssf, variant, store_states=store_states)
    gl = variant != "pose" if general_loop is None else general_loop
    out, wts, _ = cc.build(h2_init=_cuda(O0), h1_init=_cuda(I0) if gl else None, compute_dtype=dtype,
                           general_loop=gl, nhwc_loop=nhwc_loop)
    return out.cpu().numpy(), wts


@pytest.mark.parametrize("c", C.CASES, ids=C.case_id)
def test_parity(c):
    """O_T (and the final I where the entry point returns it) against the float64 oracle"""
    ref_O, ref_I, _, _ = C.oracle(*C.shape_of(c), c.variant)
    e = C.e32(*C.shape_of(c), c.variant)
    O, wts = _build(*C.shape_of(c), c.variant, c.dtype, nhwc_loop=c.nhwc_loop)
    assert O.shape == (c.n, c.h, c.w, c.k)
    S.check(f"{C.case_id(c)} O_T", O, ref_O, c.ssf, c.dtype, e["O"])
    if 'I' in wts:
        S.check(f"{C.case_id(c)} I_T", wts['I'].cpu().numpy(), ref_I, c.ssf, c.dtype, e["I"])
    else:
        assert c.variant == "pose"


@pytest.mark.parametrize("variant", C.STATES_VARIANTS)
def test_store_states(variant):
    """every step's O_t and I_t; the last stack entry is the plain call's output bit for bit"""
    k, n, h, w, ssf = C.STATES
    _, _, ref_so, ref_si = C.oracle(k, n, h, w, ssf, variant)
    e = C.e32(k, n, h, w, ssf, variant)
    sO, wts = _build(k, n, h, w, ssf, variant, "fp32_split", store_states=True)
    sI = wts['store_I'].cpu().numpy()
    assert sO.shape == sI.shape == (n, C.T, h, w, k)
    for t in range(C.T):
        S.check(f"{variant} O_{t + 1}", sO[:, t], ref_so[t], ssf, "fp32_split", e["O_t"][t])
        S.check(f"{variant} I_{t + 1}", sI[:, t], ref_si[t], ssf, "fp32_split", e["I_t"][t])
    assert np.array_equal(wts['store_O'].cpu().numpy(), sO)
    plain, _ = _build(k, n, h, w, ssf, variant, "fp32_split")
    assert np.array_equal(sO[:, -1], plain)


@pytest.mark.parametrize("variant", C.STATES_VARIANTS)
@pytest.mark.parametrize("hidden_init", ["zeros", "identity"])
def test_hidden_init(variant, hidden_init):
    k, n, h, w, ssf = C.STATES
    ref = C.oracle(k, n, h, w, ssf, variant, "float64", hidden_init)
    e = C.e32(k, n, h, w, ssf, variant, hidden_init)
    cc = _circuit(C.inputs(k, n, h, w)[0], k, ssf, variant, hidden_init=hidden_init)
    O, wts, _ = cc.build(compute_dtype="fp32_split")
    S.check(f"{variant} {hidden_init} O_T", O.cpu().numpy(), ref[0], ssf, "fp32_split", e["O"])
    if 'I' in wts:
        S.check(f"{variant} {hidden_init} I_T", wts['I'].cpu().numpy(), ref[1], ssf, "fp32_split", e["I"])


@pytest.mark.parametrize("variant", C.STATES_VARIANTS)
def test_device_draw_reproduces_on_the_host(variant):
    """hidden_init='random' with no given state: call c draws O0 (and I0) on the device as
    weights.synth_hidden(shape, seed=hidden_seed + c) / (seed=hidden_seed_i + c), bit for bit"""
    W = pkg().weights
    k, n, h, w, ssf = C.STATES
    X = C.inputs(k, n, h, w)[0]
    cc = _circuit(X, k, ssf, variant)
    outs = [cc.build(compute_dtype="fp32_split")[0].cpu().numpy() for _ in range(2)]
    assert not np.array_equal(outs[0], outs[1])
    gl = variant != "pose"
    for c in range(2):
        o0 = W.synth_hidden(X.shape, seed=cc.hidden_seed + c)
        i0 = W.synth_hidden(X.shape, seed=cc.hidden_seed_i + c)
        assert np.abs(o0).max() <= np.sqrt(6.0 / (2 * k)) and np.abs(o0).max() > 0.9 * np.sqrt(6.0 / (2 * k))
        want = _circuit(X, k, ssf, variant).build(h2_init=_cuda(o0), h1_init=_cuda(i0) if gl else None,
                                                  compute_dtype="fp32_split", general_loop=gl)[0].cpu().numpy()
        assert np.array_equal(outs[c], want), c


def test_batch_invariance_and_determinism():
    """9 x 32, ssf 5, k = 8 at n = 1, 3 and 66: image 0's bytes are the same at every n, images 31, 32
    and 65 of n = 66 are within the bounds, and a repeated run is bit-identical"""
    k, h, w, ssf, variant = C.BATCH
    N = max(C.BATCH_NS)
    ref = C.oracle(k, N, h, w, ssf, variant)[0]
    r32 = C.oracle(k, N, h, w, ssf, variant, "float32")[0]
    outs = {n: _build(k, N, h, w, ssf, variant, "fp32_split", images=slice(0, n))[0] for n in C.BATCH_NS}
    for n in C.BATCH_NS:
        assert outs[n].shape[0] == n and np.array_equal(outs[n][0], outs[1][0]), n
    assert np.array_equal(outs[3], outs[N][:3])
    for i in (0, 31, 32, 65):
        S.check(f"n={N} image {i}", outs[N][i:i + 1], ref[i:i + 1], ssf, "fp32_split",
                S.metrics(r32[i:i + 1], ref[i:i + 1], ssf))
    S.check(f"n={N}", outs[N], ref, ssf, "fp32_split", S.metrics(r32, ref, ssf))
    again = _build(k, N, h, w, ssf, variant, "fp32_split")[0]
    assert np.array_equal(again, outs[N])


def test_batch_invariance_odd_k():
    k, h, w, ssf, variant = C.BATCH_ODD
    three = _build(k, 3, h, w, ssf, variant, "fp32_split")[0]
    S.check("k=25 n=3", three, C.oracle(k, 3, h, w, ssf, variant)[0], ssf, "fp32_split", C.e32(k, 3, h, w, ssf, variant)["O"])
    for i in range(3):
        one = _build(k, 3, h, w, ssf, variant, "fp32_split", images=slice(i, i + 1))[0]
        assert np.array_equal(one[0], three[i]), i
    assert np.array_equal(three, _build(k, 3, h, w, ssf, variant, "fp32_split")[0])


def _context(dtype, wts, nhwc_loop=False):
    L = pkg()._lib
    ctx = L.Context(L.MP_MODEL_HGRU_CIRCUIT, 0)
    for name, v in wts.items():
        ctx.set_weight(name, v)
    if nhwc_loop:
        ctx.set_nhwc_loop(True)
    ctx.finalize(L.dtype_code(dtype))
    return ctx


def _ctx_fwd(ctx, X, O0):
    L = pkg()._lib
    x, o0 = _cuda(X), _cuda(O0)
    out = torch.empty_like(x)
    ctx.circuit_fwd(x, o0, out, C.T, L.current_stream(x.device))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def test_one_context_serves_maps_of_different_sizes():
    """(2,16,32) -> (1,7,9) -> (3,20,28) -> (2,16,32) on one k = 24 context: each output is a fresh
    context's bit for bit, the last equals the first"""
    k, ssf = C.REUSE_K, C.REUSE_SSF
    wts = C.variant_weights("pose", k, ssf)
    ctx = _context("fp32_split", wts)
    assert ctx.info("channels") == k and ctx.info("ssf") == ssf and ctx.info("nhwc_loop") == 1
    outs = []
    for n, h, w in C.REUSE_SEQUENCE:
        X, O0, _ = C.inputs(k, n, h, w)
        outs.append(_ctx_fwd(ctx, X, O0))
        fresh = _context("fp32_split", wts)
        want = _ctx_fwd(fresh, X, O0)
        fresh.close()
        assert np.array_equal(outs[-1], want), (n, h, w)
        S.check(f"call {len(outs)} n{n} {h}x{w}", outs[-1], C.oracle(k, n, h, w, ssf, "pose")[0], ssf, "fp32_split",
                C.e32(k, n, h, w, ssf, "pose")["O"])
    ctx.close()
    assert np.array_equal(outs[0], outs[-1])


@pytest.mark.parametrize("dtype", ["fp32_split", "fp32"])
@pytest.mark.parametrize("variant", C.BOTH_VARIANTS)
def test_64_channels_on_both_loops(variant, dtype):
    """today's general loop and the new loop are each within the bounds of the oracle; without
    nhwc_loop a 64-channel call is the general loop's, bit for bit (it has not moved)"""
    k, n, h, w, ssf = C.BOTH_LOOPS
    if not S.map_ok(dtype, h, w):
        # today's fp32_split loop tiles rows by 32 and rejects this 16-row map (MP_ERR_SHAPE, before any
        # launch): there the new loop alone is held to the oracle, and the two loops meet at 32 rows
        L = pkg()._lib
        with pytest.raises(L.MonkeyPoseError) as err:
            _build(k, n, h, w, ssf, variant, dtype, general_loop=True)
        assert err.value.code == -5
        only, wts = _build(k, n, h, w, ssf, variant, dtype, general_loop=True, nhwc_loop=True)
        e16 = C.e32(k, n, h, w, ssf, variant)
        S.check(f"{variant} {dtype} {h}x{w} nhwc loop O_T", only, C.oracle(k, n, h, w, ssf, variant)[0], ssf, dtype, e16["O"])
        S.check(f"{variant} {dtype} {h}x{w} nhwc loop I_T", wts['I'].cpu().numpy(), C.oracle(k, n, h, w, ssf, variant)[1],
                ssf, dtype, e16["I"])
        h = 32
    ref_O, ref_I, _, _ = C.oracle(k, n, h, w, ssf, variant)
    e = C.e32(k, n, h, w, ssf, variant)
    old, wo = _build(k, n, h, w, ssf, variant, dtype, general_loop=True)
    new, wn = _build(k, n, h, w, ssf, variant, dtype, general_loop=True, nhwc_loop=True)
    S.check(f"{variant} {dtype} general loop O_T", old, ref_O, ssf, dtype, e["O"])
    S.check(f"{variant} {dtype} nhwc loop O_T", new, ref_O, ssf, dtype, e["O"])
    S.check(f"{variant} {dtype} general loop I_T", wo['I'].cpu().numpy(), ref_I, ssf, dtype, e["I"])
    S.check(f"{variant} {dtype} nhwc loop I_T", wn['I'].cpu().numpy(), ref_I, ssf, dtype, e["I"])
    print(f"{variant} {dtype} nhwc vs general: rel_inf {S.rel_inf(new, old):.3e}")
    default, _ = _build(k, n, h, w, ssf, variant, dtype, general_loop=True, nhwc_loop=False)
    assert np.array_equal(default, old)
    if variant == "pose":           # and the fused entry point at 64 channels stays the fused loop
        ctx = _context(dtype, C.variant_weights("pose", k, ssf))
        assert ctx.info("channels") == 64 and ctx.info("nhwc_loop") == 0
        X, O0, _ = C.inputs(k, n, h, w)
        fused = _ctx_fwd(ctx, X, O0)
        ctx.close()
        assert np.array_equal(fused, _build(k, n, h, w, ssf, variant, dtype, general_loop=False)[0])
        S.check(f"{variant} {dtype} fused loop O_T", fused, ref_O, ssf, dtype, e["O"])


@pytest.mark.parametrize("what,k,dtype,name,shape,status", C.REJECTED, ids=[r[0] for r in C.REJECTED])
def test_rejected_at_finalize_before_any_launch(what, k, dtype, name, shape, status):
    L = pkg()._lib
    W = pkg().weights
    if 4 <= k <= 256:
        wts = dict(C.variant_weights("pose", k, 5))
    else:       # outside the range the case table's weights cover
        wts = {v.name: W.synth_value(v, C.SEED, C.T) for v in W.hgru_circuit_vars(k=k, ssf=5, timesteps=C.T, scope=C.SCOPE)}
    if name:
        wts[f"{C.SCOPE}/{name}"] = np.zeros(shape, np.float32)
    ctx = L.Context(L.MP_MODEL_HGRU_CIRCUIT, 0)
    for nm, v in wts.items():
        ctx.set_weight(nm, v)
    with pytest.raises(L.MonkeyPoseError) as e:
        ctx.finalize(L.dtype_code(dtype))
    assert e.value.code == status, str(e.value)
    if status == C.MP_ERR_UNSUPPORTED:
        assert str(k) in str(e.value)           # the message names the channel count
    x = torch.zeros((1, 4, 4, k), device="cuda")
    out = torch.full_like(x, 7.0)
    with pytest.raises(L.MonkeyPoseError) as e2:      # not finalized: no forward either
        ctx.circuit_fwd(x, x, out, C.T, L.current_stream(x.device))
    assert e2.value.code == -2                  # MP_ERR_STATE
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    ctx.close()
    if status == C.MP_ERR_UNSUPPORTED:          # the facade refuses the same thing, naming k
        cc = _circuit(np.zeros((1, 4, 4, k), np.float32), k, 5, "pose")
        with pytest.raises(ValueError, match=str(k)):
            cc.build(compute_dtype=dtype)


def test_wrong_channel_count_of_x_is_rejected_before_any_launch():
    L = pkg()._lib
    ctx = _context("fp32_split", C.variant_weights("pose", 24, 5))
    x = torch.zeros((1, 4, 4, 32), device="cuda")
    out = torch.full_like(x, 7.0)
    with pytest.raises(L.MonkeyPoseError) as e:
        ctx.circuit_fwd(x, x, out, C.T, L.current_stream(x.device))
    assert e.value.code == -5 and "24" in str(e.value)      # MP_ERR_SHAPE
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    ctx.close()
