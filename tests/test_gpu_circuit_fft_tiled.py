"""GPU: the tiled FFT association-field conv (nhwc_conv='fft_tiled': overlap-save over 64 x 64 windows through
cn_fft_fwd, cn_spec_gemm, cn_fft_inv of k_circuit_fft.hip) at every case of tests/circuit_fft_tiled_cases.py
against the float64 oracle, on the three error metrics of circuit_shape_cases and on the seam band, held to
the project gate and to max(10 * e32, 1e-5) -- the bounds of the direct conv, no new tolerance; per-step
states; bit equality with 'fft' on maps of one window; batch invariance, determinism and a conv chunk that
ends inside an image; one context serving several maps; the tiled conv against the direct one; and the
refusals, before any launch."""
import numpy as np
import pytest

import circuit_channel_cases as C
import circuit_fft_cases as F
import circuit_fft_tiled_cases as FT
import circuit_shape_cases as S
import hgru_variant_cases as HV
from helpers import pkg

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

MP_ERR_ARG, MP_ERR_STATE, MP_ERR_UNSUPPORTED = -1, -2, -6


def _cuda(a):
    return torch.from_numpy(np.array(a, dtype=np.float32)).cuda()      # a copy: the shared inputs are read-only


def _build(k, n, h, w, ssf, variant, images=None, nhwc_loop=False, store_states=False, nhwc_conv='fft_tiled'):
    """the facade on the case's inputs (``images``: a slice of the batch) -> (O or the O_t stack, weights)"""
    X, O0, I0 = (a[images] if images is not None else a for a in C.inputs(k, n, h, w))
    cc = pkg().hgru_module.ContextualCircuit(_cuda(X), timesteps=FT.T, SSF=ssf,
                                             aux=dict(HV.VARIANTS[variant], store_states=store_states))
    cc.weights = C.variant_weights(variant, k, ssf)
    gl = variant != "pose"
    out, wts, _ = cc.build(h2_init=_cuda(O0), h1_init=_cuda(I0) if gl else None, compute_dtype=FT.DTYPE,
                           general_loop=gl, nhwc_loop=nhwc_loop, nhwc_conv=nhwc_conv)
    return out.cpu().numpy(), wts


@pytest.mark.parametrize("c", FT.CASES, ids=FT.case_id)
def test_parity(c):
    """O_T (and the final I where the entry point returns it) against the float64 oracle, seam band included"""
    ref_O, ref_I, _, _ = C.oracle(*FT.shape_of(c), c.variant)
    r32_O, r32_I, _, _ = C.oracle(*FT.shape_of(c), c.variant, "float32")
    e = C.e32(*FT.shape_of(c), c.variant)
    O, wts = _build(*FT.shape_of(c), c.variant, nhwc_loop=c.nhwc_loop)
    assert O.shape == (c.n, c.h, c.w, c.k)
    FT.check(f"{FT.case_id(c)} O_T", O, ref_O, c.ssf, e["O"], r32_O)
    if 'I' in wts:
        FT.check(f"{FT.case_id(c)} I_T", wts['I'].cpu().numpy(), ref_I, c.ssf, e["I"], r32_I)
    else:
        assert c.variant == "pose"


@pytest.mark.parametrize("variant", FT.STATES_VARIANTS)
def test_store_states(variant):
    """every step's O_t and I_t; the last stack entry is the plain call's output bit for bit"""
    k, n, h, w, ssf = FT.STATES
    _, _, ref_so, ref_si = C.oracle(k, n, h, w, ssf, variant)
    _, _, r32_so, r32_si = C.oracle(k, n, h, w, ssf, variant, "float32")
    e = C.e32(k, n, h, w, ssf, variant)
    sO, wts = _build(k, n, h, w, ssf, variant, store_states=True)
    sI = wts['store_I'].cpu().numpy()
    assert sO.shape == sI.shape == (n, FT.T, h, w, k)
    for t in range(FT.T):
        FT.check(f"{variant} O_{t + 1}", sO[:, t], ref_so[t], ssf, e["O_t"][t], r32_so[t])
        FT.check(f"{variant} I_{t + 1}", sI[:, t], ref_si[t], ssf, e["I_t"][t], r32_si[t])
    plain, _ = _build(k, n, h, w, ssf, variant)
    assert np.array_equal(sO[:, -1], plain)


@pytest.mark.parametrize("k,n,h,w,ssf,variant", FT.SMALL, ids=lambda v: str(v))
def test_a_map_of_one_window_is_the_fft_conv_bit_for_bit(k, n, h, w, ssf, variant):
    tiled, wt = _build(k, n, h, w, ssf, variant)
    fft, wf = _build(k, n, h, w, ssf, variant, nhwc_conv='fft')
    assert np.array_equal(tiled, fft)
    assert np.array_equal(wt['I'].cpu().numpy(), wf['I'].cpu().numpy())
    S.check(f"k{k} {h}x{w} ssf {ssf} {variant}", tiled, C.oracle(k, n, h, w, ssf, variant)[0], ssf, FT.DTYPE,
            C.e32(k, n, h, w, ssf, variant)["O"])


def test_batch_invariance_and_determinism():
    """65 x 65, ssf 5, k = 8 (4 tiles per image) at n = 1, 3 and 9: image 0's bytes are the same at every n,
    n = 3 is the first three images of n = 9 (36 tiles: two blocks of the product), image 8 is within the
    bounds, a repeated run is bit-identical"""
    k, h, w, ssf, variant = FT.BATCH
    N = max(FT.BATCH_NS)
    ref = C.oracle(k, N, h, w, ssf, variant)[0]
    r32 = C.oracle(k, N, h, w, ssf, variant, "float32")[0]
    outs = {n: _build(k, N, h, w, ssf, variant, images=slice(0, n))[0] for n in FT.BATCH_NS}
    for n in FT.BATCH_NS:
        assert outs[n].shape[0] == n and np.array_equal(outs[n][0], outs[1][0]), n
    assert np.array_equal(outs[3], outs[N][:3])
    for i in (0, 7, 8):
        FT.check(f"n={N} image {i}", outs[N][i:i + 1], ref[i:i + 1], ssf, S.metrics(r32[i:i + 1], ref[i:i + 1], ssf),
                 r32[i:i + 1])
    again = _build(k, N, h, w, ssf, variant)[0]
    assert np.array_equal(again, outs[N])


def _context(wts, dtype=FT.DTYPE, nhwc_loop=False, conv=None):
    L = pkg()._lib
    ctx = L.Context(L.MP_MODEL_HGRU_CIRCUIT, 0)
    for name, v in wts.items():
        ctx.set_weight(name, v)
    if nhwc_loop:
        ctx.set_nhwc_loop(True)
    if conv is not None:
        ctx.set_nhwc_conv(conv)
    ctx.finalize(L.dtype_code(dtype))
    return ctx


def _ctx_fwd(ctx, X, O0):
    L = pkg()._lib
    x, o0 = _cuda(X), _cuda(O0)
    out = torch.empty_like(x)
    ctx.circuit_fwd(x, o0, out, FT.T, L.current_stream(x.device))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def test_a_chunk_that_ends_inside_an_image_changes_no_bit():
    """k = 256, 1 x 250, ssf 3 (5 tiles per image) at n = 20: the conv walks 96 + 4 tiles, the boundary after
    tile 0 of image 19; images 0, 18 and 19 are each the same image run alone, bit for bit, and image 19 is
    within the bounds"""
    L = pkg()._lib
    k, h, w, ssf, variant = FT.CHUNK
    n = FT.CHUNK_N
    wts = C.variant_weights(variant, k, ssf)
    ctx = _context(wts, conv=L.MP_CN_CONV_FFT_TILED)
    chunk = ctx.info("nhwc_fft_chunk")
    assert ctx.info("nhwc_conv") == 2 and chunk == F.chunk_images(k) == 96
    tpi = FT.tiles_per_image(h, w, ssf)
    assert (n - 1) * tpi < chunk < n * tpi
    X, O0, I0 = C.inputs(k, n, h, w)
    whole = _ctx_fwd(ctx, X, O0)
    for i in FT.CHUNK_IMAGES:
        one = _ctx_fwd(ctx, X[i:i + 1], O0[i:i + 1])
        assert np.array_equal(one[0], whole[i]), i
    ctx.close()
    i = n - 1
    # image i alone: C.inputs draws image i from its own seed, so the oracle runs on that one image
    ref, r32 = (_oracle_of(X[i:i + 1], O0[i:i + 1], I0[i:i + 1], k, ssf, variant, p) for p in ("float64", "float32"))
    FT.check(f"n={n} image {i} (chunk {chunk})", whole[i:i + 1], ref, ssf, S.metrics(r32, ref, ssf), r32)


def _oracle_of(X, O0, I0, k, ssf, variant, precision):
    """O_T of hgru_variants_ref.variant_forward on given images, circuit_channel_cases.oracle's call"""
    import hgru_variants_ref as V
    dt = np.dtype(precision).type
    wts = {nm: a.astype(dt) for nm, a in C.weights(k, ssf).items()}
    return V.variant_forward(X.astype(dt), O0.astype(dt), I0.astype(dt), wts, C.aux_of(variant), FT.T,
                             scope=C.SCOPE, keep_steps=True)[0]


def test_one_context_serves_maps_of_different_sizes():
    """(1,65,8) -> (2,20,28) -> (1,12,120) -> (1,65,8) on one k = 8, ssf 15 context: each output is a fresh
    context's bit for bit, the last equals the first"""
    L = pkg()._lib
    k, ssf = FT.REUSE_K, FT.REUSE_SSF
    wts = C.variant_weights("pose", k, ssf)
    ctx = _context(wts, conv=L.MP_CN_CONV_FFT_TILED)
    assert ctx.info("channels") == k and ctx.info("nhwc_loop") == 1 and ctx.info("nhwc_conv") == 2
    outs = []
    for n, h, w in FT.REUSE_SEQUENCE:
        X, O0, _ = C.inputs(k, n, h, w)
        outs.append(_ctx_fwd(ctx, X, O0))
        fresh = _context(wts, conv=L.MP_CN_CONV_FFT_TILED)
        want = _ctx_fwd(fresh, X, O0)
        fresh.close()
        assert np.array_equal(outs[-1], want), (n, h, w)
        FT.check(f"call {len(outs)} n{n} {h}x{w}", outs[-1], C.oracle(k, n, h, w, ssf, "pose")[0], ssf,
                 C.e32(k, n, h, w, ssf, "pose")["O"], C.oracle(k, n, h, w, ssf, "pose", "float32")[0])
    ctx.close()
    assert np.array_equal(outs[0], outs[-1])


def test_tiled_against_direct():
    k, n, h, w, ssf, variant = FT.AGAINST_DIRECT
    ref = C.oracle(k, n, h, w, ssf, variant)[0]
    r32 = C.oracle(k, n, h, w, ssf, variant, "float32")[0]
    e = C.e32(k, n, h, w, ssf, variant)["O"]
    tiled, _ = _build(k, n, h, w, ssf, variant)
    direct, _ = _build(k, n, h, w, ssf, variant, nhwc_conv='direct')
    FT.check("tiled fft conv O_T", tiled, ref, ssf, e, r32)
    FT.check("direct conv O_T", direct, ref, ssf, e, r32)
    print(f"tiled fft vs direct conv: rel_inf {S.rel_inf(tiled, direct):.3e}")
    assert not np.array_equal(tiled, direct)              # the option is not a no-op


@pytest.mark.parametrize("what,k,dtype", [("k25", 25, "fp32_split"), ("k8-fp32", 8, "fp32"),
                                          ("k64-off-the-loop", 64, "fp32_split")], ids=lambda v: str(v))
def test_refused_at_finalize_before_any_launch(what, k, dtype):
    L = pkg()._lib
    ctx = L.Context(L.MP_MODEL_HGRU_CIRCUIT, 0)
    for nm, v in C.variant_weights("pose", k, 5).items():
        ctx.set_weight(nm, v)
    ctx.set_nhwc_conv(L.MP_CN_CONV_FFT_TILED)
    with pytest.raises(L.MonkeyPoseError) as e:
        ctx.finalize(L.dtype_code(dtype))
    assert e.value.code == MP_ERR_UNSUPPORTED, str(e.value)
    assert str(k) in str(e.value) and "MP_CN_CONV_FFT_TILED" in str(e.value)
    if k == 64:
        assert "MP_DTYPE_F32_FFT" in str(e.value)
    x = torch.zeros((1, 65, 4, k), device="cuda")
    out = torch.full_like(x, 7.0)
    with pytest.raises(L.MonkeyPoseError) as e2:      # not finalized: no forward either
        ctx.circuit_fwd(x, x, out, FT.T, L.current_stream(x.device))
    assert e2.value.code == MP_ERR_STATE
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    ctx.close()


def test_set_call_refuses_another_value_and_a_finalized_context():
    L = pkg()._lib
    ctx = L.Context(L.MP_MODEL_HGRU_CIRCUIT, 0)
    assert ctx.lib.mp_circuit_set_nhwc_conv(ctx.h, 3) == MP_ERR_ARG
    assert ctx.lib.mp_circuit_set_nhwc_conv(ctx.h, -1) == MP_ERR_ARG
    ctx.close()
    ctx = _context(C.variant_weights("pose", 8, 15), conv=L.MP_CN_CONV_FFT_TILED)
    assert ctx.lib.mp_circuit_set_nhwc_conv(ctx.h, L.MP_CN_CONV_FFT) == MP_ERR_STATE
    assert ctx.info("nhwc_conv") == 2
    # and the context takes the map 'fft' refuses (tests/test_gpu_circuit_fft.py pins that refusal)
    X, O0, _ = C.inputs(8, 1, 65, 8)
    FT.check("65 x 8 on the tiled context", _ctx_fwd(ctx, X, O0), C.oracle(8, 1, 65, 8, 15, "pose")[0], 15,
             C.e32(8, 1, 65, 8, 15, "pose")["O"], C.oracle(8, 1, 65, 8, 15, "pose", "float32")[0])
    ctx.close()
