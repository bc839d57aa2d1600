"""GPU: the channel-general loop's FFT association-field conv (nhwc_conv='fft': cn_fft_fwd, cn_spec_gemm,
cn_fft_inv of k_circuit_fft.hip) at every case of tests/circuit_fft_cases.py against the float64 oracle, on
the three error metrics of circuit_shape_cases, held to the project gate and to max(10 * e32, 1e-5) -- the
bounds of the direct conv, no new tolerance; per-step states; batch invariance, determinism and the conv's
chunking; one context serving several maps; the FFT conv against the direct one and against the 64-channel
FFT path; the default left alone; and the refusals, before any launch."""
import numpy as np
import pytest

import circuit_channel_cases as C
import circuit_fft_cases as F
import circuit_shape_cases as S
import hgru_variant_cases as HV
from helpers import pkg

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

MP_ERR_STATE, MP_ERR_SHAPE, MP_ERR_UNSUPPORTED = -2, -5, -6


def _cuda(a):
    return torch.from_numpy(np.array(a, dtype=np.float32)).cuda()      # a copy: the shared inputs are read-only


def _build(k, n, h, w, ssf, variant, images=None, general_loop=None, nhwc_loop=False, store_states=False,
           dtype=F.DTYPE, **conv):
    """the facade on the case's inputs (``images``: a slice of the batch) -> (O or the O_t stack, weights);
    ``conv``: nhwc_conv='fft' / 'direct', or nothing at all"""
    X, O0, I0 = (a[images] if images is not None else a for a in C.inputs(k, n, h, w))
    cc = pkg().hgru_module.ContextualCircuit(_cuda(X), timesteps=F.T, SSF=ssf,
                                             aux=dict(HV.VARIANTS[variant], store_states=store_states))
    cc.weights = C.variant_weights(variant, k, ssf)
    gl = variant != "pose" if general_loop is None else general_loop
    out, wts, _ = cc.build(h2_init=_cuda(O0), h1_init=_cuda(I0) if gl else None, compute_dtype=dtype,
                           general_loop=gl, nhwc_loop=nhwc_loop, **conv)
    return out.cpu().numpy(), wts


def _fft(*a, **kw):
    return _build(*a, nhwc_conv='fft', **kw)


@pytest.mark.parametrize("c", F.CASES, ids=F.case_id)
def test_parity(c):
    """O_T (and the final I where the entry point returns it) against the float64 oracle"""
    ref_O, ref_I, _, _ = C.oracle(*F.shape_of(c), c.variant)
    e = C.e32(*F.shape_of(c), c.variant)
    O, wts = _fft(*F.shape_of(c), c.variant, nhwc_loop=c.nhwc_loop)
    assert O.shape == (c.n, c.h, c.w, c.k)
    S.check(f"{F.case_id(c)} O_T", O, ref_O, c.ssf, F.DTYPE, e["O"])
    if 'I' in wts:
        S.check(f"{F.case_id(c)} I_T", wts['I'].cpu().numpy(), ref_I, c.ssf, F.DTYPE, e["I"])
    else:
        assert c.variant == "pose"


@pytest.mark.parametrize("variant", F.STATES_VARIANTS)
def test_store_states(variant):
    """every step's O_t and I_t; the last stack entry is the plain call's output bit for bit"""
    k, n, h, w, ssf = F.STATES
    _, _, ref_so, ref_si = C.oracle(k, n, h, w, ssf, variant)
    e = C.e32(k, n, h, w, ssf, variant)
    sO, wts = _fft(k, n, h, w, ssf, variant, store_states=True)
    sI = wts['store_I'].cpu().numpy()
    assert sO.shape == sI.shape == (n, F.T, h, w, k)
    for t in range(F.T):
        S.check(f"{variant} O_{t + 1}", sO[:, t], ref_so[t], ssf, F.DTYPE, e["O_t"][t])
        S.check(f"{variant} I_{t + 1}", sI[:, t], ref_si[t], ssf, F.DTYPE, e["I_t"][t])
    plain, _ = _fft(k, n, h, w, ssf, variant)
    assert np.array_equal(sO[:, -1], plain)


def test_batch_invariance_and_determinism():
    """9 x 32, ssf 5, k = 8 at n = 1, 3 and 66: image 0's bytes are the same at every n, n = 3 is the first
    three images of n = 66, images 31, 32 and 65 are within the bounds, a repeated run is bit-identical"""
    k, h, w, ssf, variant = F.BATCH
    N = max(F.BATCH_NS)
    ref = C.oracle(k, N, h, w, ssf, variant)[0]
    r32 = C.oracle(k, N, h, w, ssf, variant, "float32")[0]
    outs = {n: _fft(k, N, h, w, ssf, variant, images=slice(0, n))[0] for n in F.BATCH_NS}
    for n in F.BATCH_NS:
        assert outs[n].shape[0] == n and np.array_equal(outs[n][0], outs[1][0]), n
    assert np.array_equal(outs[3], outs[N][:3])
    for i in (0, 31, 32, 65):
        S.check(f"n={N} image {i}", outs[N][i:i + 1], ref[i:i + 1], ssf, F.DTYPE,
                S.metrics(r32[i:i + 1], ref[i:i + 1], ssf))
    S.check(f"n={N}", outs[N], ref, ssf, F.DTYPE, S.metrics(r32, ref, ssf))
    again = _fft(k, N, h, w, ssf, variant)[0]
    assert np.array_equal(again, outs[N])


def _context(wts, dtype=F.DTYPE, nhwc_loop=False, conv=None):
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
    ctx.circuit_fwd(x, o0, out, F.T, L.current_stream(x.device))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def test_chunked_conv_changes_no_bit():
    """k = 4, 2 x 3, ssf 3 at n = nhwc_fft_chunk + 3: the conv walks two chunks; image 0, the last image of
    chunk 0, the first of chunk 1 and the last image are each the same image run alone, bit for bit"""
    L = pkg()._lib
    k, h, w, ssf, variant = F.CHUNK
    wts = C.variant_weights(variant, k, ssf)
    ctx = _context(wts, conv=L.MP_CN_CONV_FFT)
    chunk = ctx.info("nhwc_fft_chunk")
    assert ctx.info("nhwc_conv") == 1 and chunk == F.chunk_images(k)
    n = chunk + F.CHUNK_EXTRA
    X, O0, _ = C.inputs(k, n, h, w)
    whole = _ctx_fwd(ctx, X, O0)
    for i in (0, chunk - 1, chunk, n - 1):
        one = _ctx_fwd(ctx, X[i:i + 1], O0[i:i + 1])
        assert np.array_equal(one[0], whole[i]), i
    ctx.close()
    ref = C.oracle(k, n, h, w, ssf, variant)[0]
    r32 = C.oracle(k, n, h, w, ssf, variant, "float32")[0]
    S.check(f"n={n} (chunk {chunk})", whole, ref, ssf, F.DTYPE, S.metrics(r32, ref, ssf))


def test_one_context_serves_maps_of_different_sizes():
    """(2,16,32) -> (1,7,9) -> (3,20,28) -> (2,16,32) on one k = 24 context: each output is a fresh
    context's bit for bit, the last equals the first"""
    L = pkg()._lib
    k, ssf = F.REUSE_K, F.REUSE_SSF
    wts = C.variant_weights("pose", k, ssf)
    ctx = _context(wts, conv=L.MP_CN_CONV_FFT)
    assert ctx.info("channels") == k and ctx.info("nhwc_loop") == 1 and ctx.info("nhwc_conv") == 1
    outs = []
    for n, h, w in F.REUSE_SEQUENCE:
        X, O0, _ = C.inputs(k, n, h, w)
        outs.append(_ctx_fwd(ctx, X, O0))
        fresh = _context(wts, conv=L.MP_CN_CONV_FFT)
        want = _ctx_fwd(fresh, X, O0)
        fresh.close()
        assert np.array_equal(outs[-1], want), (n, h, w)
        S.check(f"call {len(outs)} n{n} {h}x{w}", outs[-1], C.oracle(k, n, h, w, ssf, "pose")[0], ssf, F.DTYPE,
                C.e32(k, n, h, w, ssf, "pose")["O"])
    ctx.close()
    assert np.array_equal(outs[0], outs[-1])


def test_fft_against_direct():
    k, n, h, w, ssf, variant = F.AGAINST_DIRECT
    ref = C.oracle(k, n, h, w, ssf, variant)[0]
    e = C.e32(k, n, h, w, ssf, variant)["O"]
    fft, _ = _fft(k, n, h, w, ssf, variant)
    direct, _ = _build(k, n, h, w, ssf, variant, nhwc_conv='direct')
    S.check("fft conv O_T", fft, ref, ssf, F.DTYPE, e)
    S.check("direct conv O_T", direct, ref, ssf, F.DTYPE, e)
    print(f"fft vs direct conv: rel_inf {S.rel_inf(fft, direct):.3e}")


@pytest.mark.parametrize("variant", F.AGAINST_FFT64_VARIANTS)
def test_fft_against_the_64_channel_fft_path(variant):
    """k = 64: the new loop (nhwc_loop, nhwc_conv='fft') and the general loop's fp32_fft are each within the
    bounds; bit equality is not expected (other layouts, another K order)"""
    k, n, h, w, ssf = F.AGAINST_FFT64
    ref_O, ref_I, _, _ = C.oracle(k, n, h, w, ssf, variant)
    e = C.e32(k, n, h, w, ssf, variant)
    new, wn = _fft(k, n, h, w, ssf, variant, general_loop=True, nhwc_loop=True)
    old, wo = _build(k, n, h, w, ssf, variant, general_loop=True, dtype="fp32_fft")
    S.check(f"{variant} nhwc loop, fft conv O_T", new, ref_O, ssf, F.DTYPE, e["O"])
    S.check(f"{variant} nhwc loop, fft conv I_T", wn['I'].cpu().numpy(), ref_I, ssf, F.DTYPE, e["I"])
    S.check(f"{variant} general loop fp32_fft O_T", old, ref_O, ssf, "fp32_fft", e["O"])
    S.check(f"{variant} general loop fp32_fft I_T", wo['I'].cpu().numpy(), ref_I, ssf, "fp32_fft", e["I"])
    print(f"{variant} nhwc fft conv vs general loop fp32_fft: rel_inf {S.rel_inf(new, old):.3e}")


def test_default_is_unchanged():
    """nhwc_conv='direct', or no argument, is a context that never heard of the option, bit for bit"""
    L = pkg()._lib
    k, n, h, w, ssf, variant = F.AGAINST_DIRECT
    X, O0, _ = C.inputs(k, n, h, w)
    wts = C.variant_weights(variant, k, ssf)
    ctx = _context(wts)
    assert ctx.info("nhwc_conv") == 0
    never = _ctx_fwd(ctx, X, O0)
    ctx.close()
    ctx = _context(wts, conv=L.MP_CN_CONV_DIRECT)
    assert ctx.info("nhwc_conv") == 0
    assert np.array_equal(_ctx_fwd(ctx, X, O0), never)
    ctx.close()
    assert np.array_equal(_build(k, n, h, w, ssf, variant, nhwc_conv='direct')[0], never)
    assert np.array_equal(_build(k, n, h, w, ssf, variant)[0], never)
    fft = _fft(k, n, h, w, ssf, variant)[0]
    assert not np.array_equal(fft, never)                 # and the option is not a no-op


@pytest.mark.parametrize("what,k,dtype,nhwc_loop", [("k25", 25, "fp32_split", False), ("k8-fp32", 8, "fp32", False),
                                                    ("k64-off-the-loop", 64, "fp32_split", False)],
                         ids=lambda v: str(v))
def test_refused_at_finalize_before_any_launch(what, k, dtype, nhwc_loop):
    L = pkg()._lib
    ctx = L.Context(L.MP_MODEL_HGRU_CIRCUIT, 0)
    for nm, v in C.variant_weights("pose", k, 5).items():
        ctx.set_weight(nm, v)
    ctx.set_nhwc_conv(L.MP_CN_CONV_FFT)
    with pytest.raises(L.MonkeyPoseError) as e:
        ctx.finalize(L.dtype_code(dtype))
    assert e.value.code == MP_ERR_UNSUPPORTED, str(e.value)
    assert str(k) in str(e.value)
    if k == 64:
        assert "MP_DTYPE_F32_FFT" in str(e.value)
    x = torch.zeros((1, 4, 4, k), device="cuda")
    out = torch.full_like(x, 7.0)
    with pytest.raises(L.MonkeyPoseError) as e2:      # not finalized: no forward either
        ctx.circuit_fwd(x, x, out, F.T, L.current_stream(x.device))
    assert e2.value.code == MP_ERR_STATE
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    ctx.close()


@pytest.mark.parametrize("h,w", [(65, 8), (8, 65)])
def test_larger_map_is_refused_at_the_call_before_any_launch(h, w):
    L = pkg()._lib
    ctx = _context(C.variant_weights("pose", 8, 5), conv=L.MP_CN_CONV_FFT)
    x = torch.zeros((1, h, w, 8), device="cuda")
    out = torch.full_like(x, 7.0)
    with pytest.raises(L.MonkeyPoseError) as e:
        ctx.circuit_fwd(x, x, out, F.T, L.current_stream(x.device))
    assert e.value.code == MP_ERR_SHAPE and "64" in str(e.value)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    # the same context still serves a map it accepts, and the set call is refused once finalized
    X, O0, _ = C.inputs(8, 1, 9, 32)
    S.check("after the refusal", _ctx_fwd(ctx, X, O0), C.oracle(8, 1, 9, 32, 5, "pose")[0], 5, F.DTYPE,
            C.e32(8, 1, 9, 32, 5, "pose")["O"])
    assert ctx.lib.mp_circuit_set_nhwc_conv(ctx.h, L.MP_CN_CONV_DIRECT) == MP_ERR_STATE
    assert ctx.info("nhwc_conv") == 1
    ctx.close()
