"""CPU: what the GPU tests of the channel-general loop's FFT conv (tests/test_gpu_circuit_fft.py) rest on,
from the case table, the oracle and numpy alone: the table covers what it claims; the algorithm -- zero-pad
to 72 x 72, rfft2, multiply by G built from the weight kernel's formula, irfft2, crop -- is the oracle's
SAME conv (the index formula, and the claim that 72 points are enough for a 64-wide map); the oracle's conv
inputs stay inside the f16 range of the spectra; ``_lib.resolve_nhwc_conv`` makes the library's refusals
before a context exists."""
import numpy as np
import pytest

import circuit_channel_cases as C
import circuit_fft_cases as F
import circuit_shape_cases as S
import hgru_variant_cases as HV
from helpers import pkg

N = 72


def test_case_table_is_well_formed_and_covers_its_claims():
    assert len({F.case_id(c) for c in F.CASES}) == len(F.CASES)
    for c in F.CASES:
        assert c.ssf in (3, 5, 15) and c.variant in HV.VARIANTS, c
        assert 4 <= c.k <= 256 and c.k % 4 == 0 and c.n >= 1, c
        assert 1 <= c.h <= 64 and 1 <= c.w <= 64, c
        assert (c.k == 64) == c.nhwc_loop, c            # 64 channels reach the loop by the flag only
    ks = {c.k for c in F.CASES}
    assert any(k % 8 == 4 for k in ks)                  # a zero half K step
    assert any((2 * k) % 32 != 0 and k % 8 == 0 for k in ks)        # spare M rows alone
    assert any(k > 64 for k in ks) and min(ks) == 4 and max(ks) == 256
    assert any((c.h, c.w) == (64, 64) and c.ssf == 15 for c in F.CASES)     # 64 + 7 = 71 <= 72
    assert any(c.w not in (32, 64) for c in F.CASES)
    assert any(c.h < c.ssf and c.w < c.ssf for c in F.CASES)
    assert {c.ssf for c in F.CASES} == {3, 5, 15}
    assert any(c.n == 3 for c in F.CASES)
    flags = [C.derived_flags(c.variant) for c in F.CASES]
    assert any(f["gru_gates"] for f in flags) and any(f["out_gates"] for f in flags)        # gated A_in, B_in
    assert {C.aux_of(c.variant)['recurrent_nl'] for c in F.CASES} >= {"tanh", "relu"}
    c64 = [c for c in F.CASES if c.nhwc_loop]
    assert c64 and not any(S.map_ok(d, c64[0].h, c64[0].w) for d in ("fp32", "fp32_split", "fp32_fft"))
    # the chunking test's batch is small enough to run and the chunk rule gives what the issue states
    assert F.chunk_images(4) == 6272 and F.chunk_images(256) == 96 and F.chunk_images(64) == 384
    assert all(F.chunk_images(k) % 32 == 0 and F.chunk_images(k) >= 32 for k in range(4, 257, 4))
    assert all(2 * F.chunk_images(k) * (k // 4) * 2664 * 32 <= 1 << 30 for k in range(4, 257, 4))
    assert F.REUSE_SEQUENCE[0] == F.REUSE_SEQUENCE[-1]


def spectral_weights(w):
    """G[fy, fx, ci, co] of k_circuit_fft.hip cn_spec_weights_kernel, in float64:
    sum_taps w[ky, kx, ci, co] exp(-2 pi i (fy (R - ky) + fx (R - kx)) / 72) / 72^2"""
    ks = w.shape[0]
    r = ks // 2
    fy = np.arange(N)[:, None]
    fx = np.arange(N // 2 + 1)[:, None]
    ey = np.exp(-2j * np.pi * ((fy * (r - np.arange(ks)[None, :])) % N) / N)       # [fy, ky]
    ex = np.exp(-2j * np.pi * ((fx * (r - np.arange(ks)[None, :])) % N) / N)       # [fx, kx]
    return np.einsum("ya,xb,abio->yxio", ey, ex, w.astype(np.float64)) / (N * N)


def fft_conv(a, w):
    """the algorithm: zero-pad to 72 x 72, rfft2, multiply by G, irfft2 (unnormalised: 1 / 72^2 is in G), crop"""
    n, h, wd, k = a.shape
    pad = np.zeros((n, N, N, k))
    pad[:, :h, :wd] = a
    s = np.fft.rfft2(pad, axes=(1, 2))
    y = np.einsum("nyxi,yxio->nyxo", s, spectral_weights(w))
    return (np.fft.irfft2(y, s=(N, N), axes=(1, 2)) * (N * N))[:, :h, :wd]


SHAPES = sorted({(c.h, c.w, c.ssf) for c in F.CASES} | {(64, 64, 3), (64, 64, 5), (1, 64, 15), (64, 1, 15)})


@pytest.mark.parametrize("h,w,ssf", SHAPES, ids=lambda v: str(v))
def test_numpy_model_of_the_algorithm_is_the_oracles_same_conv(h, w, ssf):
    from oracle import hgru_ref as R
    k = 4
    a = C.inputs(k, 2, h, w)[0].astype(np.float64)
    p_r = C.weights(k, ssf)[f"{C.SCOPE}/p_r"].astype(np.float64)
    want = R.conv2d_same(a, p_r)
    got = fft_conv(a, p_r)
    err = np.abs(got - want).max() / np.abs(want).max()
    print(f"{h}x{w} ssf {ssf}: fft model vs SAME conv rel_inf {err:.2e}")
    assert err <= 1e-12


def test_numpy_model_at_a_wider_k():
    from oracle import hgru_ref as R
    a = C.inputs(28, 2, 7, 9)[0].astype(np.float64)
    p_r = C.weights(28, 15)[f"{C.SCOPE}/p_r"].astype(np.float64)
    want = R.conv2d_same(a, p_r)
    assert np.abs(fft_conv(a, p_r) - want).max() <= 1e-12 * np.abs(want).max()


@pytest.mark.parametrize("c", F.CASES, ids=F.case_id)
def test_oracle_conv_inputs_stay_inside_the_f16_range_of_the_spectra(c):
    """|S| <= SPEC_SCALE * sum|v| <= h * w * max|v| / 64 for every conv input of every step (O_{t-1} or
    A_in = O_{t-1} g1, I_t or B_in = I_t g2), on the float64 oracle alone"""
    from oracle import hgru_ref as R
    aux = C.aux_of(c.variant)
    wts = C.weights(c.k, c.ssf)
    _, O0, _ = C.inputs(c.k, c.n, c.h, c.w)
    _, _, so, si = C.oracle(*F.shape_of(c), c.variant)
    i_r, o_r = (wts[f"{C.SCOPE}/{n}"].astype(np.float64) for n in ("i_r", "o_r"))
    i_b, o_b = (wts[f"{C.SCOPE}/{n}"].astype(np.float64).reshape(-1) for n in ("i_b", "o_b"))
    worst = 0.0
    for t in range(F.T):
        O = O0.astype(np.float64) if t == 0 else so[t - 1]
        a_in = O * R.sigmoid(R.conv2d_same(O, i_r) + i_b) if aux['gru_gates'] else O
        b_in = si[t] * R.sigmoid(R.conv2d_same(si[t], o_r) + o_b) if aux['output_gru_gates'] else si[t]
        worst = max(worst, *(float(np.abs(v).max()) for v in (O, a_in, si[t], b_in)))
    bound = c.h * c.w * worst * F.SPEC_SCALE
    print(f"{F.case_id(c)}: max|conv input| {worst:.3f}, h w max|v| / 64 = {bound:.1f}")
    assert bound <= F.F16_RANGE_BOUND


def test_helper_refuses_before_a_context_exists():
    L = pkg()._lib
    R = L.resolve_nhwc_conv
    assert R('direct', 'auto', 200, 300, 25) == L.MP_CN_CONV_DIRECT == 0          # the default: anything goes
    assert R('direct', 'fp32_fft', 64, 64, 64) == 0
    assert R('fft', 'auto', 64, 64, 8) == L.MP_CN_CONV_FFT == 1
    assert R('fft', 'fp32_split', 1, 1, 256) == 1 and R('fft', 'fp32_split', 20, 28, 64, nhwc_loop=True) == 1
    with pytest.raises(ValueError, match="25"):
        R('fft', 'fp32_split', 7, 9, 25)
    for dtype in ('fp32', 'bf16', 'fp32_fft'):
        with pytest.raises(ValueError, match="8"):
            R('fft', dtype, 16, 32, 8)
    with pytest.raises(ValueError, match="fp32_fft"):            # 64 channels have their own FFT path
        R('fft', 'fp32_split', 16, 32, 64)
    with pytest.raises(ValueError, match="65 x 32"):
        R('fft', 'fp32_split', 65, 32, 8)
    with pytest.raises(ValueError, match="32 x 65"):
        R('fft', 'fp32_split', 32, 65, 8)
    with pytest.raises(ValueError, match="winograd"):
        R('winograd', 'fp32_split', 16, 32, 8)
    # 'auto' stays 'fp32_split' on this loop and never names the FFT conv
    for k in (4, 8, 128):
        assert L.resolve_dtype('auto', 64, 64, k) == 'fp32_split'
    assert L.resolve_dtype('auto', 20, 28, 64, nhwc_loop=True) == 'fp32_split'
    assert "mp_circuit_set_nhwc_conv" in L._SIGS
