"""CPU: what the GPU tests of the tiled FFT conv (tests/test_gpu_circuit_fft_tiled.py) rest on, from the case
table, the oracle, numpy and the library's host export alone: the table covers what it claims; the tile plan
of circuit_fft.hpp (mp_cn_fft_tiles_host) is the rule restated here in Python, partitions the axis and keeps every
read inside its window; the algorithm -- plan, zero-filled 64-windows padded to 72, rfft2, G of the weight
kernel's formula, irfft2, scatter of the owned rectangles -- is the oracle's SAME conv; the oracle's conv
inputs stay inside the per-window f16 range of the spectra; ``_lib.resolve_nhwc_conv`` makes the library's
refusals before a context exists."""
import numpy as np
import pytest

import circuit_channel_cases as C
import circuit_fft_cases as F
import circuit_fft_tiled_cases as FT
import hgru_variant_cases as HV
from helpers import pkg
from test_circuit_fft_cpu import N, spectral_weights

MP_ERR_ARG = -1


def test_case_table_is_well_formed_and_covers_its_claims():
    assert len({FT.case_id(c) for c in FT.CASES}) == len(FT.CASES)
    for c in FT.CASES:
        assert c.ssf in (3, 5, 15) and c.variant in HV.VARIANTS, c
        assert 4 <= c.k <= 256 and c.k % 4 == 0 and c.n >= 1, c
        assert c.h > 64 or c.w > 64, c                  # every case is tiled on some axis
        assert (c.k == 64) == c.nhwc_loop, c
        assert FT.seam_mask(c.h, c.w, c.ssf).any(), c
    ty = lambda c: len(FT.plan(c.h, c.ssf))
    tx = lambda c: len(FT.plan(c.w, c.ssf))
    assert any(ty(c) == 2 and tx(c) == 1 for c in FT.CASES) and any(ty(c) == 1 and tx(c) == 2 for c in FT.CASES)
    assert any(ty(c) == 2 and tx(c) == 2 and c.k == 4 for c in FT.CASES)
    # a last tile that owns one position; a middle tile; an axis that is an exact multiple of the step
    assert any(FT.plan(c.w, c.ssf)[-1][2] == 1 and tx(c) == 3 and c.k % 8 == 4 for c in FT.CASES)
    assert any(tx(c) == 3 and c.n == 3 and c.ssf == 15 for c in FT.CASES)
    assert any(c.h % (64 - 2 * (c.ssf // 2)) == 0 and c.h > 64 for c in FT.CASES)
    # a window that lies mostly beyond the map: the second tile of 65 rows at ssf 15 covers [43, 107)
    o, _, cnt = FT.plan(65, 15)[1]
    assert (o, cnt) == (43, 15) and o + 64 - 65 > 32
    assert {c.ssf for c in FT.CASES} == {3, 5, 15}
    assert any(c.k > 64 for c in FT.CASES) and any(c.nhwc_loop for c in FT.CASES)
    flags = [C.derived_flags(c.variant) for c in FT.CASES]
    assert any(f["gru_gates"] for f in flags) and any(f["out_gates"] for f in flags)
    assert {C.aux_of(c.variant)['recurrent_nl'] for c in FT.CASES} >= {"tanh", "relu"}
    # the batch and chunk tests are what their docstrings say
    k, h, w, ssf, _ = FT.BATCH
    # nine images are 36 tiles: the product (32 tiles a block) takes a second, partly filled block for image 8
    assert FT.tiles_per_image(h, w, ssf) == 4 and 3 * 4 < 32 < max(FT.BATCH_NS) * 4 < 64
    k, h, w, ssf, _ = FT.CHUNK
    tpi = FT.tiles_per_image(h, w, ssf)
    assert tpi == 5 and F.chunk_images(k) == 96
    assert 19 * tpi < 96 < 20 * tpi == FT.CHUNK_N * tpi and 96 - 19 * tpi == 1      # after tile 0 of image 19
    assert all(h <= 64 and w <= 64 for _, _, h, w, _, _ in FT.SMALL)
    assert FT.REUSE_SEQUENCE[0] == FT.REUSE_SEQUENCE[-1]
    assert {h > 64 or w > 64 for _, h, w in FT.REUSE_SEQUENCE} == {True, False}


@pytest.mark.parametrize("ssf", [3, 5, 15])
def test_tile_plan_of_the_library_is_the_stated_rule(ssf):
    L_ = pkg()._lib
    r = ssf // 2
    assert 64 - 2 * r == {3: 62, 5: 60, 15: 50}[ssf]
    for L in range(1, FT.PLAN_MAX_L + 1):
        got = L_.cn_fft_tiles_host(L, ssf)
        assert got == FT.plan(L, ssf), (L, ssf)
        if L <= 64:
            assert got == [(0, 0, L)]                   # the single 'fft' tile
        else:
            assert len(got) == -(-L // (64 - 2 * r))
        owned = []
        for origin, out0, count in got:
            assert count >= 1 and 0 <= out0 and out0 + count <= 64
            assert origin + 64 > 0 and origin < L       # the window (64 long) meets the map
            for pos in range(origin + out0, origin + out0 + count):
                for q in range(pos - r, pos + r + 1):   # every read of the output
                    local = q - origin
                    if 0 <= q < L:
                        assert 0 <= local < 64, (L, ssf, pos, q)        # a map position: inside the window
                    else:
                        # a zero: inside the window's zero fill, or (one tile) in the 72-point pad, which
                        # the circular index reaches from either side without meeting the map's L <= 64
                        assert 0 <= local % 72 < 64 and len(got) > 1 or (len(got) == 1 and L <= local % 72 < 72), (L, q)
            owned += list(range(origin + out0, origin + out0 + count))
        assert owned == list(range(L)), (L, ssf)        # the outputs partition [0, L)


def test_tile_plan_export_refuses_bad_arguments():
    L_ = pkg()._lib
    lib = L_.load()
    import ctypes
    a = [np.zeros(8, np.int32) for _ in range(3)]
    p = [x.ctypes.data_as(ctypes.c_void_p) for x in a]
    assert lib.mp_cn_fft_tiles_host(130, 15, 8, *p) == 3
    assert [int(v) for v in a[0][:3]] == [-7, 43, 93] and [int(v) for v in a[2][:3]] == [50, 50, 30]
    assert lib.mp_cn_fft_tiles_host(130, 15, 2, *p) == MP_ERR_ARG       # cap too small
    assert lib.mp_cn_fft_tiles_host(130, 7, 8, *p) == MP_ERR_ARG        # no such filter size
    assert lib.mp_cn_fft_tiles_host(0, 15, 8, *p) == MP_ERR_ARG
    assert lib.mp_cn_fft_tiles_host(10, 15, 8, None, p[1], p[2]) == MP_ERR_ARG
    with pytest.raises(L_.MonkeyPoseError):
        L_.cn_fft_tiles_host(130, 15, cap=2)


def tiled_fft_conv(a, w):
    """the algorithm: per tile of the plan a zero-filled 64 x 64 window of the map, zero-padded to 72 x 72,
    rfft2, times G, irfft2 (unnormalised: 1 / 72^2 is in G); the rectangle the tile owns goes to the output"""
    n, h, wd, k = a.shape
    ssf = w.shape[0]
    G = spectral_weights(w)
    out = np.full((n, h, wd, w.shape[3]), np.nan)
    for oy, ly, cy in FT.plan(h, ssf):
        for ox, lx, cx in FT.plan(wd, ssf):
            pad = np.zeros((n, N, N, k))
            y0, y1, x0, x1 = max(oy, 0), min(oy + 64, h), max(ox, 0), min(ox + 64, wd)
            pad[:, y0 - oy:y1 - oy, x0 - ox:x1 - ox] = a[:, y0:y1, x0:x1]
            y = np.einsum("nyxi,yxio->nyxo", np.fft.rfft2(pad, axes=(1, 2)), G)
            p = np.fft.irfft2(y, s=(N, N), axes=(1, 2)) * (N * N)
            out[:, oy + ly:oy + ly + cy, ox + lx:ox + lx + cx] = p[:, ly:ly + cy, lx:lx + cx]
    return out


MODEL_SHAPES = sorted({(c.h, c.w, c.ssf) for c in FT.CASES} | set(FT.MODEL_EXTRA_SHAPES))


@pytest.mark.parametrize("h,w,ssf", MODEL_SHAPES, ids=lambda v: str(v))
def test_numpy_model_of_the_algorithm_is_the_oracles_same_conv(h, w, ssf):
    from oracle import hgru_ref as R
    k = 4
    a = C.inputs(k, 1, h, w)[0].astype(np.float64)
    p_r = C.weights(k, ssf)[f"{C.SCOPE}/p_r"].astype(np.float64)
    want = R.conv2d_same(a, p_r)
    got = tiled_fft_conv(a, p_r)
    assert np.isfinite(got).all()                       # every pixel is owned by a tile
    err = np.abs(got - want).max() / np.abs(want).max()
    print(f"{h}x{w} ssf {ssf}: tiled fft model vs SAME conv rel_inf {err:.2e}")
    assert err <= 1e-12


@pytest.mark.parametrize("c", FT.CASES, ids=FT.case_id)
def test_oracle_conv_inputs_stay_inside_the_f16_range_of_the_spectra(c):
    """|S| <= SPEC_SCALE * sum|v| over a window <= min(h, 64) * min(w, 64) * max|v| / 64 for every conv input
    of every step (O_{t-1} or A_in = O_{t-1} g1, I_t or B_in = I_t g2), on the float64 oracle alone"""
    from oracle import hgru_ref as R
    aux = C.aux_of(c.variant)
    wts = C.weights(c.k, c.ssf)
    _, O0, _ = C.inputs(c.k, c.n, c.h, c.w)
    _, _, so, si = C.oracle(*FT.shape_of(c), c.variant)
    i_r, o_r = (wts[f"{C.SCOPE}/{n}"].astype(np.float64) for n in ("i_r", "o_r"))
    i_b, o_b = (wts[f"{C.SCOPE}/{n}"].astype(np.float64).reshape(-1) for n in ("i_b", "o_b"))
    worst = 0.0
    for t in range(FT.T):
        O = O0.astype(np.float64) if t == 0 else so[t - 1]
        a_in = O * R.sigmoid(R.conv2d_same(O, i_r) + i_b) if aux['gru_gates'] else O
        b_in = si[t] * R.sigmoid(R.conv2d_same(si[t], o_r) + o_b) if aux['output_gru_gates'] else si[t]
        worst = max(worst, *(float(np.abs(v).max()) for v in (O, a_in, si[t], b_in)))
    bound = min(c.h, 64) * min(c.w, 64) * worst * F.SPEC_SCALE
    print(f"{FT.case_id(c)}: max|conv input| {worst:.3f}, min(h, 64) min(w, 64) max|v| / 64 = {bound:.1f}")
    assert bound <= F.F16_RANGE_BOUND


def test_helper_refuses_before_a_context_exists():
    L = pkg()._lib
    R = L.resolve_nhwc_conv
    assert L.NHWC_CONVS['fft_tiled'] == L.MP_CN_CONV_FFT_TILED == 2
    for h, w in ((65, 32), (32, 65), (300, 200)):
        assert R('fft_tiled', 'fp32_split', h, w, 8) == 2
        assert R('fft_tiled', 'auto', h, w, 8) == 2     # 'auto' means 'fp32_split' on this loop
    assert R('fft_tiled', 'fp32_split', 16, 32, 8) == 2 and R('fft_tiled', 'fp32_split', 70, 20, 64, nhwc_loop=True) == 2
    with pytest.raises(ValueError, match="25"):
        R('fft_tiled', 'fp32_split', 65, 32, 25)
    for dtype in ('fp32', 'bf16', 'fp32_fft'):
        with pytest.raises(ValueError, match="8"):
            R('fft_tiled', dtype, 65, 32, 8)
    with pytest.raises(ValueError, match="fp32_fft"):            # 64 channels off the loop
        R('fft_tiled', 'fp32_split', 65, 32, 64)
    with pytest.raises(ValueError, match="65 x 32"):             # 'fft' is as it was
        R('fft', 'fp32_split', 65, 32, 8)
    # 'auto' never names an FFT conv
    assert L.resolve_dtype('auto', 128, 128, 8) == 'fp32_split'
    assert "mp_cn_fft_tiles_host" in L._SIGS
