"""CPU: the conditions the GPU shape tests (tests/test_gpu_circuit_shapes.py) rest on, from the case
table and the oracle alone: every case's shape is one its path accepts, 'auto' sends the FFT shapes
to the FFT path, the oracle is finite and per-image independent, every error region is non-empty and
carries values of the map's scale, the float32 oracle's own error leaves the 1e-5 floor as the
operative fp32-class bound, and the inputs are sensitive enough that a kernel which miscounts live
rows or drops a filter tap cannot pass."""
import numpy as np
import pytest

import circuit_shape_cases as C
from helpers import pkg, rel_inf

SHAPES = sorted({(c.n, c.h, c.w, c.ssf, c.variant if c.variant != "pose" else None) for c in C.ALL_CASES},
                key=lambda s: (s[:4], s[4] or ""))
FFT_SHAPES = sorted({(c.h, c.w) for c in C.ALL_CASES if c.dtype in ("fp32_fft", "bf16")})
ODD_FFT = [c for c in C.FFT_FUSED if c.h % 8]
TAP_CASES = [c for c in C.FFT_FUSED + C.DIRECT if c.ssf in (3, 15) and c.h >= 16]


def _id(s):
    return f"n{s[0]}-{s[1]}x{s[2]}-ssf{s[3]}" + (f"-{s[4]}" if s[4] else "")


def test_every_case_fits_its_path():
    for c in C.ALL_CASES:
        assert C.map_ok(c.dtype, c.h, c.w), c
        assert c.ssf in (3, 5, 15) and c.n >= 1
    for dtype, h, w in C.REJECTED:
        assert not C.map_ok(dtype, h, w), (dtype, h, w)
    assert {c.ssf for c in C.FFT_FUSED} == {3, 5, 15}
    assert {c.ssf for c in C.DIRECT if c.dtype == "fp32"} == {3, 5, 15}
    assert {c.ssf for c in C.DIRECT if c.dtype == "fp32_split"} == {3, 5, 15}
    assert any(c.w > 64 for c in C.DIRECT)
    assert C.REUSE_SEQUENCE[0] == C.REUSE_SEQUENCE[-1] and len(set(C.REUSE_SEQUENCE)) >= 4


def test_auto_sends_fft_shapes_to_the_fft_path():
    L = pkg()._lib
    for h, w in FFT_SHAPES + [C.DEFAULT_DTYPE_SHAPE[1:3]]:
        assert L.resolve_dtype('auto', h, w) == 'fp32_fft', (h, w)
        assert L.resolve_dtype('bf16', h, w) == 'bf16'
    for dtype, h, w in C.REJECTED:
        if dtype == "bf16":
            with pytest.raises(ValueError):
                L.resolve_dtype('bf16', h, w)
    for c in C.DIRECT:    # 'auto' agrees with the restated rule outside the FFT shapes too
        want = 'fp32_fft' if C.map_ok('fp32_fft', c.h, c.w) else ('fp32_split' if C.map_ok('fp32_split', c.h, c.w) else 'fp32')
        assert L.resolve_dtype('auto', c.h, c.w) == want, c
    for h in range(1, 130):   # the restated rule against resolve_dtype on a grid
        for w in (16, 32, 48, 64, 96, 128):
            got = L.resolve_dtype('auto', h, w)
            assert C.map_ok(got, h, w) or got == 'fp32', (h, w, got)
            assert (got == 'fp32_fft') == C.map_ok('fp32_fft', h, w)


def test_batch_slices_are_the_dispatch_the_cases_name():
    """mp_abi.hip run_circuit: two streams from 64 images on, slices of whole 32-image groups, the
    first slice the larger half -- 66 = 64 + 2 and 258 = 160 + 98"""
    assert [C.first_slice(n) for n in C.BATCH_NS] == [1, 9, 40, 64, 160]
    assert C.sampled_images(258) == [0, 159, 160, 257] and C.sampled_images(66) == [0, 63, 64, 65]
    assert C.sampled_images(1) == [0] and C.sampled_images(9) == [0, 8]


@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_oracle_is_finite_and_regions_carry_the_maps_scale(shape):
    n, h, w, ssf, variant = shape
    O, so, si = C.oracle(n, h, w, ssf, variant)
    reg = C.regions(h, w, ssf)
    for what, a in [("O_T", O)] + [(f"O_{t + 1}", a) for t, a in enumerate(so)] + [(f"I_{t + 1}", a) for t, a in enumerate(si)]:
        assert a.dtype == np.float64 and a.shape == (n, h, w, 64)
        assert np.isfinite(a).all(), what
        top = np.abs(a).max()
        assert top > 1e-2, what
        for k in C.METRICS:
            assert reg[k].any(), (what, k)
            assert np.abs(a[:, reg[k]]).max() >= 0.5 * top, (what, k)
    assert reg["border"][0].all() and reg["border"][:, 0].all() and reg["last"][h - 1].all() and reg["last"][:, w - 1].all()
    if h > 2 * (ssf // 2) + 1:
        assert not reg["border"].all() and not reg["last"].all()


@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_float32_oracle_error_leaves_the_floor_operative(shape):
    n, h, w, ssf, variant = shape
    e = C.e32(n, h, w, ssf, variant)
    rows = [e["O"], e["I"], *e["O_t"], *e["I_t"]]
    print(f"e32 {_id(shape)}: O_T " + " ".join(f"{v:.2e}" for v in e["O"]) + f"  max {max(max(r) for r in rows):.2e}")
    for r in rows:
        for v in r:
            assert 0 < v <= 1e-6, (shape, v)
            assert C.fp32_class_bound(v) == C.FP32_CLASS_FLOOR


@pytest.mark.parametrize("hidden_init", ["zeros", "identity"])
def test_hidden_init_oracles(hidden_init):
    c = C.STATES
    O, so, si = C.oracle(c.n, c.h, c.w, c.ssf, None, "float64", hidden_init)
    given = C.oracle(c.n, c.h, c.w, c.ssf)[0]
    assert np.isfinite(O).all() and rel_inf(O, given) >= 1e-2       # the initial state reaches O_T
    e = C.e32(c.n, c.h, c.w, c.ssf, None, hidden_init)
    assert max(max(r) for r in [e["O"], *e["O_t"], *e["I_t"]]) <= 1e-6


def test_oracle_is_per_image_independent():
    """a slice of a batch equals its solo run exactly: the batch cases take the first n images of one
    input set, and compare single images of a batch with their own n = 1 run"""
    from oracle import hgru_ref as R
    h, w, ssf = C.BATCH_SHAPE
    wts, X, O0, _ = C.inputs(C.BATCH_MAX, h, w, ssf)
    full = C.oracle(C.BATCH_MAX, h, w, ssf)[0]
    for i in C.sampled_images(C.BATCH_MAX):
        solo = R.hgru_forward(X[i:i + 1].astype(np.float64), O0[i:i + 1], wts, C.T)
        assert np.array_equal(solo[0], full[i]), i
    part = R.hgru_forward(X[:40].astype(np.float64), O0[:40], wts, C.T)
    assert np.array_equal(part, full[:40])
    c = C.GENERAL[-1]     # the variant oracle too
    assert c.variant == "defaults"
    wts, X, O0, I0 = C.inputs(c.n, c.h, c.w, c.ssf)
    import hgru_variants_ref as V
    solo = V.variant_forward(X[1:2].astype(np.float64), O0[1:2].astype(np.float64), I0[1:2].astype(np.float64),
                             {k: v.astype(np.float64) for k, v in wts.items()}, V.full_aux(C.aux_of("defaults")),
                             C.T, scope=C.SCOPE)
    assert np.array_equal(solo[0][0], C.oracle(c.n, c.h, c.w, c.ssf, "defaults")[0][1])


def test_defaults_variant_reads_i0_and_differs_from_pose():
    c = C.GENERAL[-1]
    O, _, si = C.oracle(c.n, c.h, c.w, c.ssf, "defaults")
    assert rel_inf(O, C.oracle(c.n, c.h, c.w, c.ssf)[0]) >= 1e-2
    import hgru_variants_ref as V
    wts, X, O0, I0 = C.inputs(c.n, c.h, c.w, c.ssf)
    w64 = {k: v.astype(np.float64) for k, v in wts.items()}
    other = V.variant_forward(X.astype(np.float64), O0.astype(np.float64), -I0.astype(np.float64), w64,
                              V.full_aux(C.aux_of("defaults")), C.T, scope=C.SCOPE)
    assert rel_inf(other[0], O) >= 1e-2


@pytest.mark.parametrize("c", ODD_FFT, ids=C.case_id)
def test_one_extra_live_row_moves_the_last_row(c):
    """the oracle on the map with one more bottom row (a copy of the last) differs from the true
    result by >= 1e-2 on the last-row metric: a kernel that treats a dead row as live cannot pass"""
    from oracle import hgru_ref as R
    wts, X, O0, _ = C.inputs(c.n, c.h, c.w, c.ssf)
    ext = lambda a: np.concatenate([a, a[:, -1:]], axis=1)
    more = R.hgru_forward(ext(X).astype(np.float64), ext(O0), wts, C.T)[:, :c.h]
    errs = C.metrics(more, C.oracle(c.n, c.h, c.w, c.ssf)[0], c.ssf)
    print(f"{C.case_id(c)}: one extra row moves " + " ".join(f"{e:.2e}" for e in errs))
    assert errs[2] >= 1e-2 and errs[1] >= 1e-2
    less = np.array(C.oracle(c.n, c.h, c.w, c.ssf)[0])     # and a dropped last row: zeros there
    less[:, -1] = 0
    assert C.metrics(less, C.oracle(c.n, c.h, c.w, c.ssf)[0], c.ssf)[2] >= 0.5


def test_odd_heights_cover_the_row_classes():
    hs = {c.h for c in ODD_FFT}
    assert {1, 7, 9, 17, 33, 63} <= hs
    assert {c.w for c in ODD_FFT} == {32, 64}


@pytest.mark.parametrize("c", TAP_CASES, ids=C.case_id)
def test_one_filter_tap_moves_the_result(c):
    """zeroing tap (0, 0) of p_r moves O_T by >= 1e-3: the 3- and 15-tap weight builds
    (build_spec_weights, pack_x3, launch_pack_conv64) cannot lose a tap unseen"""
    from oracle import hgru_ref as R
    wts, X, O0, _ = C.inputs(c.n, c.h, c.w, c.ssf)
    w2 = dict(wts)
    p = np.array(wts[f"{C.SCOPE}/p_r"])
    p[0, 0] = 0
    w2[f"{C.SCOPE}/p_r"] = p
    moved = R.hgru_forward(X.astype(np.float64), O0, w2, C.T)
    err = rel_inf(moved, C.oracle(c.n, c.h, c.w, c.ssf)[0])
    print(f"{C.case_id(c)}: p_r[0, 0] = 0 moves O_T by {err:.2e}")
    assert err >= 1e-3


def test_metrics_see_an_error_confined_to_the_last_row():
    """an error of 1e-5 of max|O| in the last live row only: inside the whole-map gate, outside the
    fp32-class bound on every metric that holds the row"""
    c = C.STATES
    ref = C.oracle(c.n, c.h, c.w, c.ssf)[0]
    bad = np.array(ref)
    bad[:, -1] += 2e-5 * np.abs(ref).max()
    errs = C.metrics(bad, ref, c.ssf)
    assert all(1e-5 < e <= 1e-4 for e in errs)
    with pytest.raises(AssertionError):
        C.check("last row off", bad, ref, c.ssf, c.dtype, C.e32(c.n, c.h, c.w, c.ssf)["O"])
    C.check("last row off (bf16 gate)", bad, ref, c.ssf, "bf16")
    inner = np.array(ref)
    inner[:, c.h // 2, c.w // 2] += 2e-5 * np.abs(ref).max()
    w_, b_, l_ = C.metrics(inner, ref, c.ssf)
    assert w_ > 1e-5 and b_ == 0 and l_ == 0
