"""The tables, inputs, references and gates of tests/attn_layer_cases.py checked without a GPU, so that no
gate of tests/test_gpu_attn_layers.py can pass vacuously.  On the float64 oracle
(oracle.regressors_ref.attn_forward with the case weights, two frames) the input conditions hold -- enough
positive pre-activations, BN(max) != max(BN) on the negative-gamma channels, every pool window position
wins somewhere -- float32 numpy of every layer passes its gates, and each planted fault exceeds its gate:
zero padding at every R-row tile seam of aconv_2 / 3 / 4, the BN applied before the max (and a fold that
loses gamma's sign), a dropped hi*lo plane in every layer the lost-plane gate covers, and the second image
of a shared 128-pixel tile of aconv_5 replaced by the first."""
import numpy as np
import pytest

import attn_layer_cases as A
import pose_layer_cases as P
from graph_op_cases import U, pool_windows, pool_winners, ratio
from oracle import regressors_ref as RR
from oracle.hgru_ref import conv2d_same, max_pool_same

N_CPU = 2        # two frames: one 128-pixel tile of aconv_5
KINDS = ("fp32_split", "fp32", "bf16")


@pytest.fixture(scope="module")
def oracle():
    """the float64 oracle's layer inputs as float32 (what the GPU taps hold) and its output"""
    wts = A.attn_weights()
    out, t = RR.attn_forward(A.attn_frames(N_CPU), wts, keep=True)
    x = {"aconv_1": t["resized"]}
    for i in range(1, 5):
        x[f"aconv_{i + 1}"] = t[f"aconv_{i}"].astype(np.float32)
    x["afc_1"] = t["aconv_5"].reshape(N_CPU, -1).astype(np.float32)
    return dict(wts=wts, x=x, out=out, relu1=t["relu1"], taps=t)


def test_tables_follow_the_issue():
    assert A.BATCHES == (1, 3, 11, 130) and A.DTYPES == ("fp32_split", "fp32", "bf16")
    assert A.REF_IMAGES == {1: (0,), 3: (0, 1, 2), 11: (0, 5, 10), 130: (0, 63, 64, 127, 128, 129)}
    assert len(A.params()) == 12 and A.TAPS == A.pkg()._lib.ATTN_TAP_NAMES
    assert A.SWITCHES == ("MP_IGEMM_HALO_TALL=0", "MP_IGEMM_HALO=0", "MP_IGEMM_XCD=0")
    for scope, k, cin, cout, side in A.CONVS[1:]:
        # 128-pixel tiles: R rows of a W-wide map, or 128 / (H W) whole images (k_igemm.hip halo_geom)
        assert A.TALL_R.get(scope, 0) == (128 // side if side * side >= 128 else 0)
        assert (k * k * cin >= 1152) == (f"conv{scope[-1]}" in A.G2_LAYERS)
    e = A.expected_paths("fp32_split")
    assert all(e[s]["family"] == "halo" and e[s]["wr"] == 1 and e[s]["pool"] == 0 for s in A.TALL_R)
    assert e["aconv_5"] == dict(family="x3w", pool=0, splits=1)
    assert A.expected_paths("bf16") == e
    assert all(A.expected_paths("fp32")[s]["family"] == "f32_im2col" for s in ("aconv_2", "aconv_5"))
    assert A.expected_paths("fp32_split", "MP_IGEMM_HALO=0")["aconv_3"]["family"] == "x3w"
    assert A.expected_paths("fp32_split", "MP_IGEMM_HALO_TALL=0")["aconv_4"]["wr"] == 2
    assert A.expected_paths("fp32_split", "MP_IGEMM_XCD=0") == e
    # a row that runs another kernel than it names is reported
    wrong = {s: dict(family="x3w", pool=0, splits=1, wr=0, ch=0, ks=0, nb=0) for s in e}
    assert {m[0] for m in A.path_mismatches(wrong, "fp32_split")} == {"aconv_1", "aconv_2", "aconv_3", "aconv_4"}
    right = {s: dict(dict(wr=0, ch=0, ks=0, nb=0), **v) for s, v in e.items()}
    assert A.path_mismatches(right, "fp32_split") == []


def test_weights_and_frames_are_the_stated_draws():
    wts = A.attn_weights()
    base = A.pkg().weights.synth_weights(A.pkg().weights.attn_vars(), A.SEED)
    assert set(wts) == set(base)
    for k, v in wts.items():
        assert v.dtype == np.float32 and v.shape == base[k].shape
        if "batch_normalization" not in k:
            assert np.array_equal(v, base[k]), k
    for scope in RR.ATTN_BN:
        g, b, m, v = A.bn_raw(wts, scope)
        assert ((np.abs(g) >= 0.5) & (np.abs(g) <= 1.5)).all() and (g < 0).mean() >= 0.25 and (g > 0).mean() >= 0.5
        for a in (b, m):
            assert ((np.abs(a) >= 0.1) & (np.abs(a) <= 0.5)).all() and (a < 0).any() and (a > 0).any()
        assert ((v >= 0.25) & (v <= 4.0)).all()
    f = A.attn_frames(130)
    assert f.shape == (130, 128, 128, 1) and np.array_equal(A.attn_frames(3), f[:3])
    assert len({f[i].tobytes() for i in range(130)}) == 130
    assert A.big_frames().shape == (3, 424, 512, 1)


def test_oracle_meets_the_input_conditions(oracle):
    wts, x = oracle["wts"], oracle["x"]
    for i, (scope, _, _, cout, _) in enumerate(A.CONVS):
        w, b = wts[f"cnn/{scope}/{scope}_filters"], wts[f"cnn/{scope}/{scope}_biases"]
        pre = conv2d_same(x[scope].astype(np.float64), w.astype(np.float64)) + b
        pos = float((pre > 0).mean())
        win = pool_windows(np.maximum(pre, 0), -np.inf)
        neg = A.bn_raw(wts, RR.ATTN_BN[i])[0] < 0
        # s < 0: max(BN(.)) = BN(min(.)), which differs from BN(max(.)) wherever the window is not constant
        differ = float((win.max(3) != win.min(3))[..., neg].mean())
        winners = pool_winners(pre)
        print(f"{scope}: positive {pos:.3f}, BN(max) != max(BN) in {differ:.3f} of the negative-gamma windows, "
              f"winning window positions {winners}")
        assert pos >= 0.25, scope
        assert differ >= 0.5, scope
        assert len(winners) >= 2, scope
    ref = A.relu1_ref(x["afc_1"], wts, "fp32")
    assert (ref.pre > 0).mean() >= 0.25
    assert np.abs(ref.want - oracle["relu1"]).max() <= 1e-5 * np.abs(ref.want).max()
    assert np.abs(A.out_ref(ref.want.astype(np.float32), wts).want - oracle["out"]).max() <= 1e-5


def test_the_two_frames_stay_distinct_through_every_stage(oracle):
    """an image read from the wrong place must change the result by far more than any gate"""
    for k, a in oracle["taps"].items():
        d = float(np.sqrt(np.mean((a[0] - a[1]) ** 2) / np.mean(a.astype(np.float64) ** 2)))
        print(f"{k}: rms(image 0 - image 1) / rms {d:.3f}")
        assert d >= 0.25, k


def _f32_conv(x, wts, scope):
    y = conv2d_same(x, wts[f"cnn/{scope}/{scope}_filters"]) + wts[f"cnn/{scope}/{scope}_biases"]
    assert y.dtype == np.float32
    return np.maximum(y, 0)


def _f32_affine(m, wts, scope):
    s, t = A.bn_fold(wts, scope)
    y = m.astype(np.float32) * s.astype(np.float32) + t.astype(np.float32)
    assert y.dtype == np.float32
    return y


def test_float32_numpy_passes_the_element_gates(oracle):
    wts, x = oracle["wts"], oracle["x"]
    g = P.g1_ratio(_f32_affine(max_pool_same(_f32_conv(x["aconv_1"], wts, "aconv_1")), wts, RR.ATTN_BN[0]),
                   A.pool1_ref(x["aconv_1"], wts))
    print(f"pool1: float32 numpy err/bound {g:.4f}")
    assert g <= 1.0
    for i, (scope, _, _, _, _) in enumerate(A.CONVS[1:], 1):
        cv = _f32_conv(x[scope], wts, scope)
        for kind in KINDS:
            assert P.g1_ratio(cv, A.conv_ref(x[scope], wts, scope, kind)) <= 1.0, (scope, kind)
        ref = A.pool_ref(cv, wts, RR.ATTN_BN[i])
        g = P.g1_ratio(_f32_affine(max_pool_same(cv), wts, RR.ATTN_BN[i]), ref)
        print(f"pool{i + 1}: float32 numpy err/bound {g:.4f}")
        assert g <= 1.0
        # the bound is a few roundings of the two terms, not a tolerance
        assert (ref.bnd <= 4.01 * U * (np.abs(ref.pre * A.bn_fold(wts, RR.ATTN_BN[i])[0])
                                       + np.abs(A.bn_fold(wts, RR.ATTN_BN[i])[1]))).all()
    f1 = x["afc_1"] @ wts["cnn/afc_1/afc_1_weights"] + wts["cnn/afc_1/afc_1_biases"]
    r1 = _f32_affine(np.maximum(f1, 0), wts, RR.ATTN_BN[5])
    for kind in KINDS:
        assert P.g1_ratio(r1, A.relu1_ref(x["afc_1"], wts, kind)) <= 1.0, kind
    o = r1 @ wts["cnn/afc_out/afc_out_weights"] + wts["cnn/afc_out/afc_out_biases"]
    assert P.g1_ratio(o, A.out_ref(r1, wts)) <= 1.0


def _seam_fault(x, wts, scope, R):
    """relu(conv + b) with every R-row tile convolved alone: zero padding at each seam"""
    w, b = wts[f"cnn/{scope}/{scope}_filters"].astype(np.float64), wts[f"cnn/{scope}/{scope}_biases"].astype(np.float64)
    x64 = x.astype(np.float64)
    strips = [conv2d_same(x64[:, r:r + R], w) for r in range(0, x.shape[1], R)]
    return np.maximum(np.concatenate(strips, 1) + b, 0)


@pytest.mark.parametrize("scope", sorted(A.TALL_R))
def test_zero_padding_at_a_tile_seam_fails_the_element_gate(oracle, scope):
    wts, x, R = oracle["wts"], oracle["x"][scope], A.TALL_R[scope]
    bad = _seam_fault(x, wts, scope, R)
    side = A.CONV[scope][4]
    seam = A.map_regions([0, 1], side, side, R)[f"seams{R}"]
    for kind in KINDS:
        ref = A.conv_ref(x, wts, scope, kind)
        over = np.abs(bad - ref.want) > ref.bnd
        g = ratio(bad, ref.want, ref.bnd)
        print(f"{scope} [{kind}] R = {R}: seam fault err/bound {g:.1f}, over the bound on {over[seam].mean():.3f} "
              f"of the seam rows' elements")
        assert g >= 8.0, (scope, kind, g)
        assert not over[~seam].any()                       # the fault is the seam's alone
        # every seam row of every image holds elements over the bound: no seam can hide
        assert over.any(axis=(2, 3))[:, seam[0, :, 0]].all(), (scope, kind)


@pytest.mark.parametrize("i", (1, 2, 3, 4))
def test_bn_before_the_max_or_a_lost_sign_fails_the_pool_gate(oracle, i):
    wts, scope = oracle["wts"], A.CONVS[i][0]
    cv = _f32_conv(oracle["x"][scope], wts, scope)
    ref = A.pool_ref(cv, wts, RR.ATTN_BN[i])
    s, t = A.bn_fold(wts, RR.ATTN_BN[i])
    early = max_pool_same(cv.astype(np.float64) * s + t)
    nosign = ref.pre * np.abs(s) + t
    for name, bad in (("BN before the max", early), ("|gamma|", nosign)):
        over = np.abs(bad - ref.want) > ref.bnd
        print(f"pool{i + 1}: {name}: err/bound {ratio(bad, ref.want, ref.bnd):.3g}, over on {over.mean():.3f}")
        assert ratio(bad, ref.want, ref.bnd) >= 8.0
        assert not over[..., s > 0].any() and over[..., s < 0].mean() >= 0.5


def _lost_plane(what, ref_of, got32, regions):
    """float32 numpy and the intact three-product model pass G2; each dropped product fails it by 8x; under
    bf16 (one product) both operands rounded to bf16 fail it.  G1 alone passes a dropped plane."""
    for d in ("fp32_split", "bf16"):
        ref = ref_of(d, P.MODELS + ("full", "bf16ops"))
        g2, where = P.g2_ratio(got32, ref, d, regions)
        print(f"{what} [{d}]: float32 numpy err/gate {g2:.4f} ({where})")
        assert g2 <= 1.0, (what, d, g2, where)
        for name, mask in regions.items():
            gate = P.g2_gate(ref, d, mask)
            assert gate > 0, (what, d, name)
            fail = {k: P._rms((ref.models[k] - ref.want)[mask]) / gate
                    for k in (("bf16ops",) if d == "bf16" else ("drop_a", "drop_w"))}
            assert min(fail.values()) >= (2.0 if d == "bf16" else 8.0), (what, d, name, fail)
            if d != "bf16":
                assert P._rms((ref.models["full"] - ref.want)[mask]) / gate <= 1.0 / 8, (what, d, name)
        if d == "fp32_split":
            worst = max(ratio(ref.models[k], ref.want, ref.bnd + 0 * ref.want) for k in ("drop_a", "drop_w"))
            print(f"{what}: a dropped plane against the element bound: {worst:.4f}")
            assert worst <= 1.0       # why G2 exists


@pytest.mark.parametrize("scope", ("aconv_3", "aconv_4", "aconv_5"))
def test_a_dropped_plane_fails_the_lost_plane_gate_conv(oracle, scope):
    wts, x = oracle["wts"], oracle["x"][scope]
    side = A.CONV[scope][4]
    _lost_plane(scope, lambda d, nm: A.conv_ref(x, wts, scope, P.KIND[d], nm), _f32_conv(x, wts, scope),
                A.map_regions([0, 1], side, side, A.TALL_R.get(scope, 0)))


def test_a_dropped_plane_fails_the_lost_plane_gate_afc_1(oracle):
    wts, x = oracle["wts"], oracle["x"]["afc_1"]
    f1 = x @ wts["cnn/afc_1/afc_1_weights"] + wts["cnn/afc_1/afc_1_biases"]
    _lost_plane("afc_1", lambda d, nm: A.relu1_ref(x, wts, P.KIND[d], nm),
                _f32_affine(np.maximum(f1, 0), wts, RR.ATTN_BN[5]), A.row_regions([0, 1]))


def test_a_repeated_image_in_a_shared_tile_fails_the_element_gate(oracle):
    """aconv_5's map is 8 x 8: two images share one 128-pixel tile"""
    wts, x = oracle["wts"], oracle["x"]["aconv_5"]
    for kind in KINDS:
        ref = A.conv_ref(x, wts, "aconv_5", kind)
        bad = ref.want.copy()
        bad[1] = bad[0]
        g = ratio(bad, ref.want, ref.bnd)
        over = np.abs(bad - ref.want) > ref.bnd
        print(f"aconv_5 [{kind}]: image 1 = image 0: err/bound {g:.1f}, over on {over[1].mean():.3f} of image 1")
        assert g >= 8.0 and over[1].mean() >= 0.25 and not over[0].any()


def test_regions_cover_both_sides_of_every_seam():
    for scope, R in A.TALL_R.items():
        side = A.CONV[scope][4]
        reg = A.map_regions([0, 5, 10], side, side, R)
        assert all(m.any() for m in reg.values())
        s = reg[f"seams{R}"][0, :, 0]
        assert [r for r in range(side) if s[r]] == sorted({r for r in range(R, side, R)} | {r - 1 for r in range(R, side, R)})
        assert {"whole", "border", "image0", "image5", "image10"} <= set(reg)
        assert not (reg[f"inside{R}"] & reg[f"seams{R}"]).any() and (reg[f"inside{R}"] | reg[f"seams{R}"]).all()
    assert set(A.map_regions([0, 1], 8, 8)) == {"whole", "border", "image0", "image1"}
    assert set(A.row_regions([0, 63])) == {"whole", "row0", "row63"}
