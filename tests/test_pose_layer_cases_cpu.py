"""The tables, models and gates of tests/pose_layer_cases.py checked without a GPU, so that no gate of
tests/test_gpu_pose_layers.py can pass vacuously: every row's shape is one the library accepts, the
split emulation reconstructs its operands, and on every row's inputs (the layer input taken from the
float64 oracle instead of the GPU) float32 numpy of the layer passes G1 and G2, the intact three-product
model passes G2, every degradation fails it, and enough of the relu's input is positive."""
import numpy as np
import pytest

import pose_layer_cases as P
from graph_op_cases import U

N_CPU = 2        # images per backbone row; the conditions are properties of the weights and crops, not of n
M_CPU = 3        # batch rows per head row


def test_every_row_has_a_shape_the_library_accepts():
    for r in P.BACKBONE_ROWS + P.HEAD_ROWS:
        for d in r.dtypes:
            assert P.shape_ok(r.H, r.W, d), (r.name, d)
    assert not P.shape_ok(16, 32, "fp32_split") and not P.shape_ok(48, 32, "fp32_split")
    assert not P.shape_ok(24, 32, "fp32") and not P.shape_ok(32, 96, "bf16") and P.shape_ok(48, 32, "fp32")
    for var, rows in P.SWITCH_ROWS.items():
        assert len(rows) == 4 and sum(nm.startswith("bb") for nm, _, _ in rows) == 2, var
        for nm, d, n in rows:
            assert d in P.ROWS[nm].dtypes and (n in P.ROWS[nm].ns or nm.startswith("bb")), (var, nm, d, n)
    assert all(d == "bf16" for _, d, _ in P.SWITCH_ROWS["MP_FC_BK64=0"])
    # the tile choices the rows name: conv_small_tiles' 128-workgroup limit of the 32-row tiling
    wg = lambda r, n: n * (r.W // 32) * (r.H // 32)
    assert wg(P.ROWS["bb_32x32"], 3) <= 128 < wg(P.ROWS["bb_32x32"], 129)
    assert wg(P.ROWS["bb_32x32"], 96) <= 128 and wg(P.ROWS["bb_32x32"], 33) <= 128   # its untapped slices
    assert wg(P.ROWS["bb_64x32"], 65) > 128 and wg(P.ROWS["bb_32x64"], 65) > 128
    assert P.slice_ends(129) == [95, 128] and P.slice_ends(65) == [63, 64] and P.slice_ends(63) == [62]


def test_split_emulation_reconstructs_operands():
    """hi + lo carries the operand to 2^-22 relative; a subnormal lo (activations below ~2^-3 / scale)
    leaves at most 2^-25 / scale, which is the bound's A term."""
    rng = np.random.default_rng(5)
    for scale in (1.0, P.BB_ASCALE, 2.0 ** 20):
        v = (rng.standard_normal(200000) * np.exp2(rng.integers(-18, 3, 200000)) * (2.0 ** 9 / scale)).astype(np.float32)
        hi, lo = P.f16_split(v, scale)
        err = np.abs(hi + lo - v.astype(np.float64))
        assert (err <= 2.0 ** -22 * np.abs(v) + 2.0 ** -25 / scale).all()
        big = np.abs(v) * scale >= 2.0 ** -2       # lo is normal
        assert big.any() and (err[big] <= 2.0 ** -22 * np.abs(v[big])).all()
    w = P.pose_weights(16, 32, 32)["cnn/conv_2/conv_2_filters"]
    s = P.weight_scale(w)
    assert 2.0 ** 13 <= np.abs(w).max() * s < 2.0 ** 14
    hi, lo = P.f16_split(w, s)
    assert (np.abs(hi + lo - w.astype(np.float64)) <= 2.0 ** -22 * np.abs(w) + 2.0 ** -25 / s).all()
    assert (P.to_bf16(np.float32([1.0, 1.00390625, 1.01171875, -3.0])) == [1.0, 1.0, 1.015625, -3.0]).all()


def test_width_replacement_reaches_every_dependent_weight():
    w = P.pose_weights(16, 32, 32)
    assert w["cnn/fc_1/fc_1_weights"].shape == (16 * 32 * 64, 32) and w["cnn/fc_1/fc_1_biases"].shape == (32,)
    assert w["cnn/batch_normalization_4/gamma"].shape == (32,) and w["cnn/fc_out/fc_out_weights"].shape == (32, 69)
    assert w["cnn/contextual_circuit/rho"].shape == (P.T,)
    assert 0.5 < np.abs(w["cnn/fc_1/fc_1_weights"]).max() / np.sqrt(6.0 / (16 * 32 * 64 + 32)) <= 1.0


def test_regions_are_non_empty_and_hold_both_sides_of_each_seam():
    for r in P.BACKBONE_ROWS:
        for n in r.ns:
            imgs = P.ref_images(n)
            assert imgs[0] == 0 and imgs[-1] == n - 1 and set(P.slice_ends(n)) <= set(imgs)
            if n >= 65:
                assert {0, 31, 32, 63, 64, n - 1} <= set(imgs)
            reg = P.map_regions(imgs, n, r.H, r.W)
            assert all(m.any() for m in reg.values())
            assert {"whole", "border", "rows7|8", f"image{n - 1}"} <= set(reg)
            assert ("rows31|32" in reg) == (r.H > 32) and ("cols31|32" in reg) == (r.W > 32)
            for k, m in reg.items():
                if k.startswith("rows"):
                    lo, hi = map(int, k[4:].split("|"))
                    assert m[:, lo].all() and m[:, hi].all() and m.sum() == len(imgs) * 2 * r.W
                if k.startswith("cols"):
                    assert m[:, :, 31].all() and m[:, :, 32].all() and m.sum() == len(imgs) * 2 * r.H
            b = reg["border"]
            assert b[:, 0].all() and b[:, -1].all() and b[:, :, 0].all() and b[:, :, -1].all() and not b[:, 1:-1, 1:-1].any()
    assert "rows31|32" in P.map_regions([0, 1], 2, 64, 32) and "cols31|32" in P.map_regions([0, 1], 2, 32, 64)
    for r in P.HEAD_ROWS:
        for n in r.ns:
            rows = P.fc_ref_rows(r, n)
            want = {i for i in P.FC_ROWS + (n - 1,) if i < n} | {t + d for t in range(32, n, 32) for d in (-1, 0)}
            assert want <= set(rows)
            reg = P.fc_regions(rows, n)
            assert all(m.any() for m in reg.values()) and {f"row{i}" for i in want} <= set(reg)
    assert {127, 128, 255, 256} <= set(P.fc_region_rows(257)) and P.fc_region_rows(1) == [0]


def _f32_conv_layer(x, wts, layer, bn, bf16):
    from oracle.hgru_ref import conv2d_same
    s, t = P.bn_fold(wts, bn)
    y = conv2d_same(x.astype(np.float32), wts[f"cnn/{layer}/{layer}_filters"]) + wts[f"cnn/{layer}/{layer}_biases"]
    y = np.maximum(y, 0) * s.astype(np.float32) + t.astype(np.float32)
    assert y.dtype == np.float32
    return P.to_bf16(y) if bf16 else y


def _conditions(what, got32, ref_of, dtypes, regions, bf16_fail=2.0):
    """float32 numpy passes G1 and G2 at every dtype of the row; the intact model passes G2 and each
    degradation fails it by at least 8x.  bf16's degradation is both operands rounded to bf16: nominally 4x
    over the gate, asserted at `bf16_fail`."""
    for d in dtypes:
        ref = ref_of(d, P.MODELS + ("full", "bf16ops"))
        assert (ref.pre > 0).mean() >= 0.25, what
        g1 = P.g1_ratio(got32(d), ref)
        g2, where = P.g2_ratio(got32(d), ref, d, regions)
        print(f"{what} [{d}]: float32 numpy err/bound {g1:.4f} err/gate {g2:.4f} ({where})")
        assert g1 <= 1.0 and g2 <= 1.0, (what, d, g1, g2, where)
        for name, mask in regions.items():
            gate = P.g2_gate(ref, d, mask)
            assert gate > 0, (what, d, name)
            fail = {k: P._rms((ref.models[k] - ref.want)[mask]) / gate
                    for k in (("bf16ops",) if d == "bf16" else ("drop_a", "drop_w"))}
            assert min(fail.values()) >= (bf16_fail if d == "bf16" else 8.0), (what, d, name, fail)
            if d != "bf16":
                intact = P._rms((ref.models["full"] - ref.want)[mask]) / gate
                assert intact <= 1.0 / 8, (what, d, name, intact)


@pytest.mark.parametrize("name", [r.name for r in P.BACKBONE_ROWS])
def test_backbone_row_conditions(name):
    row = P.ROWS[name]
    wts = P.pose_weights(row.H, row.W, row.width)
    depth, _ = P.inputs(row, N_CPU)
    imgs = list(range(N_CPU))
    reg = P.map_regions(imgs, N_CPU, row.H, row.W)
    p1 = P.pool1_ref(depth, wts)
    assert (p1.pre > 0).mean() >= 0.25
    from oracle.hgru_ref import conv2d_same, max_pool_same
    s, t = P.bn_fold(wts, "batch_normalization")
    c1 = np.maximum(conv2d_same(depth, wts["cnn/conv_1/conv_1_filters"]) + wts["cnn/conv_1/conv_1_biases"], 0)
    g1 = P.g1_ratio(max_pool_same(c1) * s.astype(np.float32) + t.astype(np.float32), p1)
    print(f"{name} pool1: float32 numpy err/bound {g1:.4f}")
    assert g1 <= 1.0
    x2 = p1.want.astype(np.float32)
    _conditions(f"{name} conv2", lambda d: _f32_conv_layer(x2, wts, "conv_2", "batch_normalization_1", False),
                lambda d, nm: P.conv_ref(x2, wts, "conv_2", "batch_normalization_1", P.conv_kind(d, row.H), names=nm),
                row.dtypes, reg)
    x3 = P.conv_ref(x2, wts, "conv_2", "batch_normalization_1", "fp32", names=()).want.astype(np.float32)
    _conditions(f"{name} conv3", lambda d: _f32_conv_layer(x3, wts, "conv_3", "batch_normalization_2", d == "bf16"),
                lambda d, nm: P.conv_ref(x3, wts, "conv_3", "batch_normalization_2", P.conv_kind(d, row.H),
                                         store_bf16=d == "bf16", names=nm),
                row.dtypes, reg, bf16_fail=1.0)   # the stored map's own bf16 rounding is most of both errors


@pytest.mark.parametrize("name", [r.name for r in P.HEAD_ROWS])
def test_head_row_conditions(name):
    from oracle import hgru_ref as R
    row = P.ROWS[name]
    wts = P.pose_weights(row.H, row.W, row.width)
    depth, o0 = P.inputs(row, M_CPU)
    _, inter = R.hgru_pose_forward(depth, wts, o0, P.T, np.float64, keep=True)
    x = inter["hgru_bn"].reshape(M_CPU, -1).astype(np.float32)
    rows = list(range(M_CPU))
    reg = P.fc_regions(rows, M_CPU)
    w32, b32 = wts["cnn/fc_1/fc_1_weights"], wts["cnn/fc_1/fc_1_biases"]
    f1 = x @ w32 + b32
    assert f1.dtype == np.float32
    _conditions(f"{name} fc1", lambda d: f1, lambda d, nm: P.fc1_ref(x, wts, P.KIND[d], names=nm), row.dtypes, reg)
    s, t = P.bn_fold(wts, "batch_normalization_4")
    r1 = np.maximum(f1, 0) * s.astype(np.float32) + t.astype(np.float32)
    ref = P.relu1_ref(f1, wts)
    assert (ref.pre > 0).mean() >= 0.25 and P.g1_ratio(r1, ref) <= 1.0
    out = r1 @ wts["cnn/fc_out/fc_out_weights"] + wts["cnn/fc_out/fc_out_biases"]
    assert P.g1_ratio(out, P.out_ref(r1, wts)) <= 1.0
    # G1 alone cannot see a lost plane at this K, which is why G2 exists
    lost = P.fc1_ref(x, wts, "fp32_split")
    assert P.ratio(lost.models["drop_a"], lost.want, lost.bnd) <= 1.0
    assert 2 * U * row.K > 1e-3
