"""What tests/test_gpu_magnitude.py rests on, checked without a GPU (tests/magnitude_cases.py): at every sweep
point of every path the numpy model of the f16 split is finite and inside the bound the GPU test applies; one
step beyond each top point a plane overflows; the weight-scale rule holds on the edge tensors; the rescaled
weight sets are what they claim in float64; and every row named in the tables exists where it is borrowed."""
import numpy as np
import pytest

import graph_op_cases as C
import magnitude_cases as M
import pose_layer_cases as P
from oracle.hgru_ref import conv2d_same

UNITS = M.graph_units()
EDGES = M.edge_units()
_SPLIT_OPS = [(u.name, op.layer) for u in UNITS.values() for op in u.ops if M.has_split(u, op)]


def _op(unit, layer):
    return next(o for o in unit.ops if o.layer == layer)


# ------------------------------------------------------------------------------------- the tables
def test_every_row_exists_and_every_family_is_covered():
    for r in M.GRAPH_CONV_ROWS + (M.EDGE_HALO_ROW,):
        assert r in C.CONV_BY_NAME, r
    assert {dict(c.path)["family"] for c in C.CONV_CASES} <= M.families_covered()
    assert {"x3", "x3w", "halo", "pw", "pwn", "x3w_splitk", "pm", "pm_splitk", "sibling", "conv1_pool_bn",
            "conv1_pool_any"} <= M.families_covered()
    assert any(C.CONV_BY_NAME[r].pool and dict(C.CONV_BY_NAME[r].path)["family"] == "halo" for r in M.GRAPH_CONV_ROWS)
    # the smallest row of each family, by multiply-adds of one image
    cost = lambda c: c.H * c.W * c.K * c.cout   # noqa: E731
    for fam in {dict(c.path)["family"] for c in C.CONV_CASES}:
        rows = [c for c in C.CONV_CASES if dict(c.path)["family"] == fam]
        assert min(rows, key=cost).name in M.GRAPH_CONV_ROWS, fam
    assert dict(C.CONV_BY_NAME[M.EDGE_HALO_ROW].path)["family"] == "halo"
    assert set(M.GRAPH_FC_K) <= set(C.FC_K) and M.EDGE_FC_K in C.FC_K
    assert M.GRAPH_SIBLING in [c[0] for c in C.SIBLING_CASES]
    assert {n for n, _ in M.GRAPH_CONV1} <= {c[0] for c in C.CONV1_CASES}
    assert all(hw in C.CONV1_SIZES for _, hw in M.GRAPH_CONV1)
    assert {op.layer for op in UNITS["fc32"].ops} == set(C.FC_HEADS)
    assert M.POSE_BB_ROW in P.ROWS and M.POSE_BB_N in P.ROWS[M.POSE_BB_ROW].ns
    assert M.POSE_HEAD_ROW in P.ROWS and M.POSE_HEAD_N in P.ROWS[M.POSE_HEAD_ROW].ns
    assert M.J_RESCALE == (-20, -7, 7, 20) and M.J_SMALL == (-6, -12, -24)


def test_loop_rows_are_borrowed_shapes():
    import circuit_shape_cases as S
    import hgru_variant_cases as HV
    by = M.LOOPS_BY_NAME
    assert S.Case("fp32_fft", 2, 9, 32, 5) in S.FFT_FUSED and S.Case("bf16", 2, 9, 32, 5) in S.BF16
    assert by["fused-fp32_fft"].shape == by["fused-bf16"].shape == (2, 9, 32, 5)
    assert by["direct-fp32"].shape == tuple(S.DIRECT[0][1:5]) and S.DIRECT[0].dtype == "fp32"
    assert S.map_ok("fp32_split", *by["direct-fp32_split"].shape[1:3])
    assert by["general-defaults"].shape == HV.SHAPES["fp32_fft"] and "defaults" in HV.VARIANTS
    assert {c.conv for c in M.LOOPS if c.k == 8} == {"direct", "fft", "fft_tiled"}
    assert all(c.shape[1:3] == (5, 7) for c in M.LOOPS if c.k == 8)
    assert set(M.SIX_LAUNCH) <= set(by)
    for c in M.LOOPS:
        wts, X, O0, I0, scope = M.loop_inputs(c)
        assert X.shape == O0.shape == (c.shape[0], c.shape[1], c.shape[2], c.k)
        assert all(f"{scope}/{n}" in wts for n in M.LOOP_UP + M.LOOP_DOWN), c.name


# ------------------------------------------------------------------------------ graph runtime sweeps
def test_the_reference_of_scaled_data_is_the_scaled_reference():
    """float64 of the float32 input times 2^j is ldexp(reference, j), bit for bit, at both ends of the sweep"""
    u = UNITS["halo_8x8_12to12"]
    ref = C.conv_reference(u.name)
    for j in (-24, u.top()):
        pre0, S0, _ = C.conv_terms(ref.x[:3], ref.w, ref.b)
        pre, S, A = C.conv_terms(np.ldexp(ref.x[:3], j), ref.w, np.ldexp(ref.b, j))
        assert np.array_equal(pre, np.ldexp(pre0, j)) and np.array_equal(S, np.ldexp(S0, j))
        assert np.array_equal(A, ref.A)


@pytest.mark.parametrize("name,layer", _SPLIT_OPS, ids=[f"{n}-{l}" for n, l in _SPLIT_OPS])
def test_graph_split_model_is_inside_the_bound_up_to_the_top_and_overflows_beyond(name, layer):
    u = UNITS[name]
    op, top = _op(u, layer), u.top()
    assert 8 <= top <= 16
    for dtype in M.GRAPH_SWEEP_DTYPES:
        for j in M.graph_sweep_points(u, dtype):
            r = M.graph_model_ratio(u, op, dtype, j)
            print(f"{name} {layer} [{dtype}] j={j}: model err/bound {r:.4f}")
            assert r <= 1.0, (dtype, j, r)
    # at -24 the floor is essentially the whole bound
    assert M.floor_share(u, op, -24, "fp32_split") >= 0.99
    assert M.floor_share(u, op, 0, "fp32_split") < 0.5
    # beyond the top: the first step past 2^15.9 leaves the window, and a plane of the unit overflows there or,
    # where the maximum sits in the 7 % between 2^15.9 and 65504, one step on (every image: it may sit on any)
    over = u.overflow()
    assert max(u.split_maxima()) * 2.0 ** (top + 1) > 2.0 ** M.TOP_LOG2 and over in (top + 1, top + 2)
    for o in u.ops:
        M.graph_model_ratio(u, o, "fp32_split", over - 1, images=slice(None))
    with pytest.raises(FloatingPointError):
        for o in u.ops:
            M.graph_model_ratio(u, o, "fp32_split", over, images=slice(None))


# --------------------------------------------------------------------------------------- edge tensors
@pytest.mark.parametrize("name", sorted(EDGES))
def test_edge_tensor_scale_rule(name):
    u = EDGES[name]
    for layer, (w, b) in u.layers().items():
        s = P.weight_scale(w)
        m = float(np.abs(w).max()) * s
        assert 2.0 ** 13 <= m < 2.0 ** 14, (layer, m)
        assert np.log2(s) == int(np.log2(s))
        hi, lo = P.f16_split(w, s)
        if u.edge == "pow2":
            assert np.abs(w).max() == 0.125 and m == 2.0 ** 13 and (np.abs(w) == 0.125).sum() == 1
        if u.edge == "negmax":
            assert w.ravel()[np.abs(w).argmax()] < 0 and w.max() < 0.7 * np.abs(w).max()
        if u.edge == "outlier":
            rest = np.sort(np.abs(w).ravel())[:-1]
            assert rest.max() * 2.0 ** 19 < np.abs(w).max() and M.subnormal_lo_share(w) >= 0.5
            # the derivation's claims: every such weight is off by at most 2^-25 / s, and by more than fp32-class
            # (2^-22 of itself) on at least half of them
            err = np.abs(hi + lo - w.astype(np.float64))
            sub = np.abs(w) * s < 2.0 ** -3
            assert sub.sum() == w.size - 1 and (err[sub] <= 2.0 ** -25 / s).all()
            assert (err > 2.0 ** -22 * np.abs(w)).mean() >= 0.5
        else:
            assert M.subnormal_lo_share(w) < 0.5
            assert (np.abs(hi + lo - w.astype(np.float64)) <= 2.0 ** -21 * np.abs(w)).mean() > 0.9


@pytest.mark.parametrize("name", sorted(EDGES))
def test_edge_tensor_split_model_is_inside_the_bound(name):
    """the first two by the row's ordinary bound; the outlier tensor needs its term and is inside with it"""
    u = EDGES[name]
    for op in u.ops:
        for dtype in M.GRAPH_SWEEP_DTYPES:
            r = M.graph_model_ratio(u, op, dtype, 0, images=slice(None), outlier=u.edge == "outlier")
            print(f"{name} {op.layer} [{dtype}]: model err/bound {r:.4f}")
            assert r <= 1.0, (op.layer, dtype, r)
    if u.edge == "outlier":
        assert max(M.graph_model_ratio(u, op, "fp32_split", 0, images=slice(None)) for op in u.ops) > 1.0


# ---------------------------------------------------------------------------------------- pose model
def _bb():
    row = P.ROWS[M.POSE_BB_ROW]
    return row, P.pose_weights(row.H, row.W, row.width), P.inputs(row, M.POSE_BB_N)[0]


def test_pose_weight_sets_do_what_they_state():
    """in float64: the rescaled sets leave the tap behind the BN unchanged (fc_1's tap times 2^j), the sweep sets
    scale the layer's input by 2^j exactly"""
    row, wts, depth = _bb()
    base = P.pool1_ref(depth[:1], wts).want
    c2 = P.conv_ref(base.astype(np.float32), wts, "conv_2", "batch_normalization_1", "fp32", names=()).want
    for j in (-20, 7):
        wj = M.pose_rescaled_weights(row, "conv_2", j)
        got = P.conv_ref(base.astype(np.float32), wj, "conv_2", "batch_normalization_1", "fp32", names=()).want
        np.testing.assert_allclose(got, c2, rtol=1e-12, atol=1e-12 * np.abs(c2).max())
        ws = M.pose_sweep_weights(row, "backbone", j)
        np.testing.assert_allclose(P.pool1_ref(depth[:1], ws).want, np.ldexp(base, j), rtol=1e-12,
                                   atol=1e-12 * np.abs(base).max() * 2.0 ** j)
        s0, t0 = P.bn_fold(wts, "batch_normalization_3")
        s1, t1 = P.bn_fold(M.pose_sweep_weights(row, "fc_1", j), "batch_normalization_3")
        assert np.array_equal(s1, np.ldexp(s0, j)) and np.array_equal(t1, np.ldexp(t0, j))
        for layer in M.POSE_LAYERS:
            bn = M._BN_AFTER[layer]
            s2, t2 = P.bn_fold(M.pose_rescaled_weights(row, layer, j), bn)
            s3, t3 = P.bn_fold(wts, bn)
            assert np.array_equal(s2, np.ldexp(s3, -j)) and np.array_equal(t2, t3)


@pytest.mark.parametrize("dtype", M.POSE_SWEEP_DTYPES)
def test_backbone_split_model_is_inside_the_bound_up_to_the_top_and_overflows_beyond(dtype):
    row, wts, depth = _bb()
    top = M.pose_top("backbone")
    x0 = P.pool1_ref(depth[:1], wts).want
    assert np.abs(P.pool1_ref(depth, wts).want).max() * P.BB_ASCALE * 2.0 ** top <= 2.0 ** M.TOP_LOG2
    name = "hihi" if dtype == "bf16" else "full"
    for j in M.pose_sweep_points("backbone", dtype):
        wj = M.pose_sweep_weights(row, "backbone", j)
        x = np.ldexp(x0, j).astype(np.float32)
        ref = M.backbone_ref(x, wj, dtype, row.H, names=(name,) + P.MODELS)
        r = P.ratio(ref.models[name], ref.want, ref.bnd)
        print(f"backbone [{dtype}] j={j}: model err/bound {r:.4f}")
        assert np.isfinite(ref.models[name]).all() and r <= 1.0, (j, r)
        if j in M.pose_g2_points("backbone") and dtype != "bf16":   # the dropped-plane models are 16x off or more
            g2 = P.g2_ratio(ref.models[name], ref, dtype, {"whole": np.ones(x.shape[:3], bool)})[0]
            print(f"backbone [{dtype}] j={j}: model err/gate {g2:.4f}")
            assert g2 <= 1.0, (j, g2)
    xmax = np.abs(P.pool1_ref(depth, wts).want).max()
    over = M.overflow_j([xmax], P.BB_ASCALE)
    assert xmax * P.BB_ASCALE * 2.0 ** (top + 1) > 2.0 ** M.TOP_LOG2 and over in (top + 1, top + 2)
    P.f16_split(np.ldexp(P.pool1_ref(depth, wts).want, over - 1).astype(np.float32), P.BB_ASCALE)
    with pytest.raises(FloatingPointError):
        P.f16_split(np.ldexp(P.pool1_ref(depth, wts).want, over).astype(np.float32), P.BB_ASCALE)


def test_fc1_split_model_is_inside_the_bound_up_to_the_top_and_overflows_beyond():
    """fc_1 on rows of the float64 reference of its input, the hgru tap, the row that holds the maximum among them"""
    row = P.ROWS[M.POSE_HEAD_ROW]
    tap = M.hgru_tap_reference()
    ceil = float(np.abs(tap).max())
    top = M.pose_top("fc_1")
    assert ceil * 2.0 ** top <= 2.0 ** M.TOP_LOG2 < ceil * 2.0 ** (top + 1)
    x0 = tap[sorted({0, 1, int(np.abs(tap).max(1).argmax())})].astype(np.float32)
    assert tap.shape == (M.POSE_HEAD_N, row.K) and np.abs(x0).max() == np.float32(ceil)
    for dtype in ("fp32_fft", "bf16"):
        name = "hihi" if dtype == "bf16" else "full"
        for j in M.pose_sweep_points("fc_1", dtype):
            wj = M.pose_sweep_weights(row, "fc_1", j)
            ref = P.fc1_ref(np.ldexp(x0, j), wj, P.KIND[dtype], names=(name,) + P.MODELS)
            r = P.ratio(ref.models[name], ref.want, ref.bnd)
            print(f"fc_1 [{dtype}] j={j}: model err/bound {r:.4f}")
            assert r <= 1.0, (dtype, j, r)
            if j in M.pose_g2_points("fc_1") and dtype != "bf16":
                assert P.g2_ratio(ref.models[name], ref, dtype, {"whole": np.ones(len(x0), bool)})[0] <= 1.0
    over = M.overflow_j([ceil])
    assert over in (top + 1, top + 2)
    P.f16_split(np.ldexp(x0, over - 1), 1.0)
    with pytest.raises(FloatingPointError):
        P.f16_split(np.ldexp(x0, over), 1.0)


# ----------------------------------------------------------------------------------------- hGRU loops
def test_loop_rescaling_leaves_the_oracle_unchanged():
    """the rescaled weight set is the same circuit: every O_t and I_t of the float64 oracle to 1e-12"""
    import circuit_shape_cases as S
    from oracle import hgru_ref as R
    c = M.LOOPS_BY_NAME["fused-fp32_fft"]
    wts, X, O0, _, scope = M.loop_inputs(c)
    base = R.hgru_forward(X.astype(np.float64), O0, wts, M.LOOP_T, keep_inputs=True)
    for j in (-20, 7):
        got = R.hgru_forward(X.astype(np.float64), O0, M.loop_rescaled(wts, scope, j), M.LOOP_T, keep_inputs=True)
        for a, b in zip([got[0]] + got[1] + got[2], [base[0]] + base[1] + base[2]):
            assert np.abs(a - b).max() <= 1e-12
    assert scope == S.SCOPE


@pytest.mark.parametrize("name", [t.name for t in M.TWINS])
def test_twin_is_the_baseline_and_its_split_model_is_inside_the_bound(name):
    import circuit_shape_cases as S
    t = M.TWINS_BY_NAME[name]
    c = M.TWIN_LOOPS[t.loop]
    ssf, top = c.shape[3], M.twin_top(name)
    assert set(M.TWIN_SMALL[name]) | set(M.TWIN_DROPPED[name]) == set(M.J_SMALL)
    base = M.half_step(t, *M.twin_inputs(t, 0))
    # the sensitivity condition, which the twin meets and O0 times 2^j alone does not
    if M.twin_aux(t)['recurrent_nl'] == 'tanh':
        assert (np.abs(base["arg"]) < 3).mean() >= 0.9
        wts, X, O0, I0, scope = M.twin_inputs(t, 0)
        assert (np.abs(M.half_step(t, wts, X, np.ldexp(O0, top), I0, scope)["arg"]) < 3).mean() < 0.5
    else:
        assert (base["arg"] > 0).mean() >= 0.25
    for j in M.twin_points(name):
        ref, e32 = M.twin_reference(name, j)
        assert np.abs(ref - base["I"]).max() <= 1e-12, j
        errs = S.metrics(M.half_step(t, *M.twin_inputs(t, j), model=True)["I"], ref, ssf)
        print(f"{name} j={j}: model rel_inf " + "  ".join(f"{e:.3e}" for e in errs))
        assert all(e <= S.fp32_class_bound(r) for e, r in zip(errs, e32)), (j, errs)
    j = max(M.TWIN_DROPPED[name])       # the nearest dropped point: the model itself misses the bound there
    ref, e32 = M.twin_reference(name, j)
    errs = S.metrics(M.half_step(t, *M.twin_inputs(t, j), model=True)["I"], ref, ssf)
    assert max(e / S.fp32_class_bound(r) for e, r in zip(errs, e32)) > 1.0, (j, errs)
    # the top is the edge
    mx = M.twin_split_maxima(name)
    over = M.overflow_j(mx)
    assert max(mx) * 2.0 ** top <= 2.0 ** M.TOP_LOG2 < max(mx) * 2.0 ** (top + 1) and over in (top + 1, top + 2)
    with pytest.raises(FloatingPointError):
        M.half_step(t, *M.twin_inputs(t, over), model=True)
    # hidden_init = 'identity' at its own top: X itself is scaled there and nothing can take the factor out of the
    # drive, so a tanh path saturates and that run checks range and finiteness only; the relu path stays sensitive
    mi = M.twin_split_maxima(name, True)
    jt = M.twin_top(name, True)
    assert max(mi) * 2.0 ** jt <= 2.0 ** M.TOP_LOG2 < max(mi) * 2.0 ** (jt + 1)
    arg = M.half_step(t, *M.twin_inputs(t, jt, True))["arg"]
    if M.twin_aux(t)['recurrent_nl'] == 'tanh':
        assert (np.abs(arg) < 3).mean() < 0.5
    else:
        assert (arg > 0).mean() >= 0.25


def test_cnf_worst_case_is_at_the_ceiling_and_inside_the_bound():
    import circuit_channel_cases as CC
    import circuit_fft_cases as F
    import circuit_shape_cases as S
    assert F.SPEC_SCALE == M.SPEC_SCALE and F.DTYPE == "fp32_split"
    for conv, (n, h, w) in M.CNF_CASES.items():
        wts, X, O0, I0, scope, jc = M.cnf_inputs(conv)
        assert O0.min() > 0 and O0.shape == (n, h, w, M.CNF_K)
        hh, ww = min(h, 64), min(w, 64)
        dc = max(O0[:, y:y + 64, x:x + 64].sum((1, 2)).max() for y in range(0, h, 64) for x in range(0, w, 64)) * M.SPEC_SCALE
        assert 0.75 * 2.0 ** M.TOP_LOG2 <= hh * ww * O0.max() * M.SPEC_SCALE * 0.75 <= dc <= 2.0 ** M.TOP_LOG2
        assert hh * ww * O0.max() * M.SPEC_SCALE * 2 > 65520          # one step on the worst case overflows
        ref, e32 = M.cnf_reference(conv)
        assert (np.abs(ref) < 0.995).mean() >= 0.9                   # unsaturated
    assert M.CNF_CASES["fft_tiled"][1] > 64 >= M.CNF_CASES["fft_tiled"][2]      # one seam
    # the one-window case through the split model
    conv = "fft"
    wts, X, O0, I0, scope, jc = M.cnf_inputs(conv)
    t = M.Twin("cnf", None, None, "spec")
    ref, e32 = M.cnf_reference(conv)
    mod = M.half_step(t, wts, X, O0, I0, scope, model=True, aux=CC.aux_of(M.CNF_VARIANT))["I"]
    errs = S.metrics(mod, ref, M.CNF_SSF)
    print("cnf fft: model rel_inf " + "  ".join(f"{e:.3e}" for e in errs))
    assert all(e <= S.fp32_class_bound(r) for e, r in zip(errs, e32)), errs


@pytest.mark.parametrize("edge", M.EDGE_TENSORS)
def test_circuit_edge_tensor_scale_rule(edge):
    """the spectrum of p_r is what the FFT path packs: its scale rule, for each edge tensor"""
    w, X, O0, scope = M.circuit_edge_weights(edge)
    p_r = w[f"{scope}/p_r"]
    if edge == "pow2":
        assert np.abs(p_r).max() == 0.125
    if edge == "negmax":
        assert p_r.ravel()[np.abs(p_r).argmax()] < 0
    if edge == "outlier":
        assert np.sort(np.abs(p_r).ravel())[-2] * 2.0 ** 19 < np.abs(p_r).max()
    G = M.kernel_spectrum(p_r.astype(np.float64))
    g = np.stack([G.real, G.imag]).astype(np.float32)
    assert 2.0 ** 13 <= np.abs(g).max() * P.weight_scale(g) < 2.0 ** 14
    ref, e32 = M.circuit_edge_reference(edge)
    assert np.isfinite(ref).all() and np.abs(ref).max() > 0.1
