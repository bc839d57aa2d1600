"""Every kernel path of the layer-graph runtime, one op at a time, against a float64 reference of
that op computed from the GPU's own input to it (tests/graph_op_cases.py: tables, inputs, bounds).

The gate is per element, |got - ref| <= bound(dtype, K, S, A), never a norm over the tensor; each
case asserts through ``graph_path:<scope>`` that the library took the kernel its row names.  Every
test prints its max err / bound.

Measured maxima of err / bound on an MI355X (information, not a gate), fp32_split / fp32 / bf16:
  conv rows (33 rows, all batch sizes)       0.075 / 0.145 / 0.463   (largest at K = 8; 1e-4 at K = 6400)
  the same rows under a dispatch switch      0.075 (MP_IGEMM_PW=0, the x3 im2col kernel at K = 8)
  conv reading a concat slice                0.891 / 0.073   (the identity-weight producer: one tap of
                                             weight 1, so the activation's subnormal lo, the A term, is the
                                             whole bound; the conv under test itself 0.003 / 0.014)
  conv writing a concat slice                0.061 / 0.163
  fused conv1 + pool (every dtype)           0.372
  unfused 1 -> C convs                       0.112 / 0.173 / 0.635
  1x1 siblings                               0.118 / 0.199
  avg pool                                   0.471 of 4u sum|x| / count
  fc, K % 32 == 0                            0.025 / 0.094 / 0.335;  K = 40 (fp32 kernel) 0.079
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import graph_op_cases as C
from graph_op_cases import U, bound, conv_expected, conv_terms, forward, layer_w, layer_weights, make_ctx, ratio
from graph_op_cases import fc_graph as _fc_graph, sibling_graph as _sibling_graph

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _G():
    return C.pkg()._graph


def _report(what, dtype, r):
    print(f"err/bound {what} [{dtype}]: {r:.4f}")
    assert r <= 1.0, (what, dtype, r)


def _input_conditions(pre_dense, pool):
    assert C.dense_positive_fraction(pre_dense) >= 0.25
    if pool:
        assert len(C.pool_winners(pre_dense)) >= 2


# ------------------------------------------------------------------------------------ conv rows
_CONV_PARAMS = [(c.name, d) for c in C.CONV_CASES for d in ("fp32_split", "fp32") + (("bf16",) if c.bf16 else ())]


@pytest.mark.parametrize("name,dtype", _CONV_PARAMS, ids=[f"{n}-{d}" for n, d in _CONV_PARAMS])
def test_conv_row(name, dtype):
    c, ref = C.CONV_BY_NAME[name], C.conv_reference(name)
    _input_conditions(ref.pre[:ref.n_dense], c.pool)
    path, fused, worst = C.run_conv_case(name, dtype)
    want = c.expected(dtype)
    assert {k: path[k] for k in want} == want, (path, want)
    assert fused == want["pool"]
    _report(name, dtype, worst)


def _conv_op_ratio(x, w, b, got, kind, pool=False, stride=1):
    pre, S, A = conv_terms(x, w, b, stride)
    want, bnd = conv_expected(pre, S, A, kind, int(np.prod(w.shape[:3])), pool)
    return ratio(got, want, bnd)


_SLICE = {   # H, W, cin, cout, k, expected path of the conv under test (f16-split dtypes)
    "halo": (8, 8, 32, 32, 3, dict(family="halo", wr=8, ch=32, ks=3)),
    "pointwise": (5, 5, 32, 64, 1, dict(family="pwn", nch=1, nb=2)),
}


@pytest.mark.parametrize("dtype", ["fp32_split", "fp32"])
@pytest.mark.parametrize("kind", sorted(_SLICE))
def test_conv_reads_a_concat_slice(kind, dtype):
    """The conv's input is channels [8, 8 + Cin) of a concat group (cix = 8, ldx = Cin + 8).  Its
    producer is a 1x1 identity-weight conv, so the impulse images reach it (as relu(x): the +1
    impulses); the reference starts from the producer's output as the GPU wrote it."""
    H, W, cin, cout, k, want = _SLICE[kind]
    g = _G().GraphRecorder(H, W, cin)
    p1 = g.conv(g.input, cin, 8, "p1", k=1)
    p2 = g.conv(g.input, cin, cin, "p2", k=1)
    cat = g.concat([p1, p2])
    y = g.conv(p2, cin, cout, "c", k=k)
    name = f"slice_in_{kind}"
    x = C.conv_inputs(name, H, W, cin, 3)
    w, b = layer_weights(name, (k, k, cin, cout))
    w1, b1 = layer_weights(name + "/p1", (1, 1, cin, 8))
    wts = {**layer_w("c", w, b), **layer_w("p1", w1, b1),
           **layer_w("p2", np.eye(cin, dtype=np.float32).reshape(1, 1, cin, cin), np.zeros(cin, np.float32))}
    ctx = make_ctx(g, [cat, y], wts, dtype)
    gcat, gy = forward(ctx, [cat, y], x)
    eye = np.eye(cin, dtype=np.float32).reshape(1, 1, cin, cin)
    assert gcat[-2, ..., 8:].max() > 0.99                # the last +1 impulse reached the conv's input
    _input_conditions(conv_terms(gcat[:3, ..., 8:], w, b)[0], False)
    path = _G().conv_path(ctx, "c")
    if dtype != "fp32":
        assert {q: path[q] for q in want} == want, path
    _report(name, dtype, max(_conv_op_ratio(gcat[..., 8:], w, b, gy, dtype),
                             _conv_op_ratio(x, w1, b1, gcat[..., :8], dtype),
                             _conv_op_ratio(x, eye, np.zeros(cin, np.float32), gcat[..., 8:], dtype)))


@pytest.mark.parametrize("dtype", ["fp32_split", "fp32"])
@pytest.mark.parametrize("kind", ["halo", "pointwise"])
def test_conv_writes_a_concat_slice(kind, dtype):
    """The conv's output is channels [6, 6 + Cout) of a concat with a 6-channel sibling conv
    (coff = 6, ldo = Cout + 6: every store is scalar).  The whole concat tensor is checked, so a
    store spilling into the neighbour's channels fails."""
    H, W, cin, cout, k, want = {"halo": (8, 8, 16, 32, 3, dict(family="halo", wr=8, ch=16, ks=3)),
                                "pointwise": (5, 5, 8, 16, 1, dict(family="pw", nch=1))}[kind]
    g = _G().GraphRecorder(H, W, cin)
    s = g.conv(g.input, cin, 6, "s", k=k)
    y = g.conv(g.input, cin, cout, "c", k=k)
    cat = g.concat([s, y])
    name = f"slice_out_{kind}"
    x = C.conv_inputs(name, H, W, cin, 3)
    w, b = layer_weights(name, (k, k, cin, cout))
    ws, bs = layer_weights(name + "/s", (k, k, cin, 6))
    ctx = make_ctx(g, [cat], {**layer_w("c", w, b), **layer_w("s", ws, bs)}, dtype)
    _input_conditions(conv_terms(x[:3], w, b)[0], False)
    worst = 0.0
    for n in (1, 3, len(x)):
        gcat, = forward(ctx, [cat], x[:n])
        worst = max(worst, _conv_op_ratio(x[:n], ws, bs, gcat[..., :6], dtype),
                    _conv_op_ratio(x[:n], w, b, gcat[..., 6:], dtype))
    path = _G().conv_path(ctx, "c")
    if dtype != "fp32":
        assert {q: path[q] for q in want} == want, path
    assert ctx.info("graph_buffers") == 1
    _report(name, dtype, worst)


# ------------------------------------------------------------------------ planner: conv1 + pool
_CONV1_PARAMS = C.conv1_params()


@pytest.mark.parametrize("dtype", ["fp32_split", "fp32", "bf16"])
@pytest.mark.parametrize("case,hw", _CONV1_PARAMS, ids=[f"{n}-{h}x{w}" for n, (h, w) in _CONV1_PARAMS])
def test_conv1_pool_fusion(case, hw, dtype):
    cout, form, family, H, W, x, w, b = C.conv1_case(case, hw)
    G = _G()
    g = G.GraphRecorder(H, W, 1)
    y = g.conv(g.input, 1, cout, "c")
    p = g.pool(y)
    outs = {"plain": [p], "oddH": [p], "second_consumer": [y, p]}.get(form)
    if form == "concat":   # the pooled map lands at channel 1 of a 65-channel buffer
        outs = [g.concat([g.pool(g.input, avg=True), p])]
    name = f"conv1_{case}_{H}x{W}"
    pre = conv_terms(x[:11], w, b)[0]
    _input_conditions(pre, True)
    ctx = make_ctx(g, outs, layer_w("c", w, b), dtype)
    worst = 0.0
    for n in (1, 3, len(x)):
        got = forward(ctx, outs, x[:n])
        path = G.conv_path(ctx, "c")
        kind = C.conv_bound_kind(dtype, path["family"])
        gp = got[-1]
        if form == "concat":
            assert ratio(gp[..., :1], C.avg_pool_same(x[:n].astype(np.float64)),
                         4 * U * C.avg_pool_same(np.abs(x[:n]).astype(np.float64)) + 1e-300) <= 1.0
            gp = gp[..., 1:]
        worst = max(worst, _conv_op_ratio(x[:n], w, b, gp, kind, pool=True))
        if form == "second_consumer":
            worst = max(worst, _conv_op_ratio(x[:n], w, b, got[0], kind))
    if family:
        assert path["family"] == family and path["pool"] == 1, path
    else:   # unfused: the 9-tap conv on its dtype's own kernel, the pool on pool2_kernel
        assert path["pool"] == 0 and path["family"] == ("f32_im2col" if dtype == "fp32" else "x3w" if cout > 64 else "x3"), path
    assert ctx.info("graph_fused_pools") == (1 if family else 0)
    assert ctx.info("graph_fused_1x1") == 0
    assert ctx.info("graph_buffers") == 2
    _report(name, dtype, worst)


# ----------------------------------------------------------------------- planner: 1x1 siblings
@pytest.mark.parametrize("dtype", ["fp32_split", "fp32"])
@pytest.mark.parametrize("case", [c[0] for c in C.SIBLING_CASES])
def test_1x1_siblings(case, dtype, monkeypatch):
    _, cs, couts, n_fused, families = next(c for c in C.SIBLING_CASES if c[0] == case)
    g, src, sibs, pools = _sibling_graph(cs, couts)
    outs = [src] + sibs + pools
    x = C.conv_inputs(case, 5, 5, 8, 11)
    wts, lw = {}, {}
    lw["src"] = layer_weights(case + "/src", (1, 1, 8, cs))
    for i, co in enumerate(couts):
        lw[f"s{i}"] = layer_weights(f"{case}/s{i}", (1, 1, cs, co))
    for nm, (w, b) in lw.items():
        wts.update(layer_w(nm, w, b))

    def run():
        ctx = make_ctx(g, outs, wts, dtype)
        return ctx, forward(ctx, outs, x)

    ctx, got = run()
    gsrc = got[0]
    worst = _conv_op_ratio(x, *lw["src"], gsrc, dtype)
    for i in range(len(couts)):
        w, b = lw[f"s{i}"]
        _input_conditions(conv_terms(gsrc[:11], w, b)[0], False)
        worst = max(worst, _conv_op_ratio(gsrc, w, b, got[1 + i], dtype))
        assert np.array_equal(got[1 + len(couts) + i], C.max_pool_same(got[1 + i]))   # pool2_kernel on the slice
    x3 = dtype != "fp32"
    assert ctx.info("graph_fused_1x1") == (n_fused if x3 else 0)
    assert ctx.info("graph_fused_pools") == 0
    fam = [_G().conv_path(ctx, f"s{i}")["family"] for i in range(len(couts))]
    assert fam == (list(families) if x3 else ["f32_im2col"] * len(couts)), fam
    # src, one buffer per fused run / unfused sibling, one per pool
    assert ctx.info("graph_buffers") == 1 + (len(couts) - (n_fused if x3 else 0)) + len(couts)
    monkeypatch.setenv("MP_GRAPH_FUSE_1X1", "0")
    ctx0, got0 = run()
    assert ctx0.info("graph_fused_1x1") == 0
    assert all(_G().conv_path(ctx0, f"s{i}")["family"] != "sibling" for i in range(len(couts)))
    for a, b0 in zip(got, got0):
        assert np.array_equal(a, b0)
    _report(case, dtype, worst)


# ------------------------------------------------------------------------------ pool2_kernel
@pytest.mark.parametrize("avg", [False, True], ids=["max", "avg"])
@pytest.mark.parametrize("H,W,Cc", C.POOL_MAPS)
def test_pool_from_graph_input(H, W, Cc, avg):
    """Signed input straight from the graph input: padding never wins a max, an odd edge divides
    by the in-image count."""
    g = _G().GraphRecorder(H, W, Cc)
    p = g.pool(g.input, avg=avg)
    x = C._rng(f"pool{H}x{W}").standard_normal((11, H, W, Cc)).astype(np.float32)
    x[0] = -np.abs(x[0]) - 1.0                       # an all-negative image: zero padding would win
    assert (x < 0).mean() > 0.25
    ctx = make_ctx(g, [p], {}, "fp32_split")
    for n in (1, 11):
        got, = forward(ctx, [p], x[:n])
        if avg:
            want = C.avg_pool_same(x[:n].astype(np.float64))
            bnd = 4 * U * C.avg_pool_same(np.abs(x[:n]).astype(np.float64))   # = 4u sum|x| / count
            _report(f"avgpool {H}x{W}x{Cc} n={n}", "fp32", ratio(got, want, bnd))
        else:
            assert np.array_equal(got, C.max_pool_same(x[:n]))


@pytest.mark.parametrize("avg", [False, True], ids=["max", "avg"])
def test_pool_between_concat_slices(avg):
    """8x8x16 read from channels [8, 24) of one concat group and written to channels [8, 24) of
    another (pcix = 8, pld = 24, pcoff = 8, pldo = 24)."""
    g = _G().GraphRecorder(8, 8, 4)
    c1 = g.conv(g.input, 4, 8, "c1")
    c2 = g.conv(g.input, 4, 16, "c2")
    cat1 = g.concat([c1, c2])
    q, p = g.pool(c1, avg=avg), g.pool(c2, avg=avg)
    cat2 = g.concat([q, p])
    x = C._rng("poolslice").standard_normal((5, 8, 8, 4)).astype(np.float32)
    wts = {**layer_w("c1", *layer_weights("poolslice/c1", (3, 3, 4, 8))),
           **layer_w("c2", *layer_weights("poolslice/c2", (3, 3, 4, 16)))}
    ctx = make_ctx(g, [cat1, cat2], wts, "fp32_split")
    g1, g2 = forward(ctx, [cat1, cat2], x)
    assert (g1.reshape(-1, 24) > 0).any(0).all()     # every channel live
    if avg:
        want = C.avg_pool_same(g1.astype(np.float64))
        _report("avgpool slice", "fp32", ratio(g2, want, 4 * U * want + 1e-300))   # x >= 0: sum|x| / count = want
    else:
        assert np.array_equal(g2, C.max_pool_same(g1))
    assert ctx.info("graph_buffers") == 2
    with pytest.raises(C.pkg()._lib.MonkeyPoseError, match="no conv layer"):
        ctx.info("graph_path:c3")


# --------------------------------------------------------------------------------------- FC
@pytest.mark.parametrize("dtype", ["fp32_split", "fp32", "bf16"])
@pytest.mark.parametrize("K", C.FC_K)
def test_fc(K, dtype):
    """Every K class at every M block count (1, 2, 4 row blocks, and two tiles), every N, relu
    folded and not, a rank-2 concat of two FC outputs; a row alone is the same bits as inside
    M = 130."""
    g, outs, heads = _fc_graph(K)
    assert set(n for n, _ in heads.values()) >= (set(C.FC_N) if K < 32768 else {8})
    assert {nm: n for nm, (n, _) in heads.items()} == C.fc_heads(K)
    x, lw = C.fc_inputs(K, C.fc_heads(K))
    wts = {}
    for nm, (w, b) in lw.items():
        wts.update(layer_w(nm, w, b))
    ctx = make_ctx(g, outs, wts, dtype)
    kind = dtype if (dtype == "fp32" or K % 32 == 0) else "fp32"   # K % 32 != 0: the fp32 kernel
    x64 = x.reshape(len(x), K).astype(np.float64)
    want, bnd = {}, {}
    for nm, (w, b) in lw.items():
        w64, b64 = w.astype(np.float64), b.astype(np.float64)
        pre = C.fc_ref(x64, w64, b64)
        S = np.abs(x64) @ np.abs(w64) + np.abs(b64)
        A = 2.0 ** -25 * np.abs(w64).sum(0)
        assert (pre > 0).mean() >= 0.25
        want[nm] = np.maximum(pre, 0) if heads[nm][1] else pre
        bnd[nm] = bound(kind, K, S, A)
    order = ["f8"] if K == 32768 else ["f5", "f8", "f32r", "f32", "f69", "f130r", "f130"]
    worst, rows = 0.0, {}
    for M in C.FC_M:
        got = forward(ctx, outs, x[:M])
        if K != 32768:   # split the rank-2 concat back into its heads
            assert got[0].shape == (M, 13)
            got = [got[0][:, :5], got[0][:, 5:]] + got[1:]
        rows[M] = [a[0].copy() for a in got]
        for nm, a in zip(order, got):
            worst = max(worst, ratio(a, want[nm][:M], bnd[nm][:M]))
    for a, b1 in zip(rows[1], rows[130]):
        assert np.array_equal(a, b1)
    _report(f"fc K={K}", dtype, worst)


# ------------------------------------------------------------------- dispatch switches (children)
@pytest.mark.parametrize("var", sorted(C.SWITCH_ROWS))
def test_switch_moves_the_path_and_keeps_the_bound(var):
    """The switches are cached in statics, so each setting runs in one child process: the rows
    whose kernel the switch changes, under the same per-element gate; the child reports the path
    the library took, which must differ from the row's default path."""
    rows = C.SWITCH_ROWS[var]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "graph_op_cases.py"), ",".join(rows), "fp32_split"],
                       env={**os.environ, var: "0"}, capture_output=True, text=True, timeout=110)
    assert r.returncode == 0, r.stderr[-2000:]
    res = [json.loads(l) for l in r.stdout.strip().splitlines() if l.startswith("{")]
    assert [d["row"] for d in res] == rows
    for d in res:
        default = C.CONV_BY_NAME[d["row"]].expected("fp32_split")
        print(f"{var}=0 {d['row']}: {d['path']} err/bound {d['ratio']:.4f}")
        assert {k: d["path"][k] for k in default} != default, d
        assert d["ratio"] <= 1.0, d
