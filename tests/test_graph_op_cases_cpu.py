"""The tables and references behind tests/test_gpu_graph_ops.py, checked without a GPU: the float64
reference equals a naive loop nest on every map geometry of the tables, every case's inputs can
show the faults it is meant to catch, and the tables name every kernel family of the header's
path enum."""
import os
import re

import numpy as np
import pytest

import graph_op_cases as C
from oracle.hgru_ref import avg_pool_same, conv2d_same, max_pool_same

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _geometries():
    geo = {(c.H, c.W, c.k, c.stride) for c in C.CONV_CASES}
    geo |= {(h, w, 3, 1) for h, w in C.CONV1_SIZES} | {(5, 10, 3, 1), (5, 5, 1, 1), (8, 8, 3, 1)}
    return sorted(geo)


@pytest.mark.parametrize("H,W,k,stride", _geometries())
def test_conv_reference_is_the_naive_loop_nest(H, W, k, stride):
    r = np.random.default_rng(H * 1000 + W * 10 + k + stride)
    x, w = r.standard_normal((2, H, W, 3)), r.standard_normal((k, k, 3, 2))
    got, want = conv2d_same(x, w, stride), C.naive_conv(x, w, stride)
    assert got.shape == want.shape == (2, -(-H // stride), -(-W // stride), 2)
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-13)


def _pool_maps():
    maps = {(h, w) for h, w, _ in C.POOL_MAPS} | {(8, 8), (5, 5)}
    maps |= {(-(-c.H // c.stride), -(-c.W // c.stride)) for c in C.CONV_CASES if c.pool}
    maps |= set(C.CONV1_SIZES) | {(5, 10)}
    return sorted(maps)


@pytest.mark.parametrize("H,W", _pool_maps())
def test_pool_reference_is_the_naive_loop_nest(H, W):
    x = np.random.default_rng(H * 100 + W).standard_normal((2, H, W, 3))
    x[0] = -np.abs(x[0]) - 1                      # padding must not win, the divisor counts in-image
    assert np.array_equal(max_pool_same(x), C.naive_pool(x, False))
    np.testing.assert_allclose(avg_pool_same(x), C.naive_pool(x, True), rtol=0, atol=1e-15)
    assert np.array_equal(C.pool_windows(x, -np.inf).max(3), max_pool_same(x))


@pytest.mark.parametrize("name", [c.name for c in C.CONV_CASES])
def test_conv_case_inputs_can_show_the_faults(name):
    c, ref = C.CONV_BY_NAME[name], C.conv_reference(name)
    dense = ref.pre[:ref.n_dense]
    assert ref.n_dense == max(C.BASE_N + c.extra_n) and set(C.BASE_N) <= set(C.conv_batches(c, ref))
    assert C.dense_positive_fraction(dense) >= 0.25
    if c.pool:
        assert c.H % 2 == 0 and c.W % 2 == 0
        assert len(C.pool_winners(dense)) >= 2
    # impulses: one non-zero per image, both signs, the whole basis on small inputs
    imp = ref.x[ref.n_dense:]
    sites = C.impulse_sites(c.H, c.W, c.cin)
    assert len(imp) == 2 * len(sites) and (np.count_nonzero(imp.reshape(len(imp), -1), axis=1) == 1).all()
    assert (imp.reshape(len(imp), -1).sum(1) == np.tile([1.0, -1.0], len(sites))).all()
    if c.H * c.W * c.cin <= 1024:
        assert len(sites) == c.H * c.W * c.cin
    else:
        pos = {(y, x) for y, x, _ in sites}
        assert {(0, 0), (0, c.W - 1), (c.H - 1, 0), (c.H - 1, c.W - 1), (c.H // 2, c.W // 2)} <= pos
        assert {ch for _, _, ch in sites} == {ch for ch in (0, 3, 4, 15, 16, 31, 32, c.cin - 1) if ch < c.cin}
    # on an impulse image S is one |w| + |b| (or |b| alone): a misplaced tap fails by orders of magnitude
    y, x, ci = sites[-1]
    S_imp, absb = ref.S[-1], np.abs(ref.b.astype(np.float64))
    assert (S_imp >= absb).all() and (S_imp <= np.abs(ref.w[:, :, ci].astype(np.float64)).max((0, 1)) + absb + 1e-12).all()
    for kind in ("fp32_split", "fp32", "bf16"):
        assert (C.bound(kind, c.K, ref.S, ref.A) > 0).all()


@pytest.mark.parametrize("name", [c.name for c in C.CONV_CASES])
def test_a_dropped_tap_breaks_the_bound_on_its_impulse(name):
    """The net is fine enough: an output computed without one tap of the filter misses every
    dtype's bound on the impulse image that excites the tap, by orders of magnitude -- at K = 6400
    too, where a dense image would hide it."""
    c, ref = C.CONV_BY_NAME[name], C.conv_reference(name)
    sites = C.impulse_sites(c.H, c.W, c.cin)
    i = max(range(len(sites)), key=lambda j: (sites[j][:2] == (c.H // 2, c.W // 2), sites[j][2]))   # the centre
    ci = sites[i][2]
    imp = ref.x[ref.n_dense + 2 * i:ref.n_dense + 2 * i + 2].astype(np.float64)
    pre, S = ref.pre[ref.n_dense + 2 * i:][:2], ref.S[ref.n_dense + 2 * i:][:2]
    right = np.maximum(pre, 0)
    for flat in np.argsort(-np.abs(ref.w[:, :, ci]).ravel()):   # the largest tap that the site reaches
        ky, kx, co = np.unravel_index(flat, (c.k, c.k, c.cout))
        w = ref.w.astype(np.float64).copy()
        w[ky, kx, ci, co] = 0.0
        wrong = np.maximum(conv2d_same(imp, w, c.stride) + ref.b.astype(np.float64), 0)
        if (wrong != right).any():
            break
    assert (wrong != right).any()
    for kind in ("fp32_split", "fp32", "bf16"):
        want, bnd = C.conv_expected(pre, S, ref.A, kind, c.K, c.pool)
        got = C.max_pool_same(wrong) if c.pool else wrong
        assert C.ratio(got, want, bnd) > 10, kind
        assert C.ratio(want, want, bnd) == 0.0


@pytest.mark.parametrize("case,hw", C.conv1_params(), ids=[f"{n}-{h}x{w}" for n, (h, w) in C.conv1_params()])
def test_conv1_case_inputs_can_show_the_faults(case, hw):
    cout, form, family, H, W, x, w, b = C.conv1_case(case, hw)
    pre = C.conv_terms(x[:11], w, b)[0]
    assert C.dense_positive_fraction(pre) >= 0.25 and len(C.pool_winners(pre)) >= 2
    assert (family is None) == (cout % 4 != 0 or cout > 64 or H % 2 == 1 or form == "second_consumer")
    assert len(x) == 11 + 2 * len(C.impulse_sites(H, W, 1))


@pytest.mark.parametrize("K", C.FC_K)
def test_fc_case_inputs_can_show_the_faults(K):
    x, lw = C.fc_inputs(K, C.fc_heads(K))
    assert (x < 0).mean() > 0.4 and len(x) == max(C.FC_M)
    for nm, (w, b) in lw.items():
        pre = C.fc_ref(x.reshape(len(x), K).astype(np.float64), w.astype(np.float64), b.astype(np.float64))
        assert (pre > 0).mean() >= 0.25, nm


def test_fc_and_planner_tables_cover_the_issue_axes():
    assert C.FC_K == (32, 40, 96, 160, 2112, 32768) and C.FC_M == (1, 33, 65, 130) and C.FC_N == (5, 32, 69, 130)
    assert {co for _, co, _, _ in C.CONV1_CASES} >= {64, 12, 4, 68, 6}
    assert [c[2] for c in C.SIBLING_CASES] == [(24, 40, 10), (128, 96, 64), (24, 40, 10)] and C.SIBLING_CASES[2][1] == 196
    for var, rows in C.SWITCH_ROWS.items():
        assert rows, var


def _header_enum(prefix):
    with open(os.path.join(ROOT, "include", "monkeypose.h")) as f:
        return {m.group(1).lower(): int(m.group(2)) for m in re.finditer(rf"\b{prefix}(\w+) = (\d+)", f.read())}


def test_tables_name_every_value_of_the_path_enum():
    G = C.pkg()._graph
    fam = _header_enum("MP_PATH_")
    assert {v: k for k, v in fam.items()} == G.PATH_FAMILIES
    layouts = _header_enum("MP_HALO_")
    assert {v: k for k, v in layouts.items()} == G.HALO_LAYOUTS
    named = {dict(c.path)["family"] for c in C.CONV_CASES} | {c.expected("fp32")["family"] for c in C.CONV_CASES}
    named |= {f for *_, f in C.CONV1_CASES if f} | {f for *_, fams in C.SIBLING_CASES for f in fams}
    assert named == set(fam), set(fam) ^ named
    wr = {dict(c.path)["wr"] for c in C.CONV_CASES if dict(c.path)["family"] == "halo"}
    # the WIDE layout (WR = 2) exists only under MP_IGEMM_HALO_TALL=0: a switch row reaches it
    assert wr == set(layouts.values()) - {layouts["wide"]} and C.SWITCH_ROWS["MP_IGEMM_HALO_TALL"]
    # im2col NB: 1 and 2 on the f16-split kernel (4 needs Cout > 64, which the wide kernels take), all three on fp32
    assert {dict(c.path)["nb"] for c in C.CONV_CASES if dict(c.path)["family"] == "x3"} == {1, 2}
    assert {c.expected("fp32")["nb"] for c in C.CONV_CASES} == {1, 2, 4}
    assert {(dict(c.path)["nch"], dict(c.path)["nb"]) for c in C.CONV_CASES if dict(c.path)["family"] == "pwn"} == \
        {(1, 2), (2, 3), (3, 3), (4, 4), (4, 5), (6, 6)}
    assert {dict(c.path)["nch"] for c in C.CONV_CASES if dict(c.path)["family"] in ("pw", "pwn")} == {1, 2, 3, 4, 5, 6}
    # decode_path inverts the documented bit layout
    word = 7 | 1 << 8 | 8 << 12 | 4 << 20 | 16 << 24 | 5 << 32 | 3 << 36 | 6 << 40
    assert G.decode_path(word) == dict(family="halo", pool=1, splits=8, wr=4, ch=16, ks=5, nch=3, nb=6)
