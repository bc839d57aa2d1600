"""Case tables, float64 references and error bounds for the per-op tests of the layer-graph
runtime (tests/test_gpu_graph_ops.py on the GPU, tests/test_graph_op_cases_cpu.py without one, and
the child processes that re-run rows under a dispatch switch: ``python graph_op_cases.py ROWS``).

Every conv row names the kernel the library is expected to pick for it under the f16-split dtypes
(``path``, the fields of ``_graph.decode_path``); the library's own ``graph_path:<scope>`` decides.

Inputs of a conv row, one array: ``n_dense`` standard-normal images first, then impulse images
(all zero but one +1.0 or -1.0 at (y, x, ci): conv_layer applies relu, so either sign alone would
hide half of the taps).  Where H*W*Cin <= 1024 the impulses are the whole basis; else the corners,
edge midpoints and centre at channels {0, 3, 4, 15, 16, 31, 32, Cin-1}.

Bounds (per element, u = 2^-24, S = sum_k |w_k x_k| + |b|, A = 2^-25 sum_k |w_k|, all in float64
from the float32 inputs):
  fp32_split  (3K + 16) u S + A      f16 hi+lo operands exact to 2^-22, activation lo subnormal
                                     below ~2^-3 (A), dropped lo*lo, fp32 accumulation of 3K products
  fp32        (K + 8) u S            exact-fp32 MFMA, worst-case accumulation
  bf16        (1.01 2^-10 + (K + 16) u) S + A     hi x hi only: two 2^-11 operand roundings
  conv1       (9 + 2) u S            the fused 1-channel conv + pool kernels: fp32 FMAs under every dtype
A pooled output's bound is the largest bound in its window.
"""
import functools
import json
import os
import sys
import zlib
from dataclasses import dataclass, field
from typing import Dict, Tuple

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle.hgru_ref import avg_pool_same, conv2d_same, fc as fc_ref, max_pool_same  # noqa: E402

U = 2.0 ** -24
BASE_N = (1, 3, 11)
IMPULSE_CH = (0, 3, 4, 15, 16, 31, 32)


def bound(kind: str, K: int, S, A):
    if kind == "fp32_split":
        return (3 * K + 16) * U * S + A
    if kind == "fp32":
        return (K + 8) * U * S
    if kind == "bf16":
        return (1.01 * 2.0 ** -10 + (K + 16) * U) * S + A
    if kind == "conv1":
        return (9 + 2) * U * S
    raise ValueError(kind)


@dataclass(frozen=True)
class ConvCase:
    name: str
    H: int
    W: int
    cin: int
    cout: int
    k: int = 3
    stride: int = 1
    pool: bool = False
    path: Tuple = ()            # expected graph_path fields under the f16-split dtypes, as items
    bf16: bool = False          # also run at bf16
    extra_n: Tuple = ()         # batch sizes besides 1, 3, 11
    edge: str = ""

    @property
    def K(self):
        return self.k * self.k * self.cin

    def expected(self, dtype: str) -> Dict[str, int]:
        if dtype == "fp32":   # exact fp32 im2col, pools never fused
            n32 = (self.cout + 31) // 32
            return dict(family="f32_im2col", nb=4 if n32 >= 4 else 2 if n32 >= 2 else 1, pool=0, splits=1)
        d = dict(pool=0, splits=1)
        d.update(dict(self.path))
        return d


def _c(name, H, W, cin, cout, k=3, stride=1, pool=False, bf16=False, extra_n=(), edge="", **path):
    path = {("pool" if k == "pool_" else k): v for k, v in path.items()}   # `pool_`: apart from the row's own flag
    return ConvCase(name, H, W, cin, cout, k, stride, pool, tuple(sorted(path.items())), bf16, tuple(extra_n), edge)


def _halo(wr, ch, ks=3, pool=0):
    return dict(family="halo", wr=wr, ch=ch, ks=ks, pool_=pool)


CONV_CASES = [
    _c("x3_5x7_3to23", 5, 7, 3, 23, family="x3", nb=1, edge="scalar gather, scalar epilogue, odd map"),
    _c("x3_6x6_4to64_s2", 6, 6, 4, 64, stride=2, family="x3", nb=2, edge="stride-2 SAME: pad 0 before, 1 after"),
    _c("x3_5x5_196to64_k1", 5, 5, 196, 64, k=1, family="x3", nb=2, edge="1x1 with K > 192"),
    _c("x3_8x8_20to32", 8, 8, 20, 32, family="x3", nb=1, edge="Cin padding rejected by the 4/3 rule"),
    _c("x3w_7x5_36to96", 7, 5, 36, 96, bf16=True, family="x3w", edge="128 % W != 0"),
    _c("x3w_7x5_8to200_s2", 7, 5, 8, 200, stride=2, family="x3w", edge="two 128-channel tiles, 72-channel tail"),
    _c("x3wsk_4x4_68to96", 4, 4, 68, 96, family="x3w_splitk", splits=2, edge="igemm_split_reduce_kernel"),
    _c("x3wsk_4x4_512to96_k1", 4, 4, 512, 96, k=1, family="x3w_splitk", splits=2),
    _c("pm_2x2_32to96", 2, 2, 32, 96, bf16=True, extra_n=(130,), family="pm", edge="position-major, N = 3 and 130"),
    _c("pmsk_4x4_64to96_k5", 4, 4, 64, 96, k=5, family="pm_splitk", splits=2),
    _c("pmsk_4x4_256to96_k5_pool", 4, 4, 256, 96, k=5, pool=True, bf16=True, family="pm_splitk", splits=8, pool_=1,
       edge="pooled reduce"),
    _c("pmsk_2x2_64to96_pool", 2, 2, 64, 96, pool=True, family="pm_splitk", splits=2, pool_=1, edge="1x1 pooled map"),
    _c("halo_8x8_12to12", 8, 8, 12, 12, **_halo(8, 16), edge="Cin 12 padded to 16"),
    _c("halo_8x8_16to32", 8, 8, 16, 32, **_halo(8, 16), edge="one 16-channel chunk"),
    _c("halo_8x8_48to32", 8, 8, 48, 32, **_halo(8, 16), edge="three 16-channel chunks"),
    _c("halo_8x8_32to32", 8, 8, 32, 32, bf16=True, **_halo(8, 32)),
    _c("halo_8x8_24to48", 8, 8, 24, 48, **_halo(4, 32), edge="Cin 24 padded to 32"),
    _c("halo5_8x8_40to64", 8, 8, 40, 64, k=5, bf16=True, **_halo(4, 16, ks=5)),
    _c("tall_8x16_32to96_pool", 8, 16, 32, 96, pool=True, bf16=True, **_halo(1, 32, pool=1), edge="NI = 1, W <= 16"),
    _c("tall_8x8_32to96_pool", 8, 8, 32, 96, pool=True, **_halo(1, 32, pool=1), edge="NI = 2, N = 3: partial tile"),
    _c("tall_4x4_32to128_pool", 4, 4, 32, 128, pool=True, extra_n=(5,), **_halo(1, 32, pool=1),
       edge="NI = 8, PH * 8 at the 2304-item limit"),
    _c("tall_4x32_32to96_pool", 4, 32, 32, 96, pool=True, **_halo(1, 32, pool=1), edge="W = 32 branch"),
    _c("tall_2x64_32to96_pool", 2, 64, 32, 96, pool=True, **_halo(1, 32, pool=1), edge="W = 64 in-wave branch"),
    _c("x3_8x8_64to64_k5", 8, 8, 64, 64, k=5, family="x3", nb=2, edge="halo refused: LDS 82,944 B > 80 KiB"),
    _c("pw_5x5_8to16", 5, 5, 8, 16, k=1, bf16=True, family="pw", nch=1),
    _c("pwn_5x5_32to64", 5, 5, 32, 64, k=1, bf16=True, family="pwn", nch=1, nb=2),
    _c("pwn_5x5_64to96", 5, 5, 64, 96, k=1, bf16=True, family="pwn", nch=2, nb=3),
    _c("pwn_5x5_72to96", 5, 5, 72, 96, k=1, bf16=True, family="pwn", nch=3, nb=3),
    _c("pwn_5x5_100to128", 5, 5, 100, 128, k=1, bf16=True, family="pwn", nch=4, nb=4),
    _c("pwn_5x5_128to160", 5, 5, 128, 160, k=1, bf16=True, family="pwn", nch=4, nb=5),
    _c("pwn_5x5_192to192", 5, 5, 192, 192, k=1, bf16=True, family="pwn", nch=6, nb=6),
    _c("pw_5x5_96to160", 5, 5, 96, 160, k=1, bf16=True, family="pw", nch=3),
    _c("pw_5x5_160to256", 5, 5, 160, 256, k=1, bf16=True, family="pw", nch=5),
]
CONV_BY_NAME = {c.name: c for c in CONV_CASES}

# fused 1-channel conv + relu + 2x2 max pool (planner); `form`: how the graph is built
CONV1_SIZES = ((2, 2), (6, 10), (34, 66))
CONV1_CASES = (
    # (name, cout, form, expected family or None = unfused)
    ("bn64", 64, "plain", "conv1_pool_bn"),
    ("any64_concat", 64, "concat", "conv1_pool_any"),
    ("any12", 12, "plain", "conv1_pool_any"),
    ("any4", 4, "plain", "conv1_pool_any"),
    ("unfused68", 68, "plain", None),
    ("unfused6", 6, "plain", None),
    ("unfused_oddH", 12, "oddH", None),
    ("unfused_2consumers", 12, "second_consumer", None),
)

# 1x1 siblings of one source: (name, source channels, couts, fused count, families of the siblings)
SIBLING_CASES = (
    ("sib_24_40_10", 32, (24, 40, 10), 2, ("pwn", "sibling", "sibling")),
    ("sib_128_96_64", 32, (128, 96, 64), 1, ("pw", "sibling", "pwn")),
    ("sib_src196", 196, (24, 40, 10), 0, ("x3", "x3", "x3")),
)

# rows whose path a dispatch switch changes (tests/test_gpu_graph_ops.py runs each in one child)
SWITCH_ROWS = {
    "MP_IGEMM_HALO_TALL": [c.name for c in CONV_CASES if dict(c.path).get("wr") == 1],
    "MP_IGEMM_HALO": [c.name for c in CONV_CASES if dict(c.path)["family"] == "halo"],
    "MP_IGEMM_PW": [c.name for c in CONV_CASES if dict(c.path)["family"] in ("pw", "pwn")],
    "MP_IGEMM_TAPSKIP": [c.name for c in CONV_CASES if dict(c.path)["family"] in ("pm", "pm_splitk")],
    "MP_IGEMM_HALO_NARROW1": [c.name for c in CONV_CASES if dict(c.path).get("wr") == 8],
}

FC_K = (32, 40, 96, 160, 2112, 32768)
FC_M = (1, 33, 65, 130)
FC_N = (5, 32, 69, 130)

# pool2_kernel maps fed from the graph input: (H, W, C)
POOL_MAPS = ((5, 7, 6), (1, 1, 4))


def _rng(name: str):
    return np.random.default_rng(zlib.crc32(name.encode()))


def impulse_sites(H, W, cin):
    """(y, x, ci) of the impulse images of an H x W x cin input."""
    if H * W * cin <= 1024:
        return [(y, x, c) for y in range(H) for x in range(W) for c in range(cin)]
    ys, xs = sorted({0, H // 2, H - 1}), sorted({0, W // 2, W - 1})
    cs = sorted({c for c in IMPULSE_CH + (cin - 1,) if 0 <= c < cin})
    return [(y, x, c) for y in ys for x in xs for c in cs]


def conv_inputs(name, H, W, cin, n_dense):
    """float32 [n_dense + 2 * sites, H, W, cin]: dense images, then +1 and -1 impulses per site."""
    sites = impulse_sites(H, W, cin)
    x = np.zeros((n_dense + 2 * len(sites), H, W, cin), np.float32)
    x[:n_dense] = _rng(name + "/x").standard_normal((n_dense, H, W, cin))
    for i, (y, xx, c) in enumerate(sites):
        x[n_dense + 2 * i, y, xx, c] = 1.0
        x[n_dense + 2 * i + 1, y, xx, c] = -1.0
    return x


def layer_weights(name, shape):
    """Weights ~ N(0, 1/K), biases ~ 0.1 N(0, 1), float32; shape HWIO (conv) or [K, N] (fc)."""
    K = int(np.prod(shape[:-1]))
    r = _rng(name + "/w")
    return ((r.standard_normal(shape) / np.sqrt(K)).astype(np.float32),
            (0.1 * r.standard_normal(shape[-1])).astype(np.float32))


def conv_terms(x, w, b, stride=1):
    """float64 pre-activation conv + bias, S and A of the bound, from float32 inputs."""
    x64, w64, b64 = np.asarray(x, np.float64), np.asarray(w, np.float64), np.asarray(b, np.float64)
    pre = conv2d_same(x64, w64, stride) + b64
    S = conv2d_same(np.abs(x64), np.abs(w64), stride) + np.abs(b64)
    A = 2.0 ** -25 * np.abs(w64).reshape(-1, w64.shape[-1]).sum(0)
    return pre, S, A


def pool_windows(v, fill):
    """[n, Ho, Wo, 4, C]: the 2x2 window elements of every pooled position (`fill` outside)."""
    n, h, w, c = v.shape
    p = np.full((n, h + h % 2, w + w % 2, c), fill, v.dtype)
    p[:, :h, :w] = v
    return np.stack([p[:, dy::2, dx::2] for dy in (0, 1) for dx in (0, 1)], 3)


def conv_expected(pre, S, A, kind, K, pool):
    """(expected output, per-element bound) of relu(conv) [+ 2x2 max pool]."""
    want, bnd = np.maximum(pre, 0), bound(kind, K, S, A) + 0 * pre
    if pool:
        want, bnd = max_pool_same(want), pool_windows(bnd, 0.0).max(3)
    return want, bnd


def ratio(got, want, bnd):
    """max |got - want| / bound over every element; inf where got is not finite, or differs from
    want under a zero bound (an all-zero image through a bias-free layer)."""
    got = np.asarray(got, np.float64)
    assert got.shape == want.shape == bnd.shape, (got.shape, want.shape, bnd.shape)
    err = np.abs(got - want)
    r = np.where(err == 0, 0.0, err / np.where(bnd > 0, bnd, 1.0))
    r[~np.isfinite(got) | ((bnd <= 0) & (err > 0))] = np.inf
    return float(r.max())


def dense_positive_fraction(pre_dense):
    return float((pre_dense > 0).mean())


def pool_winners(pre_dense):
    """the distinct window positions (0..3) that win the max somewhere in relu(pre)"""
    win = pool_windows(np.maximum(pre_dense, 0), -np.inf)
    top = win.max(3, keepdims=True)
    strict = (win == top) & ((win == top).sum(3, keepdims=True) == 1) & (top > 0)
    return sorted(set(np.nonzero(strict)[3].tolist()))


@dataclass
class ConvRef:
    x: np.ndarray
    w: np.ndarray
    b: np.ndarray
    n_dense: int
    pre: np.ndarray
    S: np.ndarray
    A: np.ndarray
    extra: dict = field(default_factory=dict)


@functools.lru_cache(maxsize=None)
def conv_reference(name) -> ConvRef:
    """Inputs, weights and float64 terms of a CONV_CASES row; computed once, never modified."""
    c = CONV_BY_NAME[name]
    n_dense = max(BASE_N + c.extra_n)
    x = conv_inputs(name, c.H, c.W, c.cin, n_dense)
    w, b = layer_weights(name, (c.k, c.k, c.cin, c.cout))
    pre, S, A = conv_terms(x, w, b, c.stride)
    for a in (x, w, b, pre, S, A):
        a.setflags(write=False)
    return ConvRef(x, w, b, n_dense, pre, S, A)


def conv1_case(case, hw):
    """(cout, form, family, H, W, x, w, b) of a CONV1_CASES row at one of CONV1_SIZES."""
    _, cout, form, family = next(c for c in CONV1_CASES if c[0] == case)
    H, W = (5, 10) if form == "oddH" else hw
    name = f"conv1_{case}_{H}x{W}"
    w, b = layer_weights(name, (3, 3, 1, cout))
    return cout, form, family, H, W, conv_inputs(name, H, W, 1, max(BASE_N)), w, b


def conv1_params():
    return [(nm, hw) for nm, _, _, fam in CONV1_CASES for hw in (CONV1_SIZES if fam else CONV1_SIZES[1:2])]


def fc_inputs(K, heads):
    """x [max M, 1, 1, K] signed, and {head: (w, b)} for {head: N}."""
    x = _rng(f"fc{K}").standard_normal((max(FC_M), 1, 1, K)).astype(np.float32)
    return x, {nm: layer_weights(f"fc{K}/{nm}", (K, n)) for nm, n in heads.items()}


FC_HEADS = {"f5": 5, "f8": 8, "f32r": 32, "f32": 32, "f69": 69, "f130r": 130, "f130": 130}   # r: relu folded


def fc_heads(K):
    return {"f8": 8} if K == 32768 else dict(FC_HEADS)


def conv_batches(c: ConvCase, ref: ConvRef):
    return sorted(set(BASE_N + c.extra_n)) + [len(ref.x)]


def conv_bound_kind(dtype, family):
    return "conv1" if family.startswith("conv1_pool") else dtype


# ---- naive references (the CPU tests compare the oracle's GEMM forms with these) ----
def naive_conv(x, w, stride):
    n, H, W, cin = x.shape
    k = w.shape[0]
    Ho, Wo = -(-H // stride), -(-W // stride)
    pt = max((Ho - 1) * stride + k - H, 0) // 2
    pl = max((Wo - 1) * stride + k - W, 0) // 2
    out = np.zeros((n, Ho, Wo, w.shape[3]))
    for i in range(n):
        for oy in range(Ho):
            for ox in range(Wo):
                for ky in range(k):
                    for kx in range(k):
                        iy, ix = oy * stride - pt + ky, ox * stride - pl + kx
                        if 0 <= iy < H and 0 <= ix < W:
                            for ci in range(cin):
                                out[i, oy, ox] += x[i, iy, ix, ci] * w[ky, kx, ci]
    return out


def naive_pool(x, avg):
    n, H, W, C = x.shape
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    out = np.zeros((n, Ho, Wo, C))
    for i in range(n):
        for oy in range(Ho):
            for ox in range(Wo):
                for c in range(C):
                    v = [x[i, iy, ix, c] for iy in (2 * oy, 2 * oy + 1) for ix in (2 * ox, 2 * ox + 1)
                         if iy < H and ix < W]
                    out[i, oy, ox, c] = sum(v) / len(v) if avg else max(v)
    return out


# ---- running a recorded graph on the GPU ----
def pkg():
    import importlib
    return importlib.import_module("monkey-pose_amd")


def make_ctx(g, outs, wts, dtype):
    mp = pkg()
    ctx = mp._lib.Context(mp._lib.MP_MODEL_GRAPH, 0)
    mp._graph.install(ctx, g, outs)
    for k, v in wts.items():
        ctx.set_weight(k, np.asarray(v, np.float32))
    ctx.finalize(mp._lib.dtype_code(dtype))
    return ctx


def forward(ctx, outs, x):
    """Run the context's graph on x; the outputs as numpy (buffers pre-filled with NaN)."""
    import torch
    L = pkg()._lib
    xt = torch.from_numpy(np.array(x, np.float32)).cuda()   # a copy: the shared references are read-only
    bufs = [torch.full((xt.shape[0],) + tuple(s.shape), float("nan"), device="cuda") for s in outs]
    ctx.graph_fwd(xt, bufs, L.current_stream())
    torch.cuda.synchronize()
    return [b.cpu().numpy() for b in bufs]


def layer_w(name, w, b):
    return {f"{name}/{name}_filters" if w.ndim == 4 else f"{name}/{name}_weights": w, f"{name}/{name}_biases": b}


def conv_graph(c: ConvCase):
    G = pkg()._graph
    g = G.GraphRecorder(c.H, c.W, c.cin)
    y = g.conv(g.input, c.cin, c.cout, "c", k=c.k, stride=c.stride)
    return g, [g.pool(y) if c.pool else y]


def sibling_graph(cs, couts, H=5, W=5):
    """(recorder, source, siblings, their pools): an 8 -> cs 1x1 source conv and its 1x1 siblings"""
    G = pkg()._graph
    g = G.GraphRecorder(H, W, 8)
    src = g.conv(g.input, 8, cs, "src", k=1)
    sibs = [g.conv(src, cs, co, f"s{i}", k=1) for i, co in enumerate(couts)]
    pools = [g.pool(s) for s in sibs]                 # each consumer reads its slice in place
    return g, src, sibs, pools


def fc_graph(K):
    """(recorder, outputs, {head: (N, relu folded)}): every FC head of FC_HEADS on one K-wide input"""
    G = pkg()._graph
    g = G.GraphRecorder(1, 1, K)
    if K == 32768:
        return g, [g.fc(g.input, K, 8, "f8")], {"f8": (8, False)}
    f5, f8 = g.fc(g.input, K, 5, "f5"), g.fc(g.input, K, 8, "f8")
    cat = g.concat([f5, f8])                                   # rank-2: ldo = 13, coff = 5
    f32r = g.relu(g.fc(g.input, K, 32, "f32r"))
    f32 = g.fc(g.input, K, 32, "f32")
    f69 = g.fc(g.input, K, 69, "f69")
    f130r = g.relu(g.fc(g.input, K, 130, "f130r"))
    f130 = g.fc(g.input, K, 130, "f130")
    return g, [cat, f32r, f32, f69, f130r, f130], {"f5": (5, False), "f8": (8, False), "f32r": (32, True),
                                                   "f32": (32, False), "f69": (69, False), "f130r": (130, True),
                                                   "f130": (130, False)}


def run_conv_case(name, dtype):
    """One CONV_CASES row at one dtype, at every batch size: (reported path, fused pools,
    max err / bound)."""
    c, ref = CONV_BY_NAME[name], conv_reference(name)
    g, outs = conv_graph(c)
    ctx = make_ctx(g, outs, layer_w("c", ref.w, ref.b), dtype)
    worst, path = 0.0, None
    for n in conv_batches(c, ref):
        got, = forward(ctx, outs, ref.x[:n])
        p = pkg()._graph.conv_path(ctx, "c")
        assert path is None or p == path, (n, p, path)   # a property of the layer, never of the batch
        path = p
        want, bnd = conv_expected(ref.pre[:n], ref.S[:n], ref.A, conv_bound_kind(dtype, p["family"]), c.K, c.pool)
        worst = max(worst, ratio(got, want, bnd))
    return path, ctx.info("graph_fused_pools"), worst


if __name__ == "__main__":   # child of a dispatch-switch test: rows, comma separated, and the dtype
    for row in sys.argv[1].split(","):
        path, fused, worst = run_conv_case(row, sys.argv[2])
        print(json.dumps(dict(row=row, path=path, fused_pools=fused, ratio=worst)), flush=True)
