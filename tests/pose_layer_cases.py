"""Case tables, float64 references, split-precision models and gates for the per-layer tests of the
pose model's backbone and head (tests/test_gpu_pose_layers.py on the GPU,
tests/test_pose_layer_cases_cpu.py without one, and the child processes that re-run rows under a
dispatch switch: ``python pose_layer_cases.py ROWS``).

Every layer is compared with float64 of that one layer applied to the GPU's own input to it (the
previous tap, read back as float32), through ``_lib.Context(MP_MODEL_HGRU_POSE)`` and
``pose_fwd_taps``.  Weights are ``weights.hgru_pose_vars(crop=(2H, 2W), timesteps=2)`` with fc_1's
width replaced where a row asks for one (the library takes it from the weight's shape,
mp_abi.hip finalize_pose).

G1, per element: |got - ref| <= bound(kind, K, S, A) of graph_op_cases.  A folded BN after the relu
multiplies the bound by |bn_s[c]| and adds 2u|ref|.  pool1 is the fused conv_1 + pool kernel (kind
conv1).  Catches a wrong halo, seam, row or column; at K = 65536 its (3K + 16)u is 1.2e-2 of S, so
it cannot see a lost product plane.

G2, per region, from the reference alone: the f16x3 split is emulated on the layer's inputs exactly as
the kernels state it, hi = f16(s v), lo = f16(s v - hi), with the library's scales:
  backbone activations  s = BB_ASCALE = 16                      (mp_abi.hip)
  conv / fc weights     s = 2^(14 - e), frexp(max|w|) = (m, e)   (mp_abi.hip pack_x3, k_fc.hip launch_pack_fc_x3)
  fc_1 activations      s = 1: the planes are split unscaled     (k_fft4.hip ROW_FINAL mode 2, k_fc.hip)
and the products hi*hi + hi_w*lo_a + lo_w*hi_a summed in float64.  Dropping hi_w*lo_a ("drop_a") or
lo_w*hi_a ("drop_w") gives the two degraded outputs; for the three-product dtypes
  rms_R(got - ref) <= (1/16) min(rms_R(drop_a - ref), rms_R(drop_w - ref))
and for bf16 (one f16 product)  rms_R(got - ref) <= 2 rms_R(hi*hi - ref).
Where the library stores the map as bf16 (conv_3's output under bf16), the reference and the models
are rounded to bf16 the same way before both gates; G1's interval [ref - bound, ref + bound] is rounded
at both ends (the bound holds for the kernel's fp32 value, and one bf16 ulp of a value that sits at a
rounding boundary is 2^-8 of it, more than the exact-fp32 bound).
"""
import dataclasses
import functools
import json
import os
import sys
from dataclasses import dataclass
from typing import Tuple

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from graph_op_cases import U, bound, conv_terms, pkg, pool_windows, ratio  # noqa: E402
from oracle.hgru_ref import conv2d_same, max_pool_same  # noqa: E402

T = 2                       # hGRU steps: the last one still writes fc_1's planes
SEED = 4321
NOUT = 69
BB_ASCALE = 16.0            # mp_abi.hip
BN_EPS = 1e-5
SENTINEL = np.float32(-1.25e30)
KIND = {"fp32": "fp32", "fp32_split": "fp32_split", "fp32_fft": "fp32_split", "bf16": "bf16"}
BACKBONE_TAPS = ("pool1", "conv2", "conv3")
HEAD_TAPS = ("fc1", "relu1")
ROW_SEAMS, COL_SEAMS = ((7, 8), (15, 16), (23, 24), (31, 32)), ((31, 32),)
FC_ROWS = (0, 31, 32, 63, 64, 127, 128, 255, 256)


@dataclass(frozen=True)
class Row:
    name: str
    H: int                  # map = crop / 2
    W: int
    width: int              # fc_1 outputs
    dtypes: Tuple[str, ...]
    ns: Tuple[int, ...]
    all_rows: bool = True   # head rows: reference on every batch row (else the listed ones)
    edge: str = ""

    @property
    def K(self):
        return self.H * self.W * 64


BACKBONE_ROWS = (
    Row("bb_32x32", 32, 32, 32, ("fp32_fft", "fp32_split", "bf16", "fp32"), (1, 3, 129),
        edge="1, 3: 8-row tiles, one 32-channel block per workgroup; 129: 32-row tiles; fp32: conv64_kernel"),
    Row("bb_64x32", 64, 32, 32, ("fp32_fft", "bf16"), (2, 65), edge="row seam 31|32 of the 32-row tiles"),
    Row("bb_32x64", 32, 64, 32, ("fp32_fft", "bf16"), (2, 65), edge="column seam 31|32"),
    Row("bb_16x32", 16, 32, 32, ("fp32_fft", "bf16"), (3,), edge="H % 32 != 0: conv64_kernel, bf16 map under bf16"),
    Row("bb_48x32", 48, 32, 32, ("fp32",), (3,), edge="three 16-row tiles"),
)
HEAD_ROWS = (
    Row("head_16x32_w1024", 16, 32, 1024, ("fp32_fft", "bf16"), (1, 33, 65, 129, 257), all_rows=False,
        edge="production slice count (N % 256 == 0); 32/64/128-row tiles, partial and one-row 256-row tiles"),
    Row("head_32x32_w160", 32, 32, 160, ("fp32_fft", "bf16", "fp32_split", "fp32"), (1, 33, 65, 130, 257),
        edge="N32 = 5: one live wave of four, five of eight, padded columns of part"),
)
ROWS = {r.name: r for r in BACKBONE_ROWS + HEAD_ROWS}


def params(rows):
    return [(r.name, d, n) for r in rows for d in r.dtypes for n in r.ns]


_DEFAULT_SWITCH = (("bb_32x32", "fp32_fft", 3), ("bb_64x32", "bf16", 65),
                   ("head_32x32_w160", "fp32_fft", 130), ("head_16x32_w1024", "bf16", 65))
# one child process per setting (the switches are cached in statics)
SWITCH_ROWS = {
    "MP_CONV_DB=0": _DEFAULT_SWITCH,
    "MP_CONV_SMALL=0": _DEFAULT_SWITCH,
    "MP_FC_BK64=0": (("bb_32x32", "bf16", 3), ("bb_64x32", "bf16", 65),
                     ("head_32x32_w160", "bf16", 130), ("head_16x32_w1024", "bf16", 65)),
    "MP_FC_PRESPLIT=0": _DEFAULT_SWITCH,
    "MP_BB_PIPE=0": _DEFAULT_SWITCH,
}


# ------------------------------------------------------------------------- the library's rules
def shape_ok(H, W, dtype):
    """mp_abi.hip pose_fwd: crop/2 % (16, 32) == 0, then check_map for the dtype."""
    if H % 16 or W % 32:
        return False
    if dtype in ("fp32_fft", "bf16"):
        return 1 <= H <= 64 and W in (32, 64)
    return H % (32 if dtype == "fp32_split" else 16) == 0


def conv_kind(dtype, H):
    """The backbone convs' bound kind: the f16 kernels need H % 32 == 0 (mp_abi.hip pose_fwd `x3`),
    else conv64_kernel's exact fp32 under every dtype."""
    return KIND[dtype] if dtype != "fp32" and H % 32 == 0 else "fp32"


def slice_ends(n):
    """Last image of each hGRU batch slice (mp_abi.hip run_circuit: two streams from 64 images on, whole
    32-image groups, the first slice the larger half)."""
    if n < 64:
        return [n - 1]
    groups = (n + 31) // 32
    return [min(n, (groups + 1) // 2 * 32) - 1, n - 1]


def ref_images(n):
    """Images the backbone reference is computed on."""
    if n < 65:
        return list(range(n))
    return sorted({0, 31, 32, 63, 64, n - 1} | set(slice_ends(n)))


def fc_ref_rows(row: Row, n):
    if row.all_rows:
        return list(range(n))
    return fc_region_rows(n)


def fc_region_rows(n):
    """0, 31, 32, 63, 64, 127, 128, 255, 256, n - 1, and t - 1, t of every row-tile start (tiles of 32,
    64, 128 or 256 rows all start at multiples of 32)."""
    r = set(FC_ROWS) | {n - 1}
    for t in range(32, n, 32):
        r |= {t - 1, t}
    return sorted(i for i in r if 0 <= i < n)


# -------------------------------------------------------------------------------- inputs
@functools.lru_cache(maxsize=2)
def pose_weights(H, W, width):
    Wt = pkg().weights
    shapes = {"cnn/fc_1/fc_1_weights": (H * W * 64, width), "cnn/fc_1/fc_1_biases": (width,),
              "cnn/fc_out/fc_out_weights": (width, NOUT)}
    out = {}
    for v in Wt.hgru_pose_vars(output_shape=NOUT, timesteps=T, crop=(2 * H, 2 * W)):
        if v.name in shapes:
            v = dataclasses.replace(v, shape=shapes[v.name])
        elif v.name.startswith("cnn/batch_normalization_4/"):
            v = dataclasses.replace(v, shape=(width,))
        out[v.name] = Wt.synth_value(v, SEED, T)
        out[v.name].setflags(write=False)
    return out


@functools.lru_cache(maxsize=4)
def _inputs_max(H, W, n):
    Wt = pkg().weights
    size = 2 * max(H, W)
    depth = np.ascontiguousarray(Wt.synth_crops(n, seed=SEED + 1, size=size)[:, :2 * H, :2 * W])
    o0 = Wt.synth_hidden((n, H, W, 64), seed=SEED + 2)
    for a in (depth, o0):
        a.setflags(write=False)
    return depth, o0


def inputs(row: Row, n):
    """(depth [n, 2H, 2W, 1], O0 [n, H, W, 64]); image i is the same at every batch size."""
    depth, o0 = _inputs_max(row.H, row.W, max(row.ns))
    return depth[:n], o0[:n]


def bn_fold(wts, scope):
    """(s, t) of inference BN as one affine, float64."""
    g, b, m, v = (wts[f"cnn/{scope}/{k}"].astype(np.float64) for k in ("gamma", "beta", "moving_mean", "moving_variance"))
    s = g / np.sqrt(v + BN_EPS)
    return s, b - m * s


# ------------------------------------------------------------------------- the split emulation
def to_bf16(v):
    """round to nearest even bf16, as float64"""
    a = np.ascontiguousarray(v, np.float32).view(np.uint32)
    r = ((a + np.uint32(0x7FFF) + ((a >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000)).view(np.float32)
    return r.astype(np.float64)


def weight_scale(w):
    mx = float(np.abs(w).max())
    return 2.0 ** (14 - np.frexp(mx)[1]) if mx > 0 else 2.0 ** 14


def f16_split(v, scale):
    """(hi, lo) of float32 v at power-of-two `scale`, unscaled again (exact), float64."""
    with np.errstate(over="raise"):
        s = np.asarray(v, np.float32) * np.float32(scale)
        hi = s.astype(np.float16).astype(np.float32)
        lo = (s - hi).astype(np.float16).astype(np.float32)
    return hi.astype(np.float64) / scale, lo.astype(np.float64) / scale


MODELS = ("drop_a", "drop_w", "hihi")


def split_models(lin, x, w, ascale, names=MODELS, wsplit=None):
    """The emulated products of lin(x, w) (bilinear), float64: `full` = hi*hi + hi_w*lo_a + lo_w*hi_a,
    `drop_a` without hi_w*lo_a, `drop_w` without lo_w*hi_a, `hihi` the one-product form, and `bf16ops`
    both operands rounded to bf16.  `wsplit`: f16_split of w where the caller keeps it."""
    ah, al = f16_split(x, ascale)
    wh, wl = wsplit or f16_split(w, weight_scale(w))
    form = {"full": lambda: lin(ah + al, wh + wl) - lin(al, wl), "drop_a": lambda: lin(ah, wh + wl),
            "drop_w": lambda: lin(ah + al, wh), "hihi": lambda: lin(ah, wh),
            "bf16ops": lambda: lin(to_bf16(x), to_bf16(w))}
    return {k: form[k]() for k in names}


# ------------------------------------------------------------------------------- layer references
@dataclass
class LayerRef:
    want: np.ndarray        # float64 expected output
    bnd: np.ndarray         # G1 bound per element
    models: dict            # degraded outputs after the same epilogue
    pre: np.ndarray         # before the relu
    lo: np.ndarray = None   # a bf16-stored map: bf16(ref - bound) and bf16(ref + bound)
    hi: np.ndarray = None


def pool1_ref(depth, wts):
    """BN_0(maxpool(relu(conv_1))) of float32 depth crops."""
    pre, S, _ = conv_terms(depth, wts["cnn/conv_1/conv_1_filters"], wts["cnn/conv_1/conv_1_biases"])
    s, t = bn_fold(wts, "batch_normalization")
    want = s * max_pool_same(np.maximum(pre, 0)) + t
    bnd = pool_windows(bound("conv1", 9, S, 0.0), 0.0).max(3) * np.abs(s) + 2 * U * np.abs(want)
    return LayerRef(want, bnd, {}, pre)


def conv_ref(x, wts, layer, bn, kind, store_bf16=False, names=MODELS):
    """BN(relu(conv + b)) of the float32 map x: conv_2 (bn = batch_normalization_1) or conv_3."""
    w, b = wts[f"cnn/{layer}/{layer}_filters"], wts[f"cnn/{layer}/{layer}_biases"]
    pre, S, A = conv_terms(x, w, b)
    s, t = bn_fold(wts, bn)
    rnd = to_bf16 if store_bf16 else (lambda v: v)

    def epi(p):
        return rnd(s * np.maximum(p, 0) + t)

    exact = s * np.maximum(pre, 0) + t
    bnd = bound(kind, w.shape[0] * w.shape[1] * w.shape[2], S, A) * np.abs(s) + 2 * U * np.abs(exact)
    b64 = b.astype(np.float64)
    models = {k: epi(v + b64) for k, v in split_models(conv2d_same, x, w, BB_ASCALE, names).items()}
    if store_bf16:
        return LayerRef(rnd(exact), bnd, models, pre, rnd(exact - bnd), rnd(exact + bnd))
    return LayerRef(exact, bnd, models, pre)


def _mm(a, b):
    return a @ b


_FC1_TERMS = {}


def _fc1_terms(w):
    """float64 w, |w| and the f16 split of fc_1's weights, kept for the last w (128 MB at width 1024)."""
    if _FC1_TERMS.get("w") is not w:
        w64 = w.astype(np.float64)
        _FC1_TERMS.update(w=w, terms=(w64, np.abs(w64), f16_split(w, weight_scale(w))))
    return _FC1_TERMS["terms"]


def fc1_ref(x, wts, kind, names=MODELS):
    """fc_1 + bias (before the relu) of float32 rows x [m, K]."""
    w, b = wts["cnn/fc_1/fc_1_weights"], wts["cnn/fc_1/fc_1_biases"].astype(np.float64)
    w64, aw, wsplit = _fc1_terms(w)
    x64 = x.astype(np.float64)
    pre = x64 @ w64 + b
    S = np.abs(x64) @ aw + np.abs(b)
    A = 2.0 ** -25 * aw.sum(0)
    models = {k: v + b for k, v in split_models(_mm, x, w, 1.0, names, wsplit).items()}
    return LayerRef(pre, bound(kind, w.shape[0], S, A) + 0 * pre, models, pre)


def relu1_ref(f1, wts):
    """BN_4(relu(fc1)) of the float32 fc1 tap; exact-fp32 kind at K = the width."""
    s, t = bn_fold(wts, "batch_normalization_4")
    f64 = f1.astype(np.float64)
    want = s * np.maximum(f64, 0) + t
    return LayerRef(want, bound("fp32", f1.shape[1], np.abs(f64), 0.0) * np.abs(s) + 2 * U * np.abs(want), {}, f64)


def out_ref(r1, wts):
    w, b = wts["cnn/fc_out/fc_out_weights"].astype(np.float64), wts["cnn/fc_out/fc_out_biases"].astype(np.float64)
    x64 = r1.astype(np.float64)
    pre = x64 @ w + b
    return LayerRef(pre, bound("fp32", w.shape[0], np.abs(x64) @ np.abs(w) + np.abs(b), 0.0), {}, pre)


# --------------------------------------------------------------------------------------- regions
def map_regions(imgs, n, H, W):
    """{name: bool mask [len(imgs), H, W]} over the reference images `imgs` of a batch of n."""
    m = len(imgs)
    reg = {"whole": np.ones((m, H, W), bool)}
    b = np.zeros((m, H, W), bool)
    b[:, (0, H - 1), :] = True
    b[:, :, (0, W - 1)] = True
    reg["border"] = b
    for lo, hi in ROW_SEAMS:
        if hi < H:
            s = np.zeros((m, H, W), bool)
            s[:, lo:hi + 1] = True
            reg[f"rows{lo}|{hi}"] = s
    for lo, hi in COL_SEAMS:
        if hi < W:
            s = np.zeros((m, H, W), bool)
            s[:, :, lo:hi + 1] = True
            reg[f"cols{lo}|{hi}"] = s
    for i in sorted(set(slice_ends(n))):
        s = np.zeros((m, H, W), bool)
        s[imgs.index(i)] = True
        reg[f"image{i}"] = s
    return reg


def fc_regions(rows, n):
    """{name: bool mask [len(rows)]} over the reference rows `rows` of a batch of n."""
    reg = {"whole": np.ones(len(rows), bool)}
    for i in fc_region_rows(n):
        s = np.zeros(len(rows), bool)
        s[rows.index(i)] = True
        reg[f"row{i}"] = s
    return reg


def _rms(d):
    return float(np.sqrt(np.mean(np.square(d)))) if d.size else float("nan")


def g2_gate(ref: LayerRef, dtype, mask):
    """The G2 gate of one region, from the reference and its models alone."""
    if dtype == "bf16":
        return 2.0 * _rms((ref.models["hihi"] - ref.want)[mask])
    return min(_rms((ref.models["drop_a"] - ref.want)[mask]), _rms((ref.models["drop_w"] - ref.want)[mask])) / 16.0


def g2_ratio(got, ref: LayerRef, dtype, regions):
    """(max over regions of rms(got - ref) / gate, the region); inf under a zero gate unless got == ref."""
    worst, where = 0.0, ""
    d = np.asarray(got, np.float64) - ref.want
    for name, mask in regions.items():
        e, g = _rms(d[mask]), g2_gate(ref, dtype, mask)
        r = 0.0 if e == 0 else (e / g if g > 0 else float("inf"))
        if r != r:
            r = float("inf")
        if r > worst or not where:
            worst, where = r, name
    return worst, where


def g1_ratio(got, ref: LayerRef):
    """max |got - ref| / bound.  For a bf16-stored map the kernel's fp32 value is what the bound holds for and
    the rounding is monotone, so got must lie in [bf16(ref - bound), bf16(ref + bound)]: the distance from
    bf16(ref) is measured against that end."""
    if ref.lo is None:
        return ratio(got, ref.want, ref.bnd + 0 * ref.want)
    got = np.asarray(got, np.float64)
    return max(ratio(np.maximum(got, ref.want), ref.want, ref.hi - ref.want),
               ratio(np.minimum(got, ref.want), ref.want, ref.want - ref.lo))


# ------------------------------------------------------------------------------ running the library
@functools.lru_cache(maxsize=2)
def context(name, dtype):
    row = ROWS[name]
    L = pkg()._lib
    ctx = L.Context(L.MP_MODEL_HGRU_POSE, 0)
    for k, v in pose_weights(row.H, row.W, row.width).items():
        ctx.set_weight(k, v)
    ctx.finalize(L.dtype_code(dtype))
    return ctx


def forward(ctx, row: Row, depth, o0, taps=()):
    """One pose_fwd_taps call: {"out": [n, 69], tap: array}.  Every buffer is one image / row too long and
    pre-filled with a sentinel that must survive (a partial tile must not store past n)."""
    import torch
    L = pkg()._lib
    n = depth.shape[0]
    shape = {k: (row.H, row.W, 64) for k in BACKBONE_TAPS + ("hgru",)}
    shape.update(fc1=(row.width,), relu1=(row.width,))
    d, o = torch.from_numpy(np.array(depth)).cuda(), torch.from_numpy(np.array(o0)).cuda()
    bufs = {k: torch.full((n + 1,) + shape[k], float(SENTINEL), device="cuda") for k in taps}
    out = torch.full((n + 1, NOUT), float(SENTINEL), device="cuda")
    ctx.pose_fwd_taps(d, o, out, bufs, L.current_stream())
    torch.cuda.synchronize()
    res = {"out": out.cpu().numpy(), **{k: v.cpu().numpy() for k, v in bufs.items()}}
    for k, a in res.items():
        assert (a[n:] == SENTINEL).all(), f"{k}: stored past image / row {n}"
        assert np.isfinite(a[:n]).all() and not (a[:n] == SENTINEL).all(), k
        res[k] = a[:n]
    return res


def _three_calls(ctx, row, depth, o0, same):
    """out of the untapped call (the production path) and the results of the calls with the backbone taps
    only and with the head taps only; `same` records whether their out is the untapped call's, bit for bit
    (asserted by the test after the gates, so that a differing path still reports its figures)."""
    plain = forward(ctx, row, depth, o0)
    bb = forward(ctx, row, depth, o0, BACKBONE_TAPS)
    hd = forward(ctx, row, depth, o0, HEAD_TAPS)
    same["out: backbone taps"] = bool(np.array_equal(plain["out"], bb["out"]))
    same["out: head taps"] = bool(np.array_equal(plain["out"], hd["out"]))
    return plain["out"], bb, hd


def _check(res, layer, got, ref, dtype, regions):
    g1 = g1_ratio(got, ref)
    g2, where = g2_ratio(got, ref, dtype, regions) if ref.models else (0.0, "")
    res["layers"][layer] = dict(g1=g1, g2=g2, g2_region=where)
    res["g1"], res["g2"] = max(res["g1"], g1), max(res["g2"], g2)


def run_backbone_row(name, dtype, n):
    """pool1, conv2, conv3 of one BACKBONE_ROWS row: worst err / bound (g1) and err / gate (g2)."""
    row, wts = ROWS[name], pose_weights(ROWS[name].H, ROWS[name].W, ROWS[name].width)
    ctx = context(name, dtype)
    depth, o0 = inputs(row, n)
    res = dict(row=name, dtype=dtype, n=n, g1=0.0, g2=0.0, layers={}, same={})
    _, bb, _ = _three_calls(ctx, row, depth, o0, res["same"])
    imgs = ref_images(n)
    reg = map_regions(imgs, n, row.H, row.W)
    kind = conv_kind(dtype, row.H)
    _check(res, "pool1", bb["pool1"][imgs], pool1_ref(depth[imgs], wts), dtype, reg)
    _check(res, "conv2", bb["conv2"][imgs], conv_ref(bb["pool1"][imgs], wts, "conv_2", "batch_normalization_1", kind),
           dtype, reg)
    _check(res, "conv3", bb["conv3"][imgs],
           conv_ref(bb["conv2"][imgs], wts, "conv_3", "batch_normalization_2", kind, store_bf16=dtype == "bf16"),
           dtype, reg)
    return res


def run_head_row(name, dtype, n):
    """fc1 (G1 + G2), relu1 and out (G1) of one HEAD_ROWS row, fc_1 on the production path (only fc1 and
    relu1 tapped: pre-split planes) against the hgru map of a second call; and the same gates on the call
    that taps all three (fc_1 splitting the fp32 map in its K loop)."""
    row, wts = ROWS[name], pose_weights(ROWS[name].H, ROWS[name].W, ROWS[name].width)
    ctx = context(name, dtype)
    depth, o0 = inputs(row, n)
    same = {}
    out, _, hd = _three_calls(ctx, row, depth, o0, same)
    hg = forward(ctx, row, depth, o0, ("hgru",))
    allh = forward(ctx, row, depth, o0, ("hgru",) + HEAD_TAPS)
    same["out: hgru tap"] = bool(np.array_equal(hg["out"], out))
    same["out: hgru and head taps"] = bool(np.array_equal(allh["out"], out))
    same["hgru: with head taps"] = bool(np.array_equal(allh["hgru"], hg["hgru"]))
    rows = fc_ref_rows(row, n)
    reg = fc_regions(rows, n)
    ref1 = fc1_ref(hg["hgru"].reshape(n, -1)[rows], wts, KIND[dtype])
    res = dict(row=name, dtype=dtype, n=n, g1=0.0, g2=0.0, layers={}, same=same,
               positive=float((ref1.pre > 0).mean()))
    for tag, r in (("", hd), ("/inloop", allh)):
        _check(res, "fc1" + tag, r["fc1"][rows], ref1, dtype, reg)
        _check(res, "relu1" + tag, r["relu1"], relu1_ref(r["fc1"], wts), dtype, reg)
        _check(res, "out" + tag, r["out"], out_ref(r["relu1"], wts), dtype, reg)
    return res


def run_row(name, dtype, n):
    return (run_head_row if name.startswith("head") else run_backbone_row)(name, dtype, n)


if __name__ == "__main__":   # child of a dispatch-switch test: rows as name:dtype:n, comma separated
    for spec in sys.argv[1].split(","):
        nm, dt, nn = spec.split(":")
        print(json.dumps(run_row(nm, dt, int(nn))), flush=True)
