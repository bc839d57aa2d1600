"""Case tables, inputs, float64 references and gates for the per-layer tests of the attention net
(attn_model_struct, MP_MODEL_ATTN; tests/test_gpu_attn_layers.py on the GPU,
tests/test_attn_layer_cases_cpu.py without one, and the child processes that re-run a row under a
dispatch switch: ``python attn_layer_cases.py ROWS``).

Every layer is compared with float64 of that one layer applied to the GPU's own input to it (the
previous tap of ``Context.attn_fwd_taps``, read back as float32), at 128 x 128 frames (the resize is
skipped), batches 1 / 3 / 11 / 130 and dtypes fp32_split / fp32 / bf16.  One further row feeds
424 x 512 frames at n = 3 and compares the ``resized`` tap with the TF1 bilinear restatement, bit for bit.

Frames: ``weights.synth_frames`` at 128 x 128 times FRAME_GAIN.  The glorot draw passes about a third of a
frame's signal from one stage to the next while every BN adds offsets of 0.1 .. 0.5: on depth in [0, 1] two
frames differ by 0.2 % rms at aconv_5, and an image taken from the wrong place in a shared tile hides
under every gate.  At FRAME_GAIN = 300 (depth in units of 1/30 m) they differ by 38 % there and 32 % at
relu1; tests/test_attn_layer_cases_cpu.py asserts it.

Weights: ``weights.synth_weights(weights.attn_vars(), SEED)`` with the six BN scopes redrawn: gamma in
+-[0.5, 1.5], negative on 30 % of each layer's channels (an affine applied before the max, or a fold that
loses the sign, is invisible on gammas near +1), beta and moving_mean of magnitude 0.1 .. 0.5 with random
sign, moving_variance in [0.25, 4].

Gates, per element (u = 2^-24; bound, kinds, S and A as in graph_op_cases):
  resized          np.array_equal with oracle.regressors_ref.resize_bilinear_tf1
  pool1            the fused aconv_1 + pool + BN kernel: kind conv1 with the folded-BN rule of
                   pose_layer_cases (the window's largest bound x |bn_s[c]| + 2u|ref|)
  conv2 .. conv5   relu(conv + b): bound(kind, K, S, A); kind is the dtype's (fp32 under fp32)
  pool2 .. pool5   BN(max) of the GPU's own conv tap.  The max m is exact.  mp_abi.hip bn_fold computes
                   s = g / sqrt(v + eps) and t = b - mean s in double and rounds each to float once:
                   s_f = s(1 + d1), t_f = t(1 + d2); pool2_kernel then evaluates fl(fl(m s_f) + t_f)
                   = ((m s (1 + d1)(1 + d3)) + t(1 + d2))(1 + d4), every |d| <= u (a contracted fma only
                   removes d3).  To first order |got - ref| <= u (2 |m s| + |t| + |ref|); the factor
                   1.001 covers the u^2 terms and the reference's own float64 rounding.
  relu1            BN(relu(afc_1)) of the pool5 tap: bound(kind, 16384, S, A) x |bn_s| + 2u|ref|
  out              afc_out of the relu1 tap: pose_layer_cases.out_ref's gate

Lost-plane gate G2 (pose_layer_cases), on conv3, conv4, conv5 and relu1 (K >= 1152) under fp32_split and
bf16: the f16 split is emulated as the kernels state it -- activations split unscaled (k_igemm.hip,
k_fc.hip: hi = f16(a), lo = f16(a - hi)), weights at 2^(14 - e) (k_fc.hip launch_pack_fc_x3) -- and per
region rms(got - ref) <= 1/16 of the lesser of the two dropped-product models (bf16: twice the
one-product model's).  Regions: the whole tensor, the image border, the rows on either side of each
R-row tile seam of the TALL halo kernel (R = 4 at 32 x 32, 8 at 16 x 16), the rows inside the tiles, and
every referenced image alone.

The kernel each conv took is read from mp_info ``attn_path:<scope>`` and must be the one the row names.
"""
import functools
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import pose_layer_cases as P  # noqa: E402
from graph_op_cases import U, conv_expected, conv_terms, pkg  # noqa: E402
from oracle import regressors_ref as RR  # noqa: E402
from oracle.hgru_ref import conv2d_same, max_pool_same  # noqa: E402

SEED = 2718
FRAME_SEED = 31
FRAME_GAIN = np.float32(300.0)
BIG_FRAME_SEED = 32
BATCHES = (1, 3, 11, 130)
DTYPES = ("fp32_split", "fp32", "bf16")
REF_IMAGES = {1: (0,), 3: (0, 1, 2), 11: (0, 5, 10), 130: (0, 63, 64, 127, 128, 129)}
BN_EPS = P.BN_EPS
SENTINEL = P.SENTINEL
NOUT = 3
# (scope, filter size, Cin, Cout, input map side)
CONVS = (("aconv_1", 3, 1, 64, 128), ("aconv_2", 3, 64, 128, 64), ("aconv_3", 3, 128, 256, 32),
         ("aconv_4", 3, 256, 512, 16), ("aconv_5", 5, 512, 1024, 8))
CONV = {c[0]: c for c in CONVS}
TALL_R = {"aconv_2": 2, "aconv_3": 4, "aconv_4": 8}      # rows per 128-pixel tile (k_igemm.hip halo_geom)
G2_LAYERS = ("conv3", "conv4", "conv5", "relu1")         # K = 1152, 2304, 12800, 16384
TAPS = ("resized", "conv2", "conv3", "conv4", "conv5", "pool1", "pool2", "pool3", "pool4", "pool5", "relu1")
LAYER_TAPS = TAPS[1:]
TAP_SHAPE = {"resized": (128, 128, 1), "pool1": (64, 64, 64), "conv2": (64, 64, 128), "pool2": (32, 32, 128),
             "conv3": (32, 32, 256), "pool3": (16, 16, 256), "conv4": (16, 16, 512), "pool4": (8, 8, 512),
             "conv5": (8, 8, 1024), "pool5": (4, 4, 1024), "relu1": (1024,)}
BIG_ROW = ("fp32_split", 3)                               # the 424 x 512 row (resized tap)
SWITCHES = ("MP_IGEMM_HALO_TALL=0", "MP_IGEMM_HALO=0", "MP_IGEMM_XCD=0")
SWITCH_ROW = ("fp32_split", 3)

_HALO_TALL = dict(family="halo", wr=1, ch=32, ks=3, pool=0, splits=1)      # MP_HALO_TALL
_HALO_WIDE = dict(_HALO_TALL, wr=2)                                        # MP_HALO_WIDE
_X3W = dict(family="x3w", pool=0, splits=1)
_F32 = dict(family="f32_im2col", nb=4, pool=0, splits=1)


def params():
    return [(d, n) for d in DTYPES for n in BATCHES]


def expected_paths(dtype, setting=""):
    """{scope: the attn_path fields the row must report}."""
    if dtype == "fp32":
        conv = {s: _F32 for s in ("aconv_2", "aconv_3", "aconv_4", "aconv_5")}
    else:
        halo = {"MP_IGEMM_HALO_TALL=0": _HALO_WIDE, "MP_IGEMM_HALO=0": _X3W}.get(setting, _HALO_TALL)
        conv = {"aconv_2": halo, "aconv_3": halo, "aconv_4": halo, "aconv_5": _X3W}
    return dict(conv, aconv_1=dict(family="conv1_pool_bn", pool=1))


def path_mismatches(paths, dtype, setting=""):
    """the (scope, field, got, expected) of every field that differs from the row's expectation"""
    bad = []
    for scope, want in expected_paths(dtype, setting).items():
        for k, v in want.items():
            if paths[scope].get(k) != v:
                bad.append((scope, k, paths[scope].get(k), v))
    return bad


# -------------------------------------------------------------------------------- inputs
def _frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=1)
def attn_weights():
    seed = SEED
    Wt = pkg().weights
    w = Wt.synth_weights(Wt.attn_vars(), seed)
    rng = np.random.default_rng(seed)
    for scope in RR.ATTN_BN:
        C = w[f"{scope}/gamma"].shape[0]
        neg = np.zeros(C, bool)
        neg[rng.permutation(C)[:(3 * C + 9) // 10]] = True
        w[f"{scope}/gamma"] = (rng.uniform(0.5, 1.5, C) * np.where(neg, -1.0, 1.0)).astype(np.float32)
        for k in ("beta", "moving_mean"):
            w[f"{scope}/{k}"] = (rng.uniform(0.1, 0.5, C) * rng.choice((-1.0, 1.0), C)).astype(np.float32)
        w[f"{scope}/moving_variance"] = rng.uniform(0.25, 4.0, C).astype(np.float32)
    return {k: _frozen(v) for k, v in w.items()}


@functools.lru_cache(maxsize=1)
def _frames_max():
    return _frozen(pkg().weights.synth_frames(max(BATCHES), seed=FRAME_SEED, h=128, w=128) * FRAME_GAIN)


def attn_frames(n):
    """[n, 128, 128, 1]; image i is the same at every batch size"""
    return _frames_max()[:n]


@functools.lru_cache(maxsize=1)
def big_frames():
    return _frozen(pkg().weights.synth_frames(BIG_ROW[1], seed=BIG_FRAME_SEED) * FRAME_GAIN)


def bn_raw(wts, scope):
    return tuple(wts[f"{scope}/{k}"].astype(np.float64) for k in ("gamma", "beta", "moving_mean", "moving_variance"))


def bn_fold(wts, scope):
    """(s, t) of inference BN as one affine, float64 (mp_abi.hip bn_fold before its rounding)."""
    g, b, m, v = bn_raw(wts, scope)
    s = g / np.sqrt(v + BN_EPS)
    return s, b - m * s


def _conv1_alias(wts):
    """the names pose_layer_cases.pool1_ref reads"""
    a = {f"cnn/conv_1/conv_1_{k}": wts[f"cnn/aconv_1/aconv_1_{k}"] for k in ("filters", "biases")}
    a.update({k: v for k, v in wts.items() if k.startswith("cnn/batch_normalization/")})
    return a


@functools.lru_cache(maxsize=1)
def _head_alias():
    """the names pose_layer_cases.fc1_ref / out_ref read: afc_1, its BN (the sixth), afc_out"""
    wts = attn_weights()
    a = {f"cnn/fc_1/fc_1_{k}": wts[f"cnn/afc_1/afc_1_{k}"] for k in ("weights", "biases")}
    a.update({f"cnn/fc_out/fc_out_{k}": wts[f"cnn/afc_out/afc_out_{k}"] for k in ("weights", "biases")})
    a.update({f"cnn/batch_normalization_4/{k}": wts[f"{RR.ATTN_BN[5]}/{k}"]
              for k in ("gamma", "beta", "moving_mean", "moving_variance")})
    return a


@functools.lru_cache(maxsize=4)
def _wsplit(scope):
    w = attn_weights()[f"cnn/{scope}/{scope}_filters"]
    return P.f16_split(w, P.weight_scale(w))


def g2_names(dtype):
    if dtype == "fp32":
        return ()
    return ("hihi",) if dtype == "bf16" else ("drop_a", "drop_w")


# ------------------------------------------------------------------------------- layer references
def pool1_ref(x, wts):
    """BN_0(maxpool(relu(aconv_1))) of the float32 128 x 128 input"""
    return P.pool1_ref(x, _conv1_alias(wts))


def conv_ref(x, wts, scope, kind, names=()):
    """relu(conv + b) of the float32 map x"""
    w, b = wts[f"cnn/{scope}/{scope}_filters"], wts[f"cnn/{scope}/{scope}_biases"]
    pre, S, A = conv_terms(x, w, b)
    want, bnd = conv_expected(pre, S, A, kind, w.shape[0] * w.shape[1] * w.shape[2], False)
    models = {}
    if names:
        b64 = b.astype(np.float64)
        ws = _wsplit(scope) if wts is attn_weights() else None
        models = {k: np.maximum(v + b64, 0) for k, v in P.split_models(conv2d_same, x, w, 1.0, names, ws).items()}
    return P.LayerRef(want, bnd, models, pre)


def pool_ref(cv, wts, scope):
    """BN(max_pool(cv)) of the float32 conv tap, from the raw BN variables; the bound of the module docstring"""
    m = max_pool_same(cv.astype(np.float64))
    g, b, mean, var = bn_raw(wts, scope)
    want = g * (m - mean) / np.sqrt(var + BN_EPS) + b
    s, t = bn_fold(wts, scope)
    bnd = 1.001 * U * (2 * np.abs(m * s) + np.abs(t) + np.abs(want))
    return P.LayerRef(want, bnd, {}, m)


def relu1_ref(x, wts, kind, names=()):
    """BN_5(relu(afc_1 + b)) of the float32 pool5 rows x [m, 16384]"""
    assert wts is attn_weights()
    alias = _head_alias()
    r = P.fc1_ref(x, alias, kind, names)
    s, t = P.bn_fold(alias, "batch_normalization_4")

    def epi(p):
        return s * np.maximum(p, 0) + t

    want = epi(r.pre)
    return P.LayerRef(want, r.bnd * np.abs(s) + 2 * U * np.abs(want), {k: epi(v) for k, v in r.models.items()}, r.pre)


def out_ref(r1, wts):
    assert wts is attn_weights()
    return P.out_ref(r1, _head_alias())


# --------------------------------------------------------------------------------------- regions
def map_regions(imgs, H, W, R=0):
    """{name: bool mask [len(imgs), H, W]}: whole, border, each image; with R-row tiles (R < H) the rows on
    either side of every tile seam and the rows inside the tiles"""
    m = len(imgs)
    reg = {"whole": np.ones((m, H, W), bool)}
    b = np.zeros((m, H, W), bool)
    b[:, (0, H - 1), :] = True
    b[:, :, (0, W - 1)] = True
    reg["border"] = b
    if 0 < R < H:
        rows = np.arange(H)
        seam = ((rows % R == 0) & (rows > 0)) | ((rows % R == R - 1) & (rows < H - 1))
        s = np.zeros((m, H, W), bool)
        s[:, seam] = True
        reg[f"seams{R}"] = s
        if (~seam).any():
            reg[f"inside{R}"] = ~s
    for j, i in enumerate(imgs):
        s = np.zeros((m, H, W), bool)
        s[j] = True
        reg[f"image{i}"] = s
    return reg


def row_regions(imgs):
    reg = {"whole": np.ones(len(imgs), bool)}
    for j, i in enumerate(imgs):
        s = np.zeros(len(imgs), bool)
        s[j] = True
        reg[f"row{i}"] = s
    return reg


# ------------------------------------------------------------------------------ running the library
@functools.lru_cache(maxsize=3)
def context(dtype):
    L = pkg()._lib
    ctx = L.Context(L.MP_MODEL_ATTN, 0)
    for k, v in attn_weights().items():
        ctx.set_weight(k, v)
    ctx.finalize(L.dtype_code(dtype))
    return ctx


def paths_of(ctx):
    G = pkg()._graph
    return {c[0]: G.decode_path(ctx.attn_path(c[0])) for c in CONVS}


def forward(ctx, frames, taps=(), imgs=None):
    """One attn_fwd_taps call: {"out": [n, 3], tap: the images `imgs` of it} (indexed on the device).  Every
    buffer is one image / row too long and pre-filled with a sentinel that must survive."""
    import torch
    L = pkg()._lib
    n = frames.shape[0]
    f = torch.from_numpy(np.array(frames)).cuda()
    bufs = {k: torch.full((n + 1,) + TAP_SHAPE[k], float(SENTINEL), device="cuda") for k in taps}
    out = torch.full((n + 1, NOUT), float(SENTINEL), device="cuda")
    ctx.attn_fwd_taps(f, out, bufs, L.current_stream())
    torch.cuda.synchronize()
    idx = None if imgs is None else torch.tensor(list(imgs), device="cuda")
    res = {}
    for k, v in dict(bufs, out=out).items():
        assert bool((v[n:] == float(SENTINEL)).all()), f"{k}: stored past image / row {n}"
        assert bool(torch.isfinite(v[:n]).all()) and not bool((v[:n] == float(SENTINEL)).any()), k
        res[k] = (v[:n] if k == "out" or idx is None else v[idx]).cpu().numpy()
    return res


def _check(res, layer, got, ref, dtype, regions=None):
    g1 = P.g1_ratio(got, ref)
    g2, where = P.g2_ratio(got, ref, dtype, regions) if ref.models else (0.0, "")
    res["layers"][layer] = dict(g1=g1, g2=g2, g2_region=where, positive=float((ref.pre > 0).mean()))
    res["g1"], res["g2"] = max(res["g1"], g1), max(res["g2"], g2)


def run_row(dtype, n, big=False):
    """Every tap of one (dtype, n) row: worst err / bound (g1) and err / gate (g2), the reported paths, and
    whether the tapped call's out is the plain call's, bit for bit."""
    wts, ctx = attn_weights(), context(dtype)
    frames = big_frames() if big else attn_frames(n)
    assert frames.shape[0] == n
    imgs = list(REF_IMAGES[n])
    kind = "fp32" if dtype == "fp32" else P.KIND[dtype]
    names = g2_names(dtype)
    res = dict(dtype=dtype, n=n, big=big, g1=0.0, g2=0.0, layers={}, same={})
    plain = forward(ctx, frames)
    t = forward(ctx, frames, TAPS if big else LAYER_TAPS, imgs)
    res["paths"] = paths_of(ctx)
    res["same"]["out: taps"] = bool(np.array_equal(plain["out"], t["out"]))
    x = frames[imgs]
    if big:
        res["same"]["resized"] = bool(np.array_equal(t["resized"], RR.resize_bilinear_tf1(x, 128, 128)))
        x = t["resized"]
    _check(res, "pool1", t["pool1"], pool1_ref(x, wts), dtype)
    for i, (scope, _, _, _, side) in enumerate(CONVS[1:], 2):
        cv, pl = f"conv{i}", f"pool{i}"
        reg = map_regions(imgs, side, side, TALL_R.get(scope, 0))
        _check(res, cv, t[cv], conv_ref(t[f"pool{i - 1}"], wts, scope, kind, names if cv in G2_LAYERS else ()),
               dtype, reg)
        _check(res, pl, t[pl], pool_ref(t[cv], wts, RR.ATTN_BN[i - 1]), dtype)
    _check(res, "relu1", t["relu1"], relu1_ref(t["pool5"].reshape(len(imgs), -1), wts, kind, names), dtype,
           row_regions(imgs))
    _check(res, "out", t["out"][imgs], out_ref(t["relu1"], wts), dtype)
    return res


if __name__ == "__main__":   # child of a dispatch-switch test: rows as dtype:n, comma separated
    for spec in sys.argv[1].split(","):
        dt, nn = spec.split(":")
        print(json.dumps(run_row(dt, int(nn))), flush=True)
