"""The cases the tiled FFT association-field conv (nhwc_conv='fft_tiled': overlap-save over 64 x 64 windows,
k_circuit_fft.hip) is tested at, CPU and GPU.  Inputs, weights, oracle runs, metrics and bounds are
circuit_channel_cases' and circuit_shape_cases' as they stand; every case runs 'fp32_split' with
T = circuit_channel_cases.T.  One region joins the three of circuit_shape_cases: the seam band, the rows and
columns within the filter's radius of a tile boundary, held to the same bound on the same metric.

Each case is the smallest shape at which the thing it names can go wrong."""
import collections

import numpy as np

import circuit_channel_cases as C
import circuit_fft_cases as F
import circuit_shape_cases as S
from helpers import FP32_REL_TOL, rel_inf

T = C.T
DTYPE = F.DTYPE
WINDOW = 64                              # circuit_fft.hpp CNF_MAX_HW
Case = collections.namedtuple("Case", "k n h w ssf variant nhwc_loop", defaults=(False,))

CASES = [
    Case(8, 2, 65, 8, 15, "pose"),                  # two tiles in y, one in x; tile 1 owns 15 rows, its window mostly past the map
    Case(8, 2, 8, 65, 15, "pose"),                  # the transpose
    Case(4, 1, 65, 65, 3, "pose"),                  # 2 x 2 tiles, one channel group, T = 62
    Case(28, 1, 61, 121, 5, "defaults"),            # k % 8 == 4, y untiled, x in three tiles, the last owns one column; reads I0
    Case(8, 3, 12, 120, 15, "output_gru_gates"),    # three tiles: the middle one has live halos on both sides; n = 3; gated B_in
    Case(8, 1, 100, 70, 15, "mely"),                # L an exact multiple of T: no remainder tile
    Case(96, 1, 66, 20, 5, "pose"),                 # two M ranges
    Case(64, 1, 70, 20, 15, "output_gru_gates", True),   # 64 channels through the flag
    Case(8, 1, 70, 70, 3, "relu"),                  # unbounded states on a tiled map
]
STATES = (8, 2, 65, 8, 15)              # k, n, h, w, ssf: per-step states
STATES_VARIANTS = ("pose", "defaults")
SMALL = [(24, 2, 16, 32, 5, "mely"), (16, 1, 64, 64, 15, "output_gru_gates")]   # 'fft_tiled' == 'fft', bit for bit
BATCH = (8, 65, 65, 5, "pose")          # k, h, w, ssf, variant: 4 tiles per image
BATCH_NS = (1, 3, 9)                    # 36 tiles: image 8 is in the product's second, partly filled 32-tile block
CHUNK = (256, 1, 250, 3, "pose")        # k, h, w, ssf, variant: 5 tiles per image, 96 tiles per chunk
CHUNK_N = 20                            # 100 tiles: the chunk boundary falls after tile 0 of image 19
CHUNK_IMAGES = (0, 18, 19)
REUSE_K, REUSE_SSF = 8, 15
REUSE_SEQUENCE = [(1, 65, 8), (2, 20, 28), (1, 12, 120), (1, 65, 8)]
AGAINST_DIRECT = (8, 2, 65, 8, 15, "pose")
MODEL_EXTRA_SHAPES = [(64, 65, 15), (129, 1, 15), (1, 187, 3)]
PLAN_MAX_L = 300


def case_id(c):
    return F.case_id(c)


def shape_of(c):
    return c.k, c.n, c.h, c.w, c.ssf


def plan(L, ssf):
    """circuit_fft.hpp's tile plan along an axis of length L, restated: [(origin, out0, count)] per tile"""
    r = ssf // 2
    if L <= WINDOW:
        return [(0, 0, L)]
    t = WINDOW - 2 * r
    return [(i * t - r, r, min(t, L - i * t)) for i in range(-(-L // t))]


def tiles_per_image(h, w, ssf):
    return len(plan(h, ssf)) * len(plan(w, ssf))


def seam_mask(h, w, ssf):
    """boolean [h, w]: the rows and columns within the filter's radius of a tile boundary i T, i >= 1"""
    r = ssf // 2

    def axis(L):
        pos = np.arange(L)
        m = np.zeros(L, bool)
        for origin, out0, _ in plan(L, ssf)[1:]:
            b = origin + out0                       # the first position the tile owns
            m |= (pos >= b - r) & (pos < b + r)
        return m
    return axis(h)[:, None] | axis(w)[None, :]


def seam_metric(got, ref, ssf):
    """rel_inf on the seam band, relative to max|ref| of the band; None on an untiled map"""
    m = seam_mask(ref.shape[1], ref.shape[2], ssf)
    return rel_inf(np.asarray(got)[:, m], np.asarray(ref)[:, m]) if m.any() else None


def check(what, got, ref, ssf, e32_metrics, ref32):
    """circuit_shape_cases.check on its three regions, then the seam band on the same bounds: the project
    gate and max(10 * e32, 1e-5), e32 the float32 oracle's error on the band"""
    errs = S.check(what, got, ref, ssf, DTYPE, e32_metrics)
    e = seam_metric(got, ref, ssf)
    if e is not None:
        bound = S.fp32_class_bound(seam_metric(ref32, ref, ssf))
        print(f"{what}: rel_inf seam {e:.3e} (bound {min(bound, FP32_REL_TOL):.3e})")
        assert e <= FP32_REL_TOL, (what, "seam", e)
        assert e <= bound, (what, "seam", e, bound)
    return errs
