"""The cases the channel-general loop's FFT association-field conv (nhwc_conv='fft', k_circuit_fft.hip) is
tested at, CPU and GPU.  Inputs, weights, oracle runs, metrics and bounds are circuit_channel_cases' and
circuit_shape_cases' as they stand; every case runs 'fp32_split' with T = circuit_channel_cases.T.

Each case is the smallest shape at which the thing it names can go wrong."""
import collections

import circuit_channel_cases as C

T = C.T
DTYPE = "fp32_split"
Case = collections.namedtuple("Case", "k n h w ssf variant nhwc_loop", defaults=(False,))

CASES = [
    Case(4, 2, 1, 1, 3, "pose"),                    # one group, M = 8 in a 32-row block, one live pixel
    Case(28, 2, 7, 9, 15, "pose"),                  # k % 8 == 4 (a zero half K step), map < filter, gated A_in
    Case(8, 3, 20, 28, 5, "defaults"),              # reads I0, n = 3, a width that is neither 32 nor 64
    Case(24, 2, 16, 32, 5, "mely"),                 # 2k % 32 != 0 with k % 8 == 0
    Case(32, 1, 33, 17, 3, "relu"),                 # unbounded states through f16 spectra
    Case(16, 1, 64, 64, 15, "output_gru_gates"),    # the full grid: 64 + 7 = 71 <= 72, no wrap; gated B_in
    Case(96, 2, 12, 40, 5, "pose"),                 # two M ranges, three K chunks of 32 channels
    Case(128, 1, 16, 32, 15, "defaults"),           # K = 256
    Case(256, 1, 8, 8, 3, "pose"),                  # the widest: four M ranges, 1.4 GB of weights
    Case(64, 2, 20, 28, 15, "output_gru_gates", True),   # 64 channels on a map every 64-channel rule rejects
]
STATES = C.STATES                       # (24, 2, 16, 32, 5): per-step states
STATES_VARIANTS = C.STATES_VARIANTS     # pose, defaults
BATCH = C.BATCH                         # (8, 9, 32, 5, "pose") at n = 1, 3, 66
BATCH_NS = C.BATCH_NS
CHUNK = (4, 2, 3, 3, "pose")            # k, h, w, ssf, variant at n = nhwc_fft_chunk + 3
CHUNK_EXTRA = 3
REUSE_K, REUSE_SSF, REUSE_SEQUENCE = C.REUSE_K, C.REUSE_SSF, C.REUSE_SEQUENCE
AGAINST_DIRECT = (24, 2, 16, 32, 5, "pose")
AGAINST_FFT64 = C.BOTH_LOOPS            # (64, 2, 16, 32, 5): the general loop's fp32_fft of DESIGN 3e
AGAINST_FFT64_VARIANTS = ("pose", "defaults")
SPEC_SCALE = 1.0 / 64.0                 # fft_dev.hpp
F16_RANGE_BOUND = 2.0 ** 15             # h * w * max|v| * SPEC_SCALE stays below half of f16's 65504


def case_id(c):
    return f"k{c.k}-n{c.n}-{c.h}x{c.w}-ssf{c.ssf}-{c.variant}" + ("-nhwc" if c.nhwc_loop else "")


def shape_of(c):
    return c.k, c.n, c.h, c.w, c.ssf


def chunk_images(k):
    """circuit_fft.hpp cnf_chunk, restated: the largest multiple of 32 images whose S + Y (k / 4 * 2664 * 32
    bytes each per image) fit 1 GiB, and at least 32"""
    per_image = (k + 3) // 4 * 2664 * 32
    return max(1, (1 << 30) // (2 * per_image) // 32) * 32
