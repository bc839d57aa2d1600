"""Tables, inputs and bounds of the magnitude tests (tests/test_gpu_magnitude.py on the GPU,
tests/test_magnitude_cases_cpu.py without one): every f16-split kernel across the window of magnitudes
its scale gives it (include/monkeypose.h, "Magnitude windows").  Rows, inputs, float64 references, bounds
and split models are those of graph_op_cases, pose_layer_cases, circuit_shape_cases and
hgru_variant_cases; this module adds the magnitude axis.

Weight rescaling (part 1).  A layer's weights and bias times 2^j must give the same packed f16 fragments
(the per-tensor scale 2^(14 - e), frexp(max|w|) = (m, e), absorbs the factor) and an `unscale` exactly 2^j
larger, so the output is ldexp(baseline, j) bit for bit; relu and max pool commute with it.

Activation sweeps (part 2).  Input and bias times 2^j, j in J_SMALL and at the path's top: the largest j
for which every value the path splits stays at or below 2^TOP_LOG2 after its scale, computed here from the
float64 references' own maxima.  Scaling float32 data by 2^j is exact and so is the float64 reference of
the scaled data: ldexp(reference, j), which is what the sweeps use for the graph rows (pinned on the CPU).
The gate is the row's own bound (3K + 16) u S + A at the scaled input with the floor A / s of a path that
splits at scale s: an activation below the f16 normal range is split on the subnormal grid 2^-24, i.e.
2^-24 / s in its own units, half of which times sum |w| is the floor.

Outlier weights.  One weight 2^20 above the rest leaves the rest, scaled by wscale, at 2^-6 and below: their
hi halves are still normal f16 numbers (11 bits, off by up to 2^-11 |v| <= 2^-17), but the rests v - hi lie
far below 2^-14 and are stored on the subnormal grid 2^-24, so hi + lo is off by up to 2^-25 where an ordinary
tensor keeps 22 bits.  (The hi halves themselves would go subnormal only from 2^28 on.)  The weight is then
wrong by at most 2^-25 / wscale, the output by at most that times sum_k |x_k|: OUTLIER_TERM, added to the
row's bound for that tensor only (under bf16 the lost lo is inside the 2^-10 S term already).

The edge of a window.  2^15.9 is 7 % below f16's largest number, so one step beyond the top point (j + 1) a plane
overflows unless the maximum sits in that sliver; `overflow_j` is the first step that does, top + 1 or top + 2.
"""
import collections
import functools
import math

import numpy as np

import graph_op_cases as C
import pose_layer_cases as P
from graph_op_cases import U, bound, conv_expected, conv_terms, layer_w, ratio

J_RESCALE = (-20, -7, 7, 20)
J_SMALL = (-6, -12, -24)
TOP_LOG2 = 15.9                     # values the f16 planes hold after the path's scale: at most 2^15.9 < 65504
F16_MAX = 65504.0
GRAPH_SWEEP_DTYPES = ("fp32_split", "bf16")


def overflow_j(maxima, scale=1.0):
    """smallest j at which max * scale * 2^j rounds past f16's largest number (65520 and above round to inf)"""
    m = max(float(v) for v in maxima) * scale
    return int(math.floor(math.log2(65520.0 / m))) + 1


def top_j(maxima, scale=1.0):
    """largest j with max * scale * 2^j <= 2^TOP_LOG2 for every maximum given (float64)"""
    m = max(float(v) for v in maxima) * scale
    assert m > 0 and math.isfinite(m)
    return int(math.floor(TOP_LOG2 - math.log2(m)))


# ------------------------------------------------------------------------------- graph runtime
# one row of CONV_CASES per kernel family of the `path` fields, the smallest of each; the pooled halo and
# pooled split-K rows besides, for their epilogues
GRAPH_CONV_ROWS = ("x3_5x7_3to23", "x3w_7x5_8to200_s2", "x3wsk_4x4_512to96_k1", "pm_2x2_32to96", "pmsk_2x2_64to96_pool",
                   "halo_8x8_12to12", "tall_4x4_32to128_pool", "pw_5x5_8to16", "pwn_5x5_32to64")
GRAPH_SIBLING = "sib_24_40_10"
GRAPH_CONV1 = (("bn64", (6, 10)), ("any12", (6, 10)))
GRAPH_FC_K = (32, 40)
EDGE_HALO_ROW, EDGE_FC_K = "halo_8x8_16to32", 32
EDGE_TENSORS = ("pow2", "negmax", "outlier")

Op = collections.namedtuple("Op", "layer src out cols pool relu stride")


class Unit:
    """One recorded graph: its layers {name: (w, b)}, its input, the ops to check (`src`: None = the graph
    input, else the index of the output the op reads; `out`, `cols`: where its result is) and, for part 1,
    the layers whose weights are rescaled with the exponent each output then carries."""
    name = ""
    dtypes = ("fp32_split", "fp32")

    def graph(self):
        raise NotImplementedError

    def layers(self):
        raise NotImplementedError

    def x(self):
        raise NotImplementedError

    ops = ()
    rescaled = None                  # None: every layer
    out_exp = None                   # None: every output scales with j

    def kind(self, dtype, ctx, layer):
        return dtype

    def K(self, layer):
        w = self.layers()[layer][0]
        return int(np.prod(w.shape[:-1]))

    def ref_inputs(self, j, images=slice(None)):
        """{layer: the float32 input of its op} at sweep point j, each from the float64 reference of the op
        that produces it (the graph input for the first)"""
        x = np.ldexp(self.x()[images], j)
        refs, ins = {}, {}
        for op in self.ops:
            xin = x if op.src is None else refs[op.src]
            ins[op.layer] = xin
            w, b = self.layers()[op.layer]
            pre = conv_terms(_as_map(xin), _as_hwio(w), np.ldexp(b, j), op.stride)[0]
            v = np.maximum(pre, 0) if op.relu else pre
            refs[op.out] = (C.max_pool_same(v) if op.pool else v).astype(np.float32)
        return ins

    def split_maxima(self):
        """max |v| of every tensor the graph's kernels split at scale 1, from the float64 references"""
        return [float(np.abs(v).max()) for v in self.ref_inputs(0).values()]

    def top(self):
        return top_j(self.split_maxima())

    def overflow(self):
        return overflow_j(self.split_maxima())


def _as_map(x):
    return x if x.ndim == 4 else x.reshape(len(x), 1, 1, -1)


def _as_hwio(w):
    return w if w.ndim == 4 else w.reshape(1, 1, *w.shape)


class ConvUnit(Unit):
    def __init__(self, row):
        self.name, self.c = row, C.CONV_BY_NAME[row]
        self.dtypes = ("fp32_split", "fp32") + (("bf16",) if self.c.bf16 else ())
        self.ops = (Op("c", None, 0, None, self.c.pool, True, self.c.stride),)

    def graph(self):
        return C.conv_graph(self.c)

    def layers(self):
        ref = C.conv_reference(self.name)
        return {"c": (ref.w, ref.b)}

    def x(self):
        return C.conv_reference(self.name).x

    def kind(self, dtype, ctx, layer):
        return C.conv_bound_kind(dtype, C.pkg()._graph.conv_path(ctx, layer)["family"])


class EdgeConvUnit(ConvUnit):
    """a CONV_CASES row with its filter replaced by an edge tensor"""
    def __init__(self, row, edge):
        super().__init__(row)
        self.edge, self.name = edge, f"{row}/{edge}"

    @functools.lru_cache(maxsize=None)
    def layers(self):
        ref = C.conv_reference(self.c.name)
        return {"c": edge_tensor(ref.w, ref.b, self.edge)}

    def x(self):
        return C.conv_reference(self.c.name).x


class SiblingUnit(Unit):
    """test_1x1_siblings' graph: a 1x1 source conv, its 1x1 siblings (fused runs), a pool of each"""
    def __init__(self, case):
        self.name = case
        _, self.cs, self.couts, _, _ = next(c for c in C.SIBLING_CASES if c[0] == case)
        m = len(self.couts)
        self.ops = (Op("src", None, 0, None, False, True, 1),) + tuple(
            Op(f"s{i}", 0, 1 + i, None, False, True, 1) for i in range(m))
        self.rescaled = tuple(f"s{i}" for i in range(m))     # the source's output feeds their split: not scaled
        self.out_exp = (0,) + (1,) * (2 * m)

    def graph(self):
        g, src, sibs, pools = C.sibling_graph(self.cs, self.couts)
        return g, [src] + sibs + pools

    @functools.lru_cache(maxsize=None)
    def layers(self):
        lw = {"src": C.layer_weights(self.name + "/src", (1, 1, 8, self.cs))}
        for i, co in enumerate(self.couts):
            lw[f"s{i}"] = C.layer_weights(f"{self.name}/s{i}", (1, 1, self.cs, co))
        return lw

    def x(self):
        return C.conv_inputs(self.name, 5, 5, 8, 11)


class Conv1Unit(Unit):
    """the fused 1-channel conv + relu + pool kernels: fp32 FMAs under every dtype (bound kind conv1)"""
    dtypes = ("fp32_split", "fp32", "bf16")

    def __init__(self, case, hw):
        self.case, self.hw, self.name = case, hw, f"conv1_{case}_{hw[0]}x{hw[1]}"
        self.ops = (Op("c", None, 0, None, True, True, 1),)

    def graph(self):
        cout, _, _, H, W, _, _, _ = C.conv1_case(self.case, self.hw)
        g = C.pkg()._graph.GraphRecorder(H, W, 1)
        return g, [g.pool(g.conv(g.input, 1, cout, "c"))]

    @functools.lru_cache(maxsize=None)
    def layers(self):
        *_, w, b = C.conv1_case(self.case, self.hw)
        return {"c": (w, b)}

    @functools.lru_cache(maxsize=None)
    def x(self):
        return C.conv1_case(self.case, self.hw)[5]

    def kind(self, dtype, ctx, layer):
        return C.conv_bound_kind(dtype, C.pkg()._graph.conv_path(ctx, layer)["family"])


_FC_ORDER = ("f5", "f8", "f32r", "f32", "f69", "f130r", "f130")


class FcUnit(Unit):
    """test_fc's graph with all heads: K = 32 on the f16-split kernel, K = 40 on the fp32 one"""
    dtypes = ("fp32_split", "fp32", "bf16")

    def __init__(self, K, edge=None):
        self.Kin, self.edge, self.name = K, edge, f"fc{K}" + (f"/{edge}" if edge else "")
        where = {"f5": (0, slice(0, 5)), "f8": (0, slice(5, 13))}
        where.update({nm: (i + 1, None) for i, nm in enumerate(_FC_ORDER[2:])})
        self.ops = tuple(Op(nm, None, *where[nm], False, nm.endswith("r"), 1) for nm in _FC_ORDER)

    def graph(self):
        g, outs, _ = C.fc_graph(self.Kin)
        return g, outs

    @functools.lru_cache(maxsize=None)
    def layers(self):
        lw = C.fc_inputs(self.Kin, C.fc_heads(self.Kin))[1]
        return {nm: edge_tensor(w, b, self.edge) if self.edge else (w, b) for nm, (w, b) in lw.items()}

    def x(self):
        return C.fc_inputs(self.Kin, C.fc_heads(self.Kin))[0]

    def kind(self, dtype, ctx, layer):
        return dtype if (dtype == "fp32" or self.Kin % 32 == 0) else "fp32"     # K % 32 != 0: the fp32 kernel


@functools.lru_cache(maxsize=None)
def graph_units():
    units = [ConvUnit(r) for r in GRAPH_CONV_ROWS] + [SiblingUnit(GRAPH_SIBLING)]
    units += [Conv1Unit(c, hw) for c, hw in GRAPH_CONV1] + [FcUnit(K) for K in GRAPH_FC_K]
    return {u.name: u for u in units}


@functools.lru_cache(maxsize=None)
def edge_units():
    units = [EdgeConvUnit(EDGE_HALO_ROW, e) for e in EDGE_TENSORS] + [FcUnit(EDGE_FC_K, e) for e in EDGE_TENSORS]
    return {u.name: u for u in units}


def families_covered():
    fam = {dict(C.CONV_BY_NAME[r].path)["family"] for r in GRAPH_CONV_ROWS}
    fam |= set(next(c for c in C.SIBLING_CASES if c[0] == GRAPH_SIBLING)[4])
    fam |= {next(c for c in C.CONV1_CASES if c[0] == nm)[3] for nm, _ in GRAPH_CONV1}
    return fam


def edge_tensor(w, b, edge):
    """(w, b) float32 with the magnitude structure `edge` names; signs and pattern are the row's own"""
    w = np.array(w, np.float32)
    i = np.unravel_index(np.abs(w).argmax(), w.shape)
    if edge == "pow2":            # max |w| exactly 2^-3: frexp gives (0.5, -2), the lower edge of the scale's octave
        w = (w * np.float32(0.124 / np.abs(w).max())).astype(np.float32)
        w[i] = np.float32(0.125)
    elif edge == "negmax":        # the maximum held by a negative element, 1.5 times the largest positive one
        w[i] = -np.float32(1.5) * np.abs(w).max()
    elif edge == "outlier":       # one element 2^20 above the rest; the bias with the rest
        keep = w[i]
        w = np.ldexp(w, -20)
        w[i] = keep
        b = np.ldexp(np.asarray(b, np.float32), -20)
    else:
        raise ValueError(edge)
    return w, np.array(b, np.float32)


def outlier_term(x, w, stride=1):
    """OUTLIER_TERM of the module docstring, per output element: 2^-25 / wscale * sum_k |x_k|, float64"""
    w4 = _as_hwio(w)
    ones = np.ones(w4.shape[:3] + (1,))
    return 2.0 ** -25 / P.weight_scale(w) * C.conv2d_same(np.abs(np.asarray(_as_map(x), np.float64)), ones, stride)


def subnormal_lo_share(w):
    """share of the weights whose lo half is on f16's subnormal grid: |v - hi| <= 2^-11 |v| < 2^-14, i.e. the
    scaled weight below 2^-3"""
    v = np.abs(np.asarray(w, np.float64)) * P.weight_scale(w)
    return float((v < 2.0 ** -3).mean())


def op_expected(unit, op, xin, b, kind, floor_scale=1.0, outlier=False):
    """(expected output, per-element bound) of one op on the float32 input xin with bias b"""
    w = unit.layers()[op.layer][0]
    pre, S, A = conv_terms(_as_map(xin), _as_hwio(w), b, op.stride)
    want, bnd = conv_expected(pre, S, A / floor_scale, kind, unit.K(op.layer), op.pool)
    if not op.relu:
        want = pre
    if outlier and kind == "fp32_split":    # bf16 (hi x hi): the lost lo half is inside its 2^-10 S term already
        extra = outlier_term(xin, w, op.stride) + 0 * pre
        bnd = bnd + (C.pool_windows(extra, 0.0).max(3) if op.pool else extra)
    if w.ndim == 2:              # an FC head: [M, N]
        want, bnd = want.reshape(len(want), -1), bnd.reshape(len(bnd), -1)
    return want, bnd


def op_got(op, got):
    g = got[op.out]
    return g if op.cols is None else g[:, op.cols]


def floor_share(unit, op, j, kind):
    """A / bound on the dense images at sweep point j, from the float64 terms: the part of the bound that is
    the subnormal-lo floor (the smallest over the elements)"""
    w, b = unit.layers()[op.layer]
    x = unit.ref_inputs(j, slice(0, 3))[op.layer]
    pre, S, A = conv_terms(_as_map(x), _as_hwio(w), np.ldexp(b, j), op.stride)
    return float((A / bound(kind, unit.K(op.layer), S, A)).min())


def scaled_layers(unit, j, bias_only=False, zero_bias=False):
    """the unit's weights for the library: part 1 (weights and biases of `rescaled` times 2^j) or part 2
    (bias_only: every bias times 2^j; zero_bias: every bias zero)"""
    wts = {}
    for nm, (w, b) in unit.layers().items():
        if zero_bias:
            b = np.zeros_like(b)
        elif bias_only:
            b = np.ldexp(b, j)
        elif unit.rescaled is None or nm in unit.rescaled:
            w, b = np.ldexp(w, j), np.ldexp(b, j)
        wts.update(layer_w(nm, w, b))
    return wts


def run_unit(unit, dtype, wts, x):
    """the unit's graph on x with the given weights -> (outputs, ctx)"""
    g, outs = unit.graph()
    ctx = C.make_ctx(g, outs, wts, dtype)
    return C.forward(ctx, outs, x), ctx


def graph_rescale_mismatches(unit, dtype):
    """part 1 on the GPU: [(j, output index)] where the output is not ldexp(baseline, j) bit for bit"""
    x = unit.x()
    base, _ = run_unit(unit, dtype, scaled_layers(unit, 0), x)
    assert all(np.isfinite(a).all() and np.abs(a).max() > 0 for a in base)
    bad = []
    for j in J_RESCALE:
        got, _ = run_unit(unit, dtype, scaled_layers(unit, j), x)
        for i, (a, b0) in enumerate(zip(got, base)):
            e = j if unit.out_exp is None else j * unit.out_exp[i]
            if not np.array_equal(a, np.ldexp(b0, e)):
                bad.append((j, i))
    return bad


def graph_sweep_points(unit, dtype):
    return J_SMALL + (() if dtype == "bf16" else (unit.top(),))


def graph_sweep_ratio(unit, dtype, j, outlier=False):
    """part 2 on the GPU: max err / bound over the unit's ops at input and biases times 2^j, each op against
    float64 of the GPU's own input to it"""
    x = np.ldexp(unit.x(), j)
    got, ctx = run_unit(unit, dtype, scaled_layers(unit, j, bias_only=True), x)
    worst = 0.0
    for op in unit.ops:
        xin = x if op.src is None else got[op.src]
        b = np.ldexp(unit.layers()[op.layer][1], j)
        want, bnd = op_expected(unit, op, xin, b, unit.kind(dtype, ctx, op.layer), outlier=outlier)
        worst = max(worst, ratio(op_got(op, got), want, bnd))
    return worst


def graph_fp32_mismatches(unit):
    """the `fp32` dtype with zero bias: [(j, output)] where the output at input 2^j is not ldexp(baseline, j)"""
    x = unit.x()
    wts = scaled_layers(unit, 0, zero_bias=True)
    base, _ = run_unit(unit, "fp32", wts, x)
    assert all(np.abs(a).max() > 0 for a in base)
    bad = []
    for j in J_SMALL + (unit.top(),):
        got, _ = run_unit(unit, "fp32", wts, np.ldexp(x, j))
        bad += [(j, i) for i, (a, b0) in enumerate(zip(got, base)) if not np.array_equal(a, np.ldexp(b0, j))]
    return bad


def has_split(unit, op):
    """whether the op's kernel under the f16-split dtypes splits at all: the fused conv1 + pool kernels and
    the FC kernel of K % 32 != 0 are fp32 under every dtype"""
    return not isinstance(unit, Conv1Unit) and not (isinstance(unit, FcUnit) and unit.Kin % 32)


def graph_model_ratio(unit, op, dtype, j, images=slice(0, 3), outlier=False):
    """the CPU twin of graph_sweep_ratio: the numpy split model of the op (float64 sums of hi*hi + hi_w*lo_a +
    lo_w*hi_a; bf16: hi*hi) against the same reference and bound; FloatingPointError where a plane overflows"""
    assert has_split(unit, op)
    w, b = unit.layers()[op.layer]
    x = unit.ref_inputs(j, images)[op.layer]
    bj = np.ldexp(b, j)
    want, bnd = op_expected(unit, op, x, bj, dtype, outlier=outlier)
    name = "hihi" if dtype == "bf16" else "full"
    lin = lambda a, ww: C.conv2d_same(np.asarray(_as_map(a), np.float64), _as_hwio(ww), op.stride)   # noqa: E731
    pre = P.split_models(lin, x, w, 1.0, (name,))[name] + bj.astype(np.float64)
    got = np.maximum(pre, 0) if op.relu else pre
    got = C.max_pool_same(got) if op.pool else got
    return ratio(got.reshape(want.shape), want, bnd)


# ------------------------------------------------------------------------------------ pose model
POSE_BB_ROW, POSE_BB_N = "bb_32x32", 3
POSE_HEAD_ROW, POSE_HEAD_N = "head_32x32_w160", 33
POSE_LAYERS = ("conv_2", "conv_3", "fc_1")
_BN_AFTER = {"conv_1": "batch_normalization", "conv_2": "batch_normalization_1", "conv_3": "batch_normalization_2",
             "hgru": "batch_normalization_3", "fc_1": "batch_normalization_4"}
_TAP = {"conv_2": "conv2", "conv_3": "conv3", "fc_1": "fc1"}
POSE_SWEEP_DTYPES = ("fp32_fft", "fp32_split", "bf16")


def _scale(w, names, j):
    for n in names:
        w[n] = np.ldexp(w[n], j)


def _bn(layer, *fields):
    return [f"cnn/{_BN_AFTER[layer]}/{f}" for f in fields]


def _lw(layer):
    return [f"cnn/{layer}/{layer}_{'weights' if layer.startswith('fc') else 'filters'}", f"cnn/{layer}/{layer}_biases"]


def pose_rescaled_weights(row, layer, j):
    """Part 1: `layer`'s weights and biases times 2^j, and the folded BN after its relu taking the factor out
    again: gamma times 2^-j (s = gamma / sqrt(var + eps) scales exactly) and moving_mean times 2^j (so that
    t = beta - mean * s is the same double product).  relu(conv) is then ldexp(baseline, j) and
    s * relu(conv) + t the baseline's bits: conv_2's and conv_3's taps sit after that BN and must equal the
    baseline bit for bit, fc_1's tap sits before it and must equal ldexp(baseline, j); everything behind the
    layer stays inside its own window, so `out` keeps its bits too."""
    w = dict(P.pose_weights(row.H, row.W, row.width))
    _scale(w, _lw(layer), j)
    _scale(w, _bn(layer, "gamma"), -j)
    _scale(w, _bn(layer, "moving_mean"), j)
    return w


def pose_sweep_weights(row, path, j):
    """Part 2: the input of `path` ('backbone': conv_2's; 'fc_1': fc_1's) times 2^j with that layer's bias,
    the BN behind it taking the factor out again (pose_rescaled_weights).
      backbone  conv_1's filters and biases times 2^j and BN_0's shift with them (beta and moving_mean times
                2^j: t scales, s stays), so the pool1 tap is the baseline's times 2^j
      fc_1      BN_3's gamma and beta times 2^j: the hgru tap s * O + t is the baseline's times 2^j"""
    w = dict(P.pose_weights(row.H, row.W, row.width))
    if path == "backbone":
        _scale(w, _lw("conv_1") + _bn("conv_1", "beta", "moving_mean"), j)
        nxt = "conv_2"
    else:
        _scale(w, _bn("hgru", "gamma", "beta"), j)
        nxt = "fc_1"
    _scale(w, _lw(nxt)[1:], j)
    _scale(w, _bn(nxt, "gamma"), -j)
    _scale(w, _bn(nxt, "moving_mean"), j)
    return w


def pose_context(wts, dtype):
    L = C.pkg()._lib
    ctx = L.Context(L.MP_MODEL_HGRU_POSE, 0)
    for k, v in wts.items():
        ctx.set_weight(k, np.ascontiguousarray(v, np.float32))
    ctx.finalize(L.dtype_code(dtype))
    return ctx


def pose_run(row, n, wts, dtype, taps):
    ctx = pose_context(wts, dtype)
    res = P.forward(ctx, row, *P.inputs(row, n), taps)
    ctx.close()
    return res


def pose_rescale_mismatches(layer, dtype):
    """[(j, what)] where the tap (or `out`) departs from the identity pose_rescaled_weights states"""
    row, n = (P.ROWS[POSE_HEAD_ROW], POSE_HEAD_N) if layer == "fc_1" else (P.ROWS[POSE_BB_ROW], POSE_BB_N)
    tap = _TAP[layer]
    base = pose_run(row, n, dict(P.pose_weights(row.H, row.W, row.width)), dtype, (tap,))
    bad = []
    for j in J_RESCALE:
        got = pose_run(row, n, pose_rescaled_weights(row, layer, j), dtype, (tap,))
        if not np.array_equal(got[tap], np.ldexp(base[tap], j if layer == "fc_1" else 0)):
            bad.append((j, tap))
        if not np.array_equal(got["out"], base["out"]):
            bad.append((j, "out"))
    return bad


@functools.lru_cache(maxsize=None)
def hgru_tap_reference():
    """the hgru tap BN_3(O_T) of the head row's inputs [n, K] in float64 (oracle.hgru_ref.hgru_pose_forward, P.T
    steps), read-only: fc_1's input, whose maximum sets the top of fc_1's sweep"""
    from oracle import hgru_ref as R
    row = P.ROWS[POSE_HEAD_ROW]
    depth, o0 = P.inputs(row, POSE_HEAD_N)
    _, inter = R.hgru_pose_forward(depth, P.pose_weights(row.H, row.W, row.width), o0, P.T, np.float64, keep=True)
    tap = inter["hgru_bn"].reshape(POSE_HEAD_N, -1)
    tap.setflags(write=False)
    return tap


@functools.lru_cache(maxsize=None)
def pose_top(path):
    """the top sweep point of a pose path: conv_2 splits the pool1 tap at BB_ASCALE, fc_1 the hgru tap at 1"""
    if path == "backbone":
        row = P.ROWS[POSE_BB_ROW]
        wts = P.pose_weights(row.H, row.W, row.width)
        return top_j([np.abs(P.pool1_ref(P.inputs(row, POSE_BB_N)[0], wts).want).max()], P.BB_ASCALE)
    return top_j([np.abs(hgru_tap_reference()).max()], 1.0)


def pose_sweep_points(path, dtype):
    return J_SMALL + (() if dtype == "bf16" else (pose_top(path),))


def pose_g2_points(path):
    """G2 at the top and at j = -6.  At j = -12 the activations' lo halves have five bits left on the subnormal
    grid (2^-12 * 16 = 2^-8: hi ends at 2^-19, the grid at 2^-24), so the full model itself is less than 16
    times nearer than the model without them: that point cannot be reached and is left to G1 with its floor."""
    return (-6, pose_top(path))


def tighten_floor(ref, wts, layer, scale):
    """P.conv_ref's bound with the floor A / scale in place of A (the bound is linear in A, times |bn_s|)"""
    w = wts[_lw(layer)[0]].astype(np.float64)
    A = 2.0 ** -25 * np.abs(w).reshape(-1, w.shape[-1]).sum(0)
    s, _ = P.bn_fold(wts, _BN_AFTER[layer])
    ref.bnd = ref.bnd - (1.0 - 1.0 / scale) * A * np.abs(s)
    assert (ref.bnd > 0).all()
    return ref


def backbone_ref(x, wts, dtype, H, names=P.MODELS):
    """conv_2's reference on the float32 map x with the floor A / BB_ASCALE where the path splits"""
    kind = P.conv_kind(dtype, H)
    ref = P.conv_ref(x, wts, "conv_2", "batch_normalization_1", kind, names=names)
    return tighten_floor(ref, wts, "conv_2", P.BB_ASCALE) if kind != "fp32" else ref


def pose_sweep(path, dtype, j):
    """part 2 on the GPU for one pose path and sweep point: dict(g1, g2, max|input|, finite)"""
    if path == "backbone":
        row, n = P.ROWS[POSE_BB_ROW], POSE_BB_N
        wts = pose_sweep_weights(row, path, j)
        got = pose_run(row, n, wts, dtype, ("pool1", "conv2"))
        ref, xin, tap = backbone_ref(got["pool1"], wts, dtype, row.H), got["pool1"], got["conv2"]
        reg = P.map_regions(list(range(n)), n, row.H, row.W)
    else:
        row, n = P.ROWS[POSE_HEAD_ROW], POSE_HEAD_N
        wts = pose_sweep_weights(row, path, j)
        got = pose_run(row, n, wts, dtype, ("hgru", "fc1"))
        xin, tap = got["hgru"].reshape(n, -1), got["fc1"]
        ref = P.fc1_ref(xin, wts, P.KIND[dtype])
        reg = P.fc_regions(list(range(n)), n)
    g2 = P.g2_ratio(tap, ref, dtype, reg)[0] if j in pose_g2_points(path) else 0.0
    return dict(g1=P.g1_ratio(tap, ref), g2=g2, xmax=float(np.abs(xin).max()))


# ------------------------------------------------------------------------------------ hGRU loops
# Part 1: p_r and lateral_bias times 2^j, beta, nu and gamma times 2^-j.  P1 + lat and P2 + lat are then
# ldexp(baseline, j), beta O + nu and gamma ldexp(baseline, -j), and the products (beta O + nu)(P1 + lat) and
# gamma (P2 + lat) the baseline's bits (k_fft4.hip, conv_epi.hpp): every O_t and I_t must be too.
Loop = collections.namedtuple("Loop", "name source dtype shape variant general nhwc conv k", defaults=(False, False, None, 64))
LOOP_T = 3
LOOPS = (
    Loop("fused-fp32_fft", "shape", "fp32_fft", (2, 9, 32, 5), None),
    Loop("fused-bf16", "shape", "bf16", (2, 9, 32, 5), None),
    Loop("direct-fp32_split", "shape", "fp32_split", (1, 32, 32, 3), None),
    Loop("direct-fp32", "shape", "fp32", (2, 16, 32, 3), None),
    Loop("general-defaults", "variant", "fp32_fft", (2, 16, 32, 5), "defaults", True),
    Loop("nhwc-k8-direct", "channel", "fp32_split", (2, 5, 7, 3), "pose", False, False, "direct", 8),
    Loop("nhwc-k8-fft", "channel", "fp32_split", (2, 5, 7, 3), "pose", False, False, "fft", 8),
    Loop("nhwc-k8-fft_tiled", "channel", "fp32_split", (2, 5, 7, 3), "pose", False, False, "fft_tiled", 8),
)
LOOPS_BY_NAME = {c.name: c for c in LOOPS}
SIX_LAUNCH = ("fused-fp32_fft", "fused-bf16")       # again under MP_FFT4=0, in one child process
LOOP_UP, LOOP_DOWN = ("p_r", "lateral_bias"), ("beta", "nu", "gamma")


def loop_inputs(c):
    """(weights, X, O0, I0 or None, scope) of a LOOPS row from the module it is borrowed from"""
    n, h, w, ssf = c.shape
    if c.source == "shape":
        import circuit_shape_cases as S
        wts, X, O0, _ = S.inputs(n, h, w, ssf)
        return wts, X, O0, None, S.SCOPE
    if c.source == "variant":
        import hgru_variant_cases as HV
        X, O0, I0, _ = HV.inputs(c.shape)
        return HV.variant_weights(c.variant, ssf), X, O0, I0, HV.SCOPE
    import circuit_channel_cases as CC
    X, O0, I0 = CC.inputs(c.k, n, h, w)
    return CC.variant_weights(c.variant, c.k, ssf), X, O0, (I0 if c.general else None), CC.SCOPE


def loop_rescaled(wts, scope, j):
    w = dict(wts)
    _scale(w, [f"{scope}/{n}" for n in LOOP_UP if f"{scope}/{n}" in w], j)
    _scale(w, [f"{scope}/{n}" for n in LOOP_DOWN if f"{scope}/{n}" in w], -j)
    return w


def loop_run(c, wts, X, O0, I0, T=LOOP_T):
    """the facade with store_states -> (O_t stack, I_t stack) [n, T, h, w, k] as numpy"""
    import torch
    from helpers import HGRU_POSE_AUX
    import hgru_variant_cases as HV
    M = C.pkg().hgru_module

    def cuda(a):
        return torch.from_numpy(np.array(a, dtype=np.float32)).cuda()

    ssf = c.shape[3]
    if c.source == "shape":
        cc = M.ContextualCircuit(cuda(X), timesteps=T, SRF=1, SSN=ssf, SSF=ssf, aux=dict(HGRU_POSE_AUX, store_states=True))
        out, w, _ = cc.build(weights=wts, h2_init=cuda(O0), compute_dtype=c.dtype)
    else:
        cc = M.ContextualCircuit(cuda(X), timesteps=T, SSF=ssf, aux=dict(HV.VARIANTS[c.variant], store_states=True))
        cc.weights = wts
        kw = dict(nhwc_conv=c.conv) if c.conv else {}
        out, w, _ = cc.build(h2_init=cuda(O0), h1_init=cuda(I0) if I0 is not None else None, compute_dtype=c.dtype,
                             general_loop=c.general, nhwc_loop=c.nhwc, **kw)
    return out.cpu().numpy(), w['store_I'].cpu().numpy()


def loop_rescale_mismatches(name):
    """[(j, 'O' or 'I', first differing step)] of a LOOPS row"""
    c = LOOPS_BY_NAME[name]
    wts, X, O0, I0, scope = loop_inputs(c)
    assert all(f"{scope}/{n}" in wts for n in LOOP_UP + LOOP_DOWN), sorted(wts)
    bO, bI = loop_run(c, wts, X, O0, I0)
    assert np.isfinite(bO).all() and np.isfinite(bI).all() and bO.shape[1] == LOOP_T
    bad = []
    for j in J_RESCALE:
        gO, gI = loop_run(c, loop_rescaled(wts, scope, j), X, O0, I0)
        for tag, a, b0 in (("O", gO, bO), ("I", gI, bI)):
            steps = [t for t in range(LOOP_T) if not np.array_equal(a[:, t], b0[:, t])]
            if steps:
                bad.append((j, tag, steps[0], float(np.abs(a.astype(np.float64) - b0).max())))
    return bad


def loop_fft_loop(name):
    """the launches per step the library reports for the row's weights: 4 (the fused loop) or 6 (MP_FFT4=0)"""
    c = LOOPS_BY_NAME[name]
    L = C.pkg()._lib
    ctx = L.Context(L.MP_MODEL_HGRU_CIRCUIT, 0)
    for k, v in loop_inputs(c)[0].items():
        ctx.set_weight(k, v)
    ctx.finalize(L.dtype_code(c.dtype))
    n = ctx.info("fft_loop")
    ctx.close()
    return n


# ----------------------------------------------------------------- hGRU loops: the first half-step
# Part 2.  With O0 times 2^j the tanh of the input half-step saturates and hides every error, so the sweep runs a
# rescaled twin: O0 times 2^j with i_r, p_r and beta times 2^-j.  The gate g1 = sigmoid(O0 . i_r + i_b), the conv
# P1 = (O0 g1) * p_r + lat and beta O0 are then the baseline's, and so is I_1 = nl(X - (beta O0 + nu) P1) (pinned
# in float64 on the CPU), while the kernels split O0 2^j (the gate, at GATE_VSCALE), O0 g1 2^j (the direct conv,
# at ACT_SCALE) or its spectrum (at SPEC_SCALE).  One step, I_1 from states_I, held to the project's fp32-class
# rule (circuit_shape_cases.check) with e32 from the float32 oracle of the twin itself.
GATE_VSCALE, ACT_SCALE, SPEC_SCALE = 256.0, 1024.0, 1.0 / 64.0      # fft_dev.hpp, k_conv64x3.hip, fft_dev.hpp
FFT_GRID = 72
Twin = collections.namedtuple("Twin", "name loop gate conv")   # gate: the scale the i_r gate splits O0 at (None: exact fp32)
TWIN_LOOPS = {
    "fused-fp32_fft": LOOPS_BY_NAME["fused-fp32_fft"],
    "direct-fp32_split": LOOPS_BY_NAME["direct-fp32_split"],
    "general-relu": Loop("general-relu", "variant", "fp32_fft", (2, 16, 32, 5), "relu", True),
}
TWINS = (Twin("fused-fp32_fft", "fused-fp32_fft", GATE_VSCALE, "spec"),     # GATE_VSCALE, then SPEC_SCALE
         Twin("direct-fp32_split", "direct-fp32_split", None, "direct"),     # ACT_SCALE (the gates are exact fp32)
         Twin("general-relu", "general-relu", None, "spec"))                 # the gates take the exact fragment: SPEC_SCALE
TWINS_BY_NAME = {t.name: t for t in TWINS}
TWIN_DOWN = ("i_r", "p_r", "beta")
# Below 1 the twin's compensating weights grow as the state shrinks: the floor of the split, 2^-25 / s per
# activation (2^-19 per spectrum entry), reaches the gate's pre-activation times 2^-j sum|i_r| and the conv times
# 2^-j sum|p_r|, relative to an I_1 of order 1.  The numpy model of the splits itself then misses the fp32-class
# bound 1e-5: at j = -12 by 1e-4 on the two FFT paths (the direct conv's finer floor still holds: 1e-7), at
# j = -24 on every path (0.14, 4e-4, 0.35).  Those points are unreachable for this rule and dropped here
# (test_magnitude_cases_cpu.py pins that the model reaches every point kept and none of those dropped); the
# floor itself is gated in absolute terms at -12 and -24 on the graph and pose rows.
TWIN_SMALL = {"fused-fp32_fft": (-6,), "direct-fp32_split": (-6, -12), "general-relu": (-6,)}
TWIN_DROPPED = {"fused-fp32_fft": (-12, -24), "direct-fp32_split": (-24,), "general-relu": (-12, -24)}


def twin_aux(t):
    import hgru_variant_cases as HV
    c = TWIN_LOOPS[t.loop]
    from helpers import HGRU_POSE_AUX
    import hgru_variants_ref as V
    return V.full_aux(dict(HGRU_POSE_AUX) if c.source == "shape" else HV.VARIANTS[c.variant])


def twin_inputs(t, j, identity=False):
    """(weights, X, O0, I0, scope) of the twin at 2^j; identity: both initial states = X (hidden_init='identity'),
    X times 2^j"""
    c = TWIN_LOOPS[t.loop]
    wts, X, O0, I0, scope = loop_inputs(c)
    w = dict(wts)
    _scale(w, [f"{scope}/{n}" for n in TWIN_DOWN], -j)
    if identity:
        X = np.ldexp(X, j)
        return w, X, X, (None if I0 is None else X), scope
    return w, X, np.ldexp(O0, j), I0, scope


def half_step(t, wts, X, O0, I0, scope, dt=np.float64, model=False, aux=None):
    """dict(g1, A, P1, arg, I) of the first input half-step in `dt`; model: the gate and the conv through the
    numpy model of the path's f16 splits (float64 sums)"""
    import hgru_variants_ref as V
    from oracle import hgru_ref as R
    aux = aux or twin_aux(t)
    w = {k: np.asarray(v, dt) for k, v in wts.items()}
    X, O, I0 = X.astype(dt), O0.astype(dt), (None if I0 is None else I0.astype(dt))
    vec = lambda n: w[f"{scope}/{n}"].reshape(-1)   # noqa: E731
    i_r, p_r = w[f"{scope}/i_r"], w[f"{scope}/p_r"]
    if model and t.gate:
        pre = P.split_models(R.conv2d_same, O0, wts[f"{scope}/i_r"], t.gate, ("full",))["full"] + vec("i_b")
    else:
        pre = R.conv2d_same(O, i_r) + vec("i_b")
    g1 = R.sigmoid(pre)
    A = O * g1 if aux['gru_gates'] else O
    if not model:
        conv = R.conv2d_same(A, p_r)
    elif t.conv == "direct":
        conv = P.split_models(R.conv2d_same, A.astype(np.float32), wts[f"{scope}/p_r"], ACT_SCALE, ("full",))["full"]
    else:
        conv = spec_conv_model(A.astype(np.float32), wts[f"{scope}/p_r"])
    P1 = conv + vec("lateral_bias")
    c = V.constants(w, aux, scope, dt)
    arg = c['xi'] * X - (c['beta'] * O + c['nu']) * P1
    In = V.input_rule(P1, X, O, I0 if I0 is not None else X * 0, g1, c, aux)
    return dict(g1=g1, A=A, P1=P1, arg=arg, I=In)


def spectrum(a):
    """the 72 x 72 transform of [n, h, w, k] maps, as the FFT paths take it (zero padded)"""
    return np.fft.fft2(np.asarray(a, np.float64), s=(FFT_GRID, FFT_GRID), axes=(1, 2))


def kernel_spectrum(p_r):
    """G[fy, fx, ci, co] with ifft2(spectrum(a) G) = the SAME cross-correlation of a with p_r on maps up to 64 x 64"""
    ks = p_r.shape[0]
    r = ks // 2
    kf = np.zeros((FFT_GRID, FFT_GRID) + p_r.shape[2:])
    for dy in range(ks):
        for dx in range(ks):
            kf[(r - dy) % FFT_GRID, (r - dx) % FFT_GRID] = p_r[dy, dx]
    return np.fft.fft2(kf, axes=(0, 1))


def _csplit(z, scale):
    """complex hi and lo of the f16 split of z's real and imaginary parts at `scale`"""
    rh, rl = P.f16_split(z.real.astype(np.float32), scale)
    ih, il = P.f16_split(z.imag.astype(np.float32), scale)
    return rh + 1j * ih, rl + 1j * il


def spec_conv_model(a, p_r):
    """the FFT conv through the f16 split of its spectra: S = spectrum(a) / 64 and G = p_r's spectrum at its weight
    scale, each real and imaginary part hi + lo, every real product without lo * lo, float64 sums"""
    n, h, w, _ = a.shape
    Sh, Sl = _csplit(spectrum(a) * SPEC_SCALE, 1.0)
    G = kernel_spectrum(np.asarray(p_r, np.float64))
    ws = P.weight_scale(np.stack([G.real, G.imag]).astype(np.float32))
    Gh, Gl = _csplit(G, ws)
    Y = np.einsum("nyxi,yxio->nyxo", Sh + Sl, Gh + Gl) - _lolo(Sl, Gl)
    return np.fft.ifft2(Y / SPEC_SCALE, axes=(1, 2)).real[:, :h, :w]


def _lolo(Sl, Gl):
    """the lo * lo terms of the four real products of a complex product"""
    e = lambda a, b: np.einsum("nyxi,yxio->nyxo", a, b)   # noqa: E731
    return (e(Sl.real, Gl.real) - e(Sl.imag, Gl.imag)) + 1j * (e(Sl.real, Gl.imag) + e(Sl.imag, Gl.real))


@functools.lru_cache(maxsize=None)
def twin_split_maxima(name, identity=False):
    """max |v| * s of everything the twin's path splits, at j = 0, from the float64 half-step (each scales with 2^j)"""
    t = TWINS_BY_NAME[name]
    hs = half_step(t, *twin_inputs(t, 0, identity))
    O0 = twin_inputs(t, 0, identity)[2]
    m = []
    if t.gate:
        m.append(float(np.abs(O0).max()) * t.gate)
    if t.conv == "direct":
        m.append(float(np.abs(hs["A"]).max()) * ACT_SCALE)
    else:
        S = spectrum(hs["A"])
        m.append(float(max(np.abs(S.real).max(), np.abs(S.imag).max())) * SPEC_SCALE)
    return tuple(m)


def twin_top(name, identity=False):
    return top_j(twin_split_maxima(name, identity))


def twin_points(name):
    return TWIN_SMALL[name] + (twin_top(name),)


@functools.lru_cache(maxsize=None)
def twin_reference(name, j, identity=False):
    """(I_1 in float64, the three metrics of I_1 in float32 against it) of the twin at 2^j"""
    import circuit_shape_cases as S
    t = TWINS_BY_NAME[name]
    args = twin_inputs(t, j, identity)
    ref = half_step(t, *args)["I"]
    r32 = half_step(t, *args, dt=np.float32)["I"]
    ref.setflags(write=False)
    return ref, S.metrics(r32, ref, TWIN_LOOPS[t.loop].shape[3])


def twin_run(name, j, identity=False):
    """I_1 of the twin at 2^j on the GPU (one step, states_I)"""
    import torch
    from helpers import HGRU_POSE_AUX
    import hgru_variant_cases as HV
    t = TWINS_BY_NAME[name]
    c = TWIN_LOOPS[t.loop]
    wts, X, O0, I0, _ = twin_inputs(t, j, identity)
    M = C.pkg().hgru_module

    def cuda(a):
        return torch.from_numpy(np.array(a, dtype=np.float32)).cuda()

    ssf = c.shape[3]
    init = dict(hidden_init="identity") if identity else {}
    if c.source == "shape":
        cc = M.ContextualCircuit(cuda(X), timesteps=1, SRF=1, SSN=ssf, SSF=ssf, aux=dict(HGRU_POSE_AUX, store_states=True, **init))
        _, w, _ = cc.build(weights=wts, compute_dtype=c.dtype, **({} if identity else dict(h2_init=cuda(O0))))
    else:
        cc = M.ContextualCircuit(cuda(X), timesteps=1, SSF=ssf, aux=dict(HV.VARIANTS[c.variant], store_states=True, **init))
        cc.weights = wts
        kw = {} if identity else dict(h2_init=cuda(O0), h1_init=cuda(I0))
        _, w, _ = cc.build(compute_dtype=c.dtype, general_loop=c.general, **kw)
    return w['store_I'].cpu().numpy()[:, 0]


# ------------------------------------------------------------- the channel-general loop's FFT conv
# The worst case the header's sentence names: a constant-sign conv input with min(h, 64) min(w, 64) max|v| / 64 =
# 2^15.9, the DC entry of its spectrum.  The `defaults` aux convolves O itself; its twin (above) keeps I_1 unsaturated.
CNF_K, CNF_SSF, CNF_VARIANT = 8, 5, "defaults"
CNF_CASES = {"fft": (1, 20, 28), "fft_tiled": (1, 70, 40)}      # n, h, w: one window; two windows over one seam


def cnf_inputs(conv):
    """(weights, X, O0, I0, scope, jc): O0 in [0.75 c, c] with c min(h, 64) min(w, 64) / 64 = 2^15.9, the ceiling of a
    window's DC term, and i_r, p_r, beta times 2^-jc, jc = round(log2 c)"""
    import circuit_channel_cases as CC
    n, h, w = CNF_CASES[conv]
    X, O0, I0 = CC.inputs(CNF_K, n, h, w)
    c = 2.0 ** TOP_LOG2 / SPEC_SCALE / (min(h, 64) * min(w, 64))
    O0 = np.minimum(((0.75 + 0.25 * np.abs(O0) / np.abs(O0).max()) * c).astype(np.float32), np.float32(c))
    jc = int(round(math.log2(c)))
    wts = dict(CC.variant_weights(CNF_VARIANT, CNF_K, CNF_SSF))
    _scale(wts, [f"{CC.SCOPE}/{nm}" for nm in TWIN_DOWN], -jc)
    return wts, X, O0, I0, CC.SCOPE, jc


@functools.lru_cache(maxsize=None)
def cnf_reference(conv):
    """(I_1 float64, e32 metrics) through hgru_variants_ref.variant_forward"""
    import circuit_channel_cases as CC
    import circuit_shape_cases as S
    import hgru_variants_ref as V
    wts, X, O0, I0, scope, _ = cnf_inputs(conv)
    out = []
    for dt in (np.float64, np.float32):
        w = {k: v.astype(dt) for k, v in wts.items()}
        out.append(V.variant_forward(X.astype(dt), O0.astype(dt), I0.astype(dt), w, CC.aux_of(CNF_VARIANT), 1,
                                     scope=scope, keep_steps=True)[3][0])
    return out[0], S.metrics(out[1], out[0], CNF_SSF)


def cnf_run(conv):
    import torch
    import hgru_variant_cases as HV
    wts, X, O0, I0, _, _ = cnf_inputs(conv)

    def cuda(a):
        return torch.from_numpy(np.array(a, dtype=np.float32)).cuda()

    cc = C.pkg().hgru_module.ContextualCircuit(cuda(X), timesteps=1, SSF=CNF_SSF,
                                               aux=dict(HV.VARIANTS[CNF_VARIANT], store_states=True))
    cc.weights = wts
    _, w, _ = cc.build(h2_init=cuda(O0), h1_init=cuda(I0), compute_dtype="fp32_split", general_loop=True, nhwc_conv=conv)
    return w['store_I'].cpu().numpy()[:, 0]


# --------------------------------------------------------------- edge tensors on the fp32_fft circuit
def circuit_edge_weights(edge):
    """the fused loop's weights (LOOPS row fused-fp32_fft) with p_r replaced by an edge tensor"""
    wts, X, O0, _, scope = loop_inputs(LOOPS_BY_NAME["fused-fp32_fft"])
    w = dict(wts)
    w[f"{scope}/p_r"] = edge_tensor(wts[f"{scope}/p_r"], np.zeros(1, np.float32), edge)[0]
    return w, X, O0, scope


@functools.lru_cache(maxsize=None)
def circuit_edge_reference(edge):
    import circuit_shape_cases as S
    from oracle import hgru_ref as R
    w, X, O0, _ = circuit_edge_weights(edge)
    ref = R.hgru_forward(X.astype(np.float64), O0, w, LOOP_T)
    r32 = R.hgru_forward(X.astype(np.float32), O0, w, LOOP_T)
    return ref, S.metrics(r32, ref, 5)


def circuit_edge_run(edge):
    w, X, O0, _ = circuit_edge_weights(edge)
    return loop_run(LOOPS_BY_NAME["fused-fp32_fft"], w, X, O0, None)[0][:, -1]


if __name__ == "__main__":   # child of the six-launch test (MP_FFT4=0): LOOPS rows, comma separated
    import json
    import sys
    for nm in sys.argv[1].split(","):
        print(json.dumps(dict(row=nm, bad=loop_rescale_mismatches(nm), fft_loop=loop_fft_loop(nm))), flush=True)
