"""The stream-ordering contract of include/monkeypose.h ("asynchronous on `stream`"): a hazard harness
and the table of calls it runs, shared by tests/test_gpu_stream_order.py (GPU) and
tests/test_stream_order_cases_cpu.py (the table covers every exported function with a stream argument).

A case is one call as a user writes it (a facade or a ``_lib.Context`` method under
``with torch.cuda.stream(s)``) with two input sets A and B of different seeds:

    make(seed)  host inputs {name: numpy array}; no GPU
    alloc()     the context or model and the output buffers the case owns (``self.inp`` already holds one
                device tensor per input, filled with B)
    invoke()    the call on torch's current stream -> {output name: device tensor}
    outputs     the names ``invoke`` returns
    check_plain(A, got)   the plain result on A against float64 / the host function, where the suite does
                not pin that shape already

``check_hazards`` compares bytes with the plain run (default stream, inputs complete, device sync after):

    H1 late producer       a delay on the caller's stream s, then A copied into the input buffers on s from
                           device staging copies, then invoke: a side stream or a stream-0 launch that does
                           not wait for s computes on B, which is valid data (never NaN or garbage: an
                           ordering bug must give wrong numbers, not an out-of-range index)
    H2 immediate consumer  owned output buffers hold NaN before the delay; every output is cloned on s right
                           after invoke returns: a missing join clones NaN or the previous result
    H3 early release       right after the clones every input buffer is overwritten with B on s: a read
                           after the join, or of a temporary the facade dropped, sees B
    H4 back to back        invoke on A, clone, B in, invoke, clone, all on s with no host wait: both clones
                           equal their plain runs (write-after-read on the context's workspace)
    conclusive             an event recorded on s right after the delay must still be unfinished after the
                           last enqueue (everything was queued while the producer was blocked); else one
                           repeat with a 4x delay, else the test fails as inconclusive -- never a skip

The delay is a chain of in-place torch adds on a 256 MiB buffer, its length calibrated once per process
with events.  DELAY_MS follows the rule max(50 ms, 20 x the slowest case's enqueue time) capped at 1 s;
the figures it was chosen from are in tests/test_gpu_stream_order.py's docstring.
"""
import ctypes
import json
import os
import re
import sys

import numpy as np

from helpers import BF16_REL_TOL, FP32_REL_TOL, MG, ROOT, golden_array, golden_meta, pkg, rel_inf

SEED_A, SEED_B = 0, 1
DELAY_MS = 52.0
DELAY_BYTES = 256 << 20
HEADER = os.path.join(ROOT, "include", "monkeypose.h")
CAM_REF = (365.456, 365.456, 256, 212, [800, 800, 1200], 200, 10000)
CAM_NEAR = (365.456, 365.456, 256, 212, [800, 800, 1200], 200, 2500)


# ------------------------------------------------------------------------------------------ the header
def stream_prototypes(path=HEADER):
    """names of every function include/monkeypose.h declares with a ``stream`` parameter"""
    with open(path) as f:
        text = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)
    text = re.sub(r"^\s*#.*$", " ", text, flags=re.M)
    names = []
    for m in re.finditer(r"\b(mp_\w+)\s*\(([^;{}()]*)\)\s*;", text):
        params = [p.strip() for p in m.group(2).split(",")]
        if any(re.search(r"\bstream$", p) for p in params):
            names.append(m.group(1))
    return names


def exported_functions(path=HEADER):
    with open(path) as f:
        text = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)
    return sorted(set(re.findall(r"\b(mp_\w+)\s*\([^;{}()]*\)\s*;", text)))


# ------------------------------------------------------------------------------------------ the cases
class Case:
    name = ""
    covers = ()             # header functions this case reaches
    outputs = ()
    may_coincide = ()       # outputs that may be the same bytes for A and B

    def make(self, seed):
        raise NotImplementedError

    def alloc(self):
        pass

    def invoke(self):
        raise NotImplementedError

    def check_plain(self, A, got):
        pass

    def close(self):
        pass


def _W():
    return pkg().weights


def _L():
    return pkg()._lib


def _st():
    return _L().current_stream()


def _nan(shape, dtype=None):
    import torch
    return torch.full(tuple(shape), float("nan"), dtype=dtype or torch.float32, device="cuda")


def _vp(t):
    return ctypes.c_void_p(None if t is None else int(t.data_ptr()))


POSE_MAP = (16, 32)         # crop (32, 64): the smallest map the FFT path takes
POSE_WIDTH = 32
POSE_REF_IMAGES = (0, 31, 32, 63)
POSE_RNG = (77, 5)          # hidden_init 'random': the draw's seed and call index


class PoseCase(Case):
    """hgru_pose through Context.pose_fwd / pose_fwd_taps at T = 2 on pose_layer_cases' weights.  n = 3 is
    one slice (rowq); n = 64 two slices of 32 with the staggered backbone (ev_fork, ev_pre, ev_join)."""

    def __init__(self, dtype, n, mode="plain"):
        self.dtype, self.n, self.mode = dtype, n, mode
        self.name = f"pose-{dtype}-n{n}-{mode}"
        self.covers = {"plain": ("mp_hgru_pose_fwd",), "taps": ("mp_hgru_pose_fwd_taps",)}.get(
            mode, ("mp_hgru_pose_fwd_ex",))
        self.outputs = ("out",)
        if mode == "taps":
            self.outputs += _L().TAP_NAMES
        if mode == "states":
            self.outputs += _L().STATE_NAMES

    def make(self, seed):
        H, Wd = POSE_MAP
        depth = np.ascontiguousarray(_W().synth_crops(self.n, seed=9100 + 37 * seed, size=2 * Wd)[:, :2 * H, :2 * Wd])
        return {"depth": depth, "o0": _W().synth_hidden((self.n, H, Wd, 64), seed=9200 + 37 * seed)}

    def weights(self):
        import pose_layer_cases as PL
        return PL.pose_weights(POSE_MAP[0], POSE_MAP[1], POSE_WIDTH)

    def alloc(self):
        import pose_layer_cases as PL
        L, n, (H, Wd) = _L(), self.n, POSE_MAP
        self.ctx = L.Context(L.MP_MODEL_HGRU_POSE, 0)
        for k, v in self.weights().items():
            self.ctx.set_weight(k, v)
        self.ctx.finalize(L.dtype_code(self.dtype))
        self.T = PL.T
        shape = {"out": (n, PL.NOUT), "conv1": (n, 2 * H, 2 * Wd, 64), "fc1": (n, POSE_WIDTH), "relu1": (n, POSE_WIDTH)}
        for k in ("pool1", "conv2", "conv3", "hgru"):
            shape[k] = (n, H, Wd, 64)
        for k in L.STATE_NAMES:
            shape[k] = (n, self.T, H, Wd, 64)
        self.out = {k: _nan(shape[k]) for k in self.outputs}

    def invoke(self):
        L, c, o = _L(), self.ctx, self.out
        d, o0 = self.inp["depth"], self.inp["o0"]
        if self.mode == "plain":
            c.pose_fwd(d, o0, o["out"], _st())
        elif self.mode == "taps":
            taps = L.PoseTaps(*[_vp(o[k]) for k in L.TAP_NAMES])
            n, h, w, _ = d.shape
            L.check(c.lib.mp_hgru_pose_fwd_taps(c.h, _vp(d), n, h, w, _vp(o0), _vp(o["out"]), ctypes.byref(taps),
                                                ctypes.c_void_p(_st())))
        elif self.mode == "states":
            c.pose_fwd_taps(d, o0, o["out"], {k: o[k] for k in L.STATE_NAMES}, _st())
        elif self.mode == "random":
            c.pose_fwd_taps(d, None, o["out"], {}, _st(), L.MP_HIDDEN_RANDOM, *POSE_RNG)
        else:
            c.pose_fwd_taps(d, None, o["out"], {}, _st(), L.MP_HIDDEN[self.mode])
        return dict(o)

    def check_plain(self, A, got):
        if self.n != 64 or self.mode not in ("plain", "zeros", "identity", "random"):
            return
        from oracle import hgru_ref as R
        idx = list(POSE_REF_IMAGES)
        hi = "random" if self.mode == "plain" else self.mode
        o0 = A["o0"][idx] if self.mode == "plain" else None
        if self.mode == "random":       # the library's draw, restated on the host (monkeypose.h MP_HIDDEN_RANDOM)
            o0 = _W().synth_hidden((self.n,) + POSE_MAP + (64,), seed=sum(POSE_RNG))[idx]
        ref = R.hgru_pose_forward(A["depth"][idx], dict(self.weights()), None if o0 is None else o0.astype(np.float64),
                                  self.T, np.float64, hidden_init=hi)
        err = rel_inf(got["out"][idx], ref)
        print(f"{self.name}: plain out rel_inf vs float64 on images {idx}: {err:.3e}")
        assert err <= (BF16_REL_TOL if self.dtype == "bf16" else FP32_REL_TOL), err

    def close(self):
        self.ctx.close()


class CircuitCase(Case):
    """the fused 64-channel loop through _lib.Context (the ContextualCircuit.build facade synchronises by
    design): 9 x 32, ssf 5, on circuit_shape_cases' weights"""
    H, Wd, SSF = 9, 32, 5

    def __init__(self, n, entry, states=False):
        self.n, self.entry, self.states = n, entry, states
        self.name = f"circuit-fp32_fft-n{n}-{entry}" + ("-states" if states else "")
        self.covers = ({"opts": "mp_hgru_circuit_fwd_opts", "ex": "mp_hgru_circuit_fwd_ex",
                        "plain": "mp_hgru_circuit_fwd"}[entry],)
        self.outputs = ("O",) + (("states_O", "states_I") if states else ())

    def _S(self):
        import circuit_shape_cases as S
        return S

    def make(self, seed):
        S = self._S()
        if seed == SEED_A:
            _, X, O0, _ = S.inputs(self.n, self.H, self.Wd, self.SSF)
            return {"x": np.array(X), "o0": np.array(O0)}
        shape = (self.n, self.H, self.Wd, 64)
        return {"x": _W().sym_uniform(8100 + seed, "X", shape, 1.0), "o0": _W().sym_uniform(8200 + seed, "O0", shape, 0.5)}

    def alloc(self):
        S, L = self._S(), _L()
        self.ctx = L.Context(L.MP_MODEL_HGRU_CIRCUIT, 0)
        for k, v in S.inputs(self.n, self.H, self.Wd, self.SSF)[0].items():
            self.ctx.set_weight(k, v)
        self.ctx.finalize(L.dtype_code("fp32_fft"))
        shape = (self.n, self.H, self.Wd, 64)
        self.out = {"O": _nan(shape)}
        if self.states:
            for k in ("states_O", "states_I"):
                self.out[k] = _nan((self.n, S.T) + shape[1:])

    def invoke(self):
        S, L, c, o = self._S(), _L(), self.ctx, self.out
        x, o0 = self.inp["x"], self.inp["o0"]
        n, h, w, k = x.shape
        if self.entry == "opts":
            c.circuit_fwd(x, o0, o["O"], S.T, _st(), 0, o.get("states_O"), o.get("states_I"))
        elif self.entry == "ex":
            L.check(c.lib.mp_hgru_circuit_fwd_ex(c.h, _vp(x), _vp(o0), n, h, w, k, S.T, 0, _vp(o["O"]),
                                                 _vp(o.get("states_O")), _vp(o.get("states_I")), ctypes.c_void_p(_st())))
        else:
            L.check(c.lib.mp_hgru_circuit_fwd(c.h, _vp(x), _vp(o0), n, h, w, k, S.T, _vp(o["O"]), ctypes.c_void_p(_st())))
        return dict(o)

    def check_plain(self, A, got):
        S = self._S()
        args = (self.n, self.H, self.Wd, self.SSF)
        O, so, si = S.oracle(*args)
        e = S.e32(*args)
        S.check(f"{self.name} plain O", got["O"], O, self.SSF, "fp32_fft", e["O"])
        if self.states:
            t = S.T - 1
            S.check(f"{self.name} plain O_{t}", got["states_O"][:, t], so[t], self.SSF, "fp32_fft", e["O_t"][t])
            S.check(f"{self.name} plain I_{t}", got["states_I"][:, t], si[t], self.SSF, "fp32_fft", e["I_t"][t])

    def close(self):
        self.ctx.close()


class CircuitVarCase(Case):
    """mp_hgru_circuit_fwd_var, the general loop, on a variant that reads I0 (hgru_variant_cases)"""
    VARIANT, SHAPE = "defaults", (2, 16, 32, 5)
    name = "circuit_var-fp32_fft-defaults"
    covers = ("mp_hgru_circuit_fwd_var",)
    outputs = ("O", "I")

    def make(self, seed):
        import hgru_variant_cases as HV
        X, O0, I0, _ = HV.inputs(self.SHAPE, HV.SEED + 100 * seed)
        return {"x": np.array(X), "o0": np.array(O0), "i0": np.array(I0)}

    def alloc(self):
        import hgru_variant_cases as HV
        L, M = _L(), pkg().hgru_module
        aux = M.merged_aux(HV.VARIANTS[self.VARIANT])
        assert M.reads_previous_i(aux)
        self.variant = L.circuit_variant(aux)
        self.ctx = L.Context(L.MP_MODEL_HGRU_CIRCUIT, 0)
        self.ctx.set_circuit_variant(self.variant)
        for k, v in HV.variant_weights(self.VARIANT, self.SHAPE[3]).items():
            self.ctx.set_weight(k, v)
        self.ctx.finalize(L.dtype_code("fp32_fft"))
        shape = self.SHAPE[:3] + (64,)
        self.out = {"O": _nan(shape), "I": _nan(shape)}

    def invoke(self):
        import hgru_variant_cases as HV
        i, o = self.inp, self.out
        self.ctx.circuit_fwd_var(i["x"], i["o0"], i["i0"], o["O"], o["I"], HV.T, _st(), self.variant)
        return dict(o)

    def check_plain(self, A, got):
        import hgru_variant_cases as HV
        ref = HV.oracle(self.VARIANT, self.SHAPE)
        for k, r in (("O", ref[0]), ("I", ref[1])):
            err = rel_inf(got[k], r)
            print(f"{self.name}: plain {k} rel_inf vs float64 {err:.3e}")
            assert err <= FP32_REL_TOL, (k, err)

    def close(self):
        self.ctx.close()


class CircuitNhwcFftCase(Case):
    """the channel-general loop with nhwc_conv='fft' at k = 8, n = 3 (circuit_channel_cases' weights)"""
    K, N, H, Wd, SSF, VARIANT = 8, 3, 9, 32, 5, "pose"
    name = "circuit_nhwc-fft-k8-n3"
    covers = ("mp_hgru_circuit_fwd_opts",)
    outputs = ("O",)

    def make(self, seed):
        import circuit_channel_cases as CC
        if seed == SEED_A:
            X, O0, _ = CC.inputs(self.K, self.N, self.H, self.Wd)
        else:       # the draw of a taller map, cut to this one
            X, O0, _ = (a[:, 1:self.H + 1] for a in CC.inputs(self.K, self.N, self.H + 2, self.Wd))
        return {"x": np.ascontiguousarray(X), "o0": np.ascontiguousarray(O0)}

    def alloc(self):
        import circuit_channel_cases as CC
        L = _L()
        self.ctx = L.Context(L.MP_MODEL_HGRU_CIRCUIT, 0)
        self.ctx.set_nhwc_conv(L.NHWC_CONVS["fft"])
        for k, v in CC.variant_weights(self.VARIANT, self.K, self.SSF).items():
            self.ctx.set_weight(k, v)
        self.ctx.finalize(L.dtype_code("fp32_split"))
        self.out = {"O": _nan((self.N, self.H, self.Wd, self.K))}

    def invoke(self):
        import circuit_channel_cases as CC
        self.ctx.circuit_fwd(self.inp["x"], self.inp["o0"], self.out["O"], CC.T, _st())
        return dict(self.out)

    def check_plain(self, A, got):
        import circuit_channel_cases as CC
        ref = CC.oracle(self.K, self.N, self.H, self.Wd, self.SSF, self.VARIANT)[0]
        err = rel_inf(got["O"], ref)
        print(f"{self.name}: plain O rel_inf vs float64 {err:.3e}")
        assert err <= FP32_REL_TOL, err

    def close(self):
        self.ctx.close()


_REG_GOLDEN = {"dense": "dense_c128", "hier": "hier_c128", "dense_hier": "dense_hier_c128", "cnn": "cnn_c128"}


class RegressorCase(Case):
    """dense / hier / dense_hier / cnn_model on the graph runtime (the multi-stream DAG and its replay), dense
    and hier also with use_graph=False; the golden cases' crops and weights (A is the golden input, so the
    plain result is held to the committed float64 vector)"""

    def __init__(self, kind, n=2, use_graph=True):
        self.kind, self.n, self.use_graph = kind, n, use_graph
        self.name = f"regressor-{kind}-n{n}" + ("" if use_graph else "-nograph")
        self.covers = ("mp_graph_fwd",) if use_graph else ({"dense": "mp_dense_fwd", "hier": "mp_hier_fwd"}[kind],)
        self.outputs = ("out",) if kind in ("dense", "cnn") else tuple(f"out{i}" for i in range(6))
        self.meta = golden_meta()[_REG_GOLDEN[kind]]

    def make(self, seed):
        return {"depth": _W().synth_crops(self.n, seed=self.meta["crop_seed"] + 500 * seed, size=self.meta["crop"])}

    def alloc(self):
        import torch
        P, m = pkg(), self.meta
        wts, _ = MG.regressor_inputs(self.kind, 1, m["crop"], m["weight_seed"], m["crop_seed"])
        if self.kind == "dense":
            self.model = P.train_dense_networks.dense_model_struct(use_graph=self.use_graph)
        elif self.kind == "hier":
            self.model = P.train_hier_networks.hier_model_struct(use_graph=self.use_graph)
        elif self.kind == "dense_hier":
            self.model = P.train_dense_hier_networks.dense_hier_model_struct()
        else:
            self.model = P.train_cnn_networks_hgru.cnn_model_struct()
        self.model.load_weights(wts)
        heads = (69,) if self.kind in ("dense", "cnn") else MG.HIER_HEADS
        self.model.build(self.inp["depth"], *heads, train_mode=False)      # the context, the plan, its streams
        torch.cuda.synchronize()

    def invoke(self):
        m = self.model
        out = m.forward(self.inp["depth"])
        if len(self.outputs) == 1:
            return {"out": out}
        return {f"out{i}": getattr(m, a) for i, a in enumerate(m.OUTPUT_ATTRS)}

    def check_plain(self, A, got):
        ref = golden_array(_REG_GOLDEN[self.kind], "out")
        out = got[self.outputs[0]][:ref.shape[0]]
        err = rel_inf(out, ref)
        print(f"{self.name}: plain output rows 0..{ref.shape[0] - 1} rel_inf vs the golden float64 vector {err:.3e}")
        assert err <= FP32_REL_TOL, err


class AttnCase(Case):
    """the attention net on 424 x 512 frames: the resize to 128 x 128 and the one-stream regressor"""
    name = "attn-n2-424x512"
    covers = ("mp_attn_fwd",)
    outputs = ("out",)

    def make(self, seed):
        m = golden_meta()["attn_f424"]
        return {"frames": _W().synth_frames(m["n"], seed=m["frame_seed"] + 500 * seed, h=m["h"], w=m["w"])}

    def alloc(self):
        import torch
        m = golden_meta()["attn_f424"]
        self.model = pkg().train_cnn_networks_hgru.attn_model_struct()
        self.model.load_weights(_W().attn_synth_weights(seed=m["weight_seed"]))
        self.model.build(self.inp["frames"], 3, train_mode=False)
        torch.cuda.synchronize()
        self.out = {"out": _nan((m["n"], 3))}

    def invoke(self):
        return {"out": self.model.forward(self.inp["frames"], out=self.out["out"])}

    def check_plain(self, A, got):
        err = rel_inf(got["out"], golden_array("attn_f424", "out"))
        print(f"{self.name}: plain rel_inf vs the golden float64 vector {err:.3e}")
        assert err <= FP32_REL_TOL, err


class AttnTapsCase(Case):
    """mp_attn_fwd_taps on 424 x 512 frames: every tap is a copy on the caller's stream between two launches
    that reuse its source buffer (attn_conv for conv2 .. conv5, the pool ping-pong), so a copy that ran
    elsewhere would read the next stage's data"""
    name = "attn-taps-n2-424x512"
    covers = ("mp_attn_fwd_taps",)
    TAP_SHAPES = {"resized": (128, 128, 1), "conv2": (64, 64, 128), "conv3": (32, 32, 256), "conv4": (16, 16, 512),
                  "conv5": (8, 8, 1024), "pool1": (64, 64, 64), "pool2": (32, 32, 128), "pool3": (16, 16, 256),
                  "pool4": (8, 8, 512), "pool5": (4, 4, 1024), "relu1": (1024,)}
    outputs = ("out",) + tuple(TAP_SHAPES)

    def make(self, seed):
        m = golden_meta()["attn_f424"]
        return {"frames": _W().synth_frames(m["n"], seed=m["frame_seed"] + 500 * seed, h=m["h"], w=m["w"])}

    def alloc(self):
        m = golden_meta()["attn_f424"]
        L = _L()
        assert tuple(self.TAP_SHAPES) == L.ATTN_TAP_NAMES
        self.ctx = L.Context(L.MP_MODEL_ATTN, 0)
        for k, v in _W().attn_synth_weights(seed=m["weight_seed"]).items():
            self.ctx.set_weight(k, v)
        self.ctx.finalize(L.dtype_code("fp32_split"))
        self.out = {"out": _nan((m["n"], 3))}
        self.out.update({k: _nan((m["n"],) + s) for k, s in self.TAP_SHAPES.items()})

    def invoke(self):
        taps = {k: v for k, v in self.out.items() if k != "out"}
        self.ctx.attn_fwd_taps(self.inp["frames"], self.out["out"], taps, _st())
        return dict(self.out)

    def check_plain(self, A, got):
        err = rel_inf(got["out"], golden_array("attn_f424", "out"))
        print(f"{self.name}: plain rel_inf vs the golden float64 vector {err:.3e}")
        assert err <= FP32_REL_TOL, err

    def close(self):
        self.ctx.close()


def _md(cam=CAM_REF):
    return pkg().monkeydetector.MonkeyDetector(*cam)


def _frames(n, seed, h, w, u16=False):
    """frames in mm [n, h, w]: float32 (integers and fractions) or uint16"""
    fn = np.ascontiguousarray(_W().synth_frames(n, seed=seed, h=h, w=w)[..., 0])
    mm = fn * np.float32(10000.0)
    return np.round(mm).astype(np.uint16) if u16 else mm.astype(np.float32)


class ComCase(Case):
    """MonkeyDetector.calculateCoM_device, 37 x 53, float32 or uint16 millimetres"""

    def __init__(self, u16):
        self.u16 = u16
        self.name = "com-" + ("u16" if u16 else "f32")
        self.covers = ("mp_center_of_mass_dev_dt",)
        self.outputs = ("coms",)

    def make(self, seed):
        return {"frames": _frames(3, 300 + seed, 37, 53, self.u16)}

    def alloc(self):
        self.md = _md(CAM_NEAR)

    def invoke(self):
        return {"coms": self.md.calculateCoM_device(self.inp["frames"])}

    def check_plain(self, A, got):
        ref = np.stack([self.md.calculateCoM(f) for f in A["frames"]])
        assert np.array_equal(got["coms"], ref)


class DetectCase(Case):
    """detect_crop_device(check=False): the detector's own CoM, then the crop around it, with and without
    the docom refinement; the pipeline's buffers through ``_buffers=``, pre-filled"""

    def __init__(self, u16, docom):
        self.u16, self.docom = u16, docom
        self.name = f"detect-{'u16' if u16 else 'f32'}" + ("-docom" if docom else "")
        self.covers = ("mp_center_of_mass_dev_dt", "mp_crop3d_dev_coms_dt")
        self.outputs = ("patches", "Ms", "coms")
        self.N, self.H, self.Wd, self.D = 2, 120, 160, 64

    def make(self, seed):
        return {"frames": _frames(self.N, 400 + seed, self.H, self.Wd, self.u16)}

    def alloc(self):
        self.md = _md(CAM_NEAR)
        self.buf = self.md._detect_buffers(self.N, self.H, self.Wd, self.D, self.inp["frames"].device, 1 if self.u16 else 0)
        self.out = {k: self.buf[k] for k in self.outputs}

    def invoke(self):
        p, M, c = self.md.detect_crop_device(self.inp["frames"], None, dsize=self.D, docom=self.docom, check=False,
                                             _buffers=self.buf)
        return {"patches": p, "Ms": M, "coms": c}

    def check_plain(self, A, got):
        md = self.md
        if not self.docom:
            hp, hM, hc = md.crop_batch(A["frames"], coms=None, dsize=self.D)
            assert np.array_equal(got["coms"], hc) and np.array_equal(got["Ms"], hM) and np.array_equal(got["patches"], hp)
            return
        for i in range(self.N):
            crop, hM, hc = md.cropArea3D(A["frames"][i], None, (self.D, self.D), docom=True)
            assert np.array_equal(got["coms"][i], hc) and np.array_equal(got["Ms"][i], np.asarray(hM))
            assert np.array_equal(got["patches"][i, ..., 0], crop / np.float32(md.maxDepth))


class DetectRawCase(Case):
    """the float32 forms the *_dt calls forward to, called as a C caller does: mp_center_of_mass_dev into
    mp_crop3d_dev_coms on one stream"""
    name = "detect-raw-f32"
    covers = ("mp_center_of_mass_dev", "mp_crop3d_dev_coms")
    outputs = ("patches", "Ms", "coms", "status")
    may_coincide = ("status",)
    N, H, Wd, D = 2, 120, 160, 64

    def make(self, seed):
        return {"frames": _frames(self.N, 400 + seed, self.H, self.Wd)}

    def alloc(self):
        import torch
        self.md = _md(CAM_NEAR)
        self.buf = self.md._detect_buffers(self.N, self.H, self.Wd, self.D, self.inp["frames"].device, 0)
        self.out = {k: self.buf[k] for k in self.outputs}
        self.lib = pkg().monkeydetector._lib_crop()
        torch.cuda.synchronize()

    def invoke(self):
        b, fr, cam = self.buf, self.inp["frames"], self.md._cam()
        st = ctypes.c_void_p(_st())
        _L().check(self.lib.mp_center_of_mass_dev(ctypes.byref(cam), _vp(fr), self.N, self.H, self.Wd, 1.0, _vp(b["coms0"]),
                                                  _vp(b["work"]), b["work_bytes"], st))
        _L().check(self.lib.mp_crop3d_dev_coms(ctypes.byref(cam), _vp(fr), self.N, self.H, self.Wd, 1.0, _vp(b["coms0"]), 0,
                                               self.D, _vp(b["patches"]), _vp(b["Ms"]), _vp(b["coms"]), _vp(b["status"]), st))
        return dict(self.out)

    def check_plain(self, A, got):
        hp, hM, hc = self.md.crop_batch(A["frames"], coms=None, dsize=self.D)
        assert np.array_equal(got["coms"], hc) and np.array_equal(got["Ms"], hM) and np.array_equal(got["patches"], hp)
        assert not got["status"].any()


class CropBatchCase(Case):
    """crop_batch_device(check=False): the crop around an attention output still on the device"""

    def __init__(self, docom, raw=False):
        self.docom, self.raw = docom, raw
        self.name = "crop_batch" + ("-docom" if docom else "") + ("-raw" if raw else "")
        self.covers = ("mp_crop3d_dev",) if raw else ("mp_crop3d_dev_ex",)
        self.outputs = ("patches", "Ms", "coms")
        self.N, self.H, self.Wd, self.D = 2, 120, 160, 64
        self.scale = (float(self.H), float(self.Wd), 10000.0)

    def make(self, seed):
        mm = _frames(self.N, 500 + seed, self.H, self.Wd)
        md = _md(CAM_NEAR)
        coms = np.stack([md.calculateCoM(f) for f in mm])
        return {"frames": (mm / np.float32(10000.0)).astype(np.float32),
                "com_norm": (coms / np.array(self.scale)).astype(np.float32)}

    def alloc(self):
        import torch
        self.md = _md(CAM_NEAR)
        if self.raw:
            dev = self.inp["frames"].device
            self.out = {"patches": _nan((self.N, self.D, self.D, 1)), "Ms": _nan((self.N, 3, 3), torch.float64),
                        "coms": _nan((self.N, 3), torch.float64)}
            self.status = torch.zeros((self.N,), dtype=torch.int32, device=dev)
            self.lib = pkg().monkeydetector._lib_crop()
            self.cscale = (ctypes.c_double * 3)(*self.scale)

    def invoke(self):
        i = self.inp
        if not self.raw:
            p, M, c = self.md.crop_batch_device(i["frames"], i["com_norm"], com_scale=self.scale, frame_scale=10000.0,
                                                dsize=self.D, check=False, docom=self.docom)
            return {"patches": p, "Ms": M, "coms": c}
        o, cam = self.out, self.md._cam()
        _L().check(self.lib.mp_crop3d_dev(ctypes.byref(cam), _vp(i["frames"]), self.N, self.H, self.Wd, 10000.0,
                                          _vp(i["com_norm"]), ctypes.cast(self.cscale, ctypes.c_void_p), self.D,
                                          _vp(o["patches"]), _vp(o["Ms"]), _vp(o["coms"]), _vp(self.status),
                                          ctypes.c_void_p(_st())))
        return dict(o)

    def check_plain(self, A, got):
        md = self.md
        mm = A["frames"] * np.float32(10000.0)
        coms = A["com_norm"].astype(np.float64) * np.array(self.scale)
        if not self.docom:
            hp, hM, hc = md.crop_batch(mm, coms=coms, dsize=self.D)
            assert np.array_equal(got["coms"], hc) and np.array_equal(got["Ms"], hM) and np.array_equal(got["patches"], hp)
            return
        for k in range(self.N):
            crop, hM, hc = md.cropArea3D(mm[k], coms[k], (self.D, self.D), docom=True)
            assert np.array_equal(got["coms"][k], hc) and np.array_equal(got["Ms"][k], np.asarray(hM))
            assert np.array_equal(got["patches"][k, ..., 0], crop / np.float32(md.maxDepth))


def _labels(n, J, seed):
    rs = np.random.RandomState(seed)
    lab = rs.uniform(-300.0, 300.0, (n, J, 3)).astype(np.float32)
    lab[..., 2] -= np.float32(1500.0)
    return lab


def _coms(n, seed):
    rs = np.random.RandomState(seed)
    return np.stack([rs.uniform(100, 400, n), rs.uniform(100, 300, n), rs.uniform(900, 2500, n)], axis=1)


class AbsJointsCase(Case):
    name = "abs_joints"
    covers = ("mp_abs_joints_dev",)
    outputs = ("xyz", "uvd")

    def make(self, seed):
        rs = np.random.RandomState(600 + seed)
        return {"pose": rs.uniform(-1.0, 1.0, (3, 69)).astype(np.float32), "coms": _coms(3, 610 + seed)}

    def alloc(self):
        self.md = _md()
        self.out = {"xyz": _nan((3, 23, 3)), "uvd": _nan((3, 23, 3))}

    def invoke(self):
        x, u = self.md.getAbsoluteCoordinates_device(self.inp["pose"], self.inp["coms"], out=(self.out["xyz"], self.out["uvd"]))
        return {"xyz": x, "uvd": u}

    def check_plain(self, A, got):
        half = np.float32(self.md.cube[2] / 2.0)
        for i in range(3):
            x, u = self.md.getAbsoluteCoordinates(A["pose"][i].reshape(-1, 3) * half, A["coms"][i])
            assert np.array_equal(got["xyz"][i], np.asarray(x)) and np.array_equal(got["uvd"][i], np.asarray(u))


class TransformJointsCase(Case):
    name = "transform_joints"
    covers = ("mp_transform_joints_dev",)
    outputs = ("out",)

    def make(self, seed):
        rs = np.random.RandomState(620 + seed)
        ju = np.stack([rs.uniform(0, 512, (3, 23)), rs.uniform(0, 424, (3, 23)), rs.uniform(800, 2000, (3, 23))],
                      axis=2).astype(np.float32)
        Ms = np.tile(np.eye(3), (3, 1, 1))
        Ms[:, :2, :2] *= rs.uniform(0.2, 0.9, (3, 1, 1))
        Ms[:, :2, 2] = rs.uniform(-100, 20, (3, 2))
        return {"joints_uvd": ju, "Ms": Ms}

    def alloc(self):
        self.md = _md()
        self.out = {"out": _nan((3, 23, 3))}

    def invoke(self):
        return {"out": self.md.transform_joints_device(self.inp["joints_uvd"], self.inp["Ms"], out=self.out["out"])}

    def check_plain(self, A, got):      # the header's rule in float64, not fused
        u, v = A["joints_uvd"][..., 0].astype(np.float64), A["joints_uvd"][..., 1].astype(np.float64)
        M = A["Ms"][:, None]
        t = [(u * M[..., i, 0] + v * M[..., i, 1]) + M[..., i, 2] for i in range(3)]
        ref = np.stack([(t[0] / t[2]).astype(np.float32), (t[1] / t[2]).astype(np.float32), A["joints_uvd"][..., 2]], axis=2)
        assert np.array_equal(got["out"], ref)


class ComFromJointsCase(Case):
    name = "com_from_joints"
    covers = ("mp_com_from_joints_dev",)
    outputs = ("com",)
    SCALE = (424.0, 512.0, 10000.0)

    def make(self, seed):
        return {"labels": _labels(3, 23, 630 + seed)}

    def alloc(self):
        self.md = _md()
        self.out = {"com": _nan((3, 3))}

    def invoke(self):
        return {"com": self.md.calculateCoMfrom3DJoints(self.inp["labels"], scale=self.SCALE, out=self.out["com"])}

    def check_plain(self, A, got):
        assert np.array_equal(got["com"], self.md.calculateCoMfrom3DJoints(A["labels"], scale=self.SCALE))


class RelLabelsCase(Case):
    name = "rel_labels"
    covers = ("mp_rel_labels_dev",)
    outputs = ("rel",)

    def make(self, seed):
        return {"labels": _labels(3, 23, 640 + seed), "coms": _coms(3, 650 + seed)}

    def alloc(self):
        self.md = _md()
        self.out = {"rel": _nan((3, 69))}

    def invoke(self):
        return {"rel": self.md.relative_labels_device(self.inp["labels"], self.inp["coms"], out=self.out["rel"])}

    def check_plain(self, A, got):
        assert np.array_equal(got["rel"], self.md.relative_labels(A["labels"], A["coms"]))


class RealFramesCase(Case):
    """preprocess_real_frames on a CUDA tensor: transposed uint16 recordings (the LDS tiles), float32 untransposed"""

    def __init__(self, u16):
        self.u16 = u16
        self.name = "real_frames-" + ("u16" if u16 else "f32")
        self.covers = ("mp_real_frames_dev",)
        self.outputs = ("out",)

    def make(self, seed):
        mm = _frames(2, 660 + seed, 70, 45, self.u16)      # [n, w, h] as stored when transposed
        return {"raw": mm}

    def alloc(self):
        self.out = {"out": _nan((2, 45, 70, 1) if self.u16 else (2, 70, 45, 1))}

    def invoke(self):
        f = pkg().monkeydetector.preprocess_real_frames
        return {"out": f(self.inp["raw"], transposed=self.u16, out=self.out["out"])}

    def check_plain(self, A, got):
        assert np.array_equal(got["out"], pkg().monkeydetector.preprocess_real_frames(A["raw"], transposed=self.u16))


class OverlayCase(Case):
    name = "overlay"
    covers = ("mp_overlay_dev",)
    outputs = ("rgb",)
    BONES = ((0, 1), (1, 2), (2, 3), (0, 4))

    def make(self, seed):
        rs = np.random.RandomState(670 + seed)
        fr = _frames(2, 675 + seed, 60, 80) / np.float32(10000.0)
        ju = np.stack([rs.uniform(-5, 85, (2, 2, 5)), rs.uniform(-5, 65, (2, 2, 5)), rs.uniform(0, 1, (2, 2, 5))],
                      axis=3).astype(np.float32)
        return {"frames": fr.astype(np.float32), "joints_uvd": ju}

    def alloc(self):
        import torch
        self.out = {"rgb": torch.full((2, 60, 80, 3), 255, dtype=torch.uint8, device="cuda")}

    def invoke(self):
        f = pkg().monkeydetector.render_overlays
        return {"rgb": f(self.inp["frames"], self.inp["joints_uvd"], bones=self.BONES, lut="jet", out=self.out["rgb"])}

    def check_plain(self, A, got):
        ref = pkg().monkeydetector.render_overlays_np(A["frames"], A["joints_uvd"], bones=self.BONES, lut="jet")
        assert np.array_equal(got["rgb"], ref)


class ResizeCase(Case):
    name = "resize_bilinear"
    covers = ("mp_resize_bilinear",)
    outputs = ("out",)

    def make(self, seed):
        return {"x": _W().sym_uniform(680 + seed, "x", (2, 37, 53, 3), 1.0)}

    def invoke(self):
        return {"out": _L().resize_bilinear(self.inp["x"], (16, 24))}

    def check_plain(self, A, got):      # TF's float32 kernel restated on the host: the same bits
        from oracle import regressors_ref as RR
        assert np.array_equal(got["out"], RR.resize_bilinear_tf1(A["x"], 16, 24))


class EvaluatorCase(Case):
    """PoseEvaluator.reset / update / update / the summary kernel: its device state carries across calls.
    (``summary_array`` itself ends with a host read; the case calls mp_eval_summary_dev as that method does
    and leaves the read to the harness's clone.)"""
    name = "evaluator"
    covers = ("mp_eval_reset_dev", "mp_eval_accumulate_dev", "mp_eval_summary_dev")
    outputs = ("summary", "dist", "frame_mean", "frame_max")
    J, T = 23, 16

    def make(self, seed):
        lab = _labels(5, self.J, 690 + seed)
        rs = np.random.RandomState(695 + seed)
        return {"labels": lab, "results": lab + rs.normal(0, 20, lab.shape).astype(np.float32)}

    def alloc(self):
        import torch
        PE = pkg().pose_evaluation
        self.ev = PE.PoseEvaluator(self.J, thresholds=np.arange(self.T) * 4.0)
        self.ev.update(self.inp["labels"], self.inp["results"])     # the state, the work buffer
        torch.cuda.synchronize()

    def invoke(self):
        ev, i = self.ev, self.inp
        ev.reset()
        ev.update(i["labels"][:2], i["results"][:2])
        ev.update(i["labels"][2:], i["results"][2:])
        _L().check(ev._lib().mp_eval_summary_dev(_vp(ev._state), ev.J, ev.T, _vp(ev._summary), ctypes.c_void_p(_st())))
        d, m, x = ev.last_frame_errors
        return {"summary": ev._summary, "dist": d, "frame_mean": m, "frame_max": x}

    def check_plain(self, A, got):
        d = A["labels"].astype(np.float32) - A["results"].astype(np.float32)
        dist = np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])
        assert np.array_equal(got["dist"], dist[2:])
        s = got["summary"]
        assert s[0] == 5 and s[1] == 5
        assert abs(s[2] - dist.mean(axis=1, dtype=np.float64).mean()) <= 1e-5 * s[2]
        assert s[3] == dist.max()


def _pose_model(crop, T, seed=1234):
    W = _W()
    pm = pkg().hgru_pose.model()
    wts = W.synth_weights(W.hgru_pose_vars(output_shape=69, timesteps=T, crop=crop), seed=seed, timesteps=T)
    pm.load_weights(wts)
    return pm, wts


class DetectorPipelineCase(Case):
    """DetectorPosePipeline.run with check_crops=False (no status read): CoM, crop, pose, joints on one stream"""

    def __init__(self, u16):
        self.u16 = u16
        self.name = "detector_pipeline-" + ("u16" if u16 else "f32")
        self.covers = ("mp_center_of_mass_dev_dt", "mp_crop3d_dev_coms_dt", "mp_hgru_pose_fwd", "mp_abs_joints_dev")
        self.outputs = ("xyz", "uvd", "coms", "Ms")
        self.N, self.H, self.Wd, self.D = 3, 120, 160, 64

    def make(self, seed):
        return {"frames": _frames(self.N, 700 + seed, self.H, self.Wd, self.u16),
                "o0": _W().synth_hidden((self.N, self.D // 2, self.D // 2, 64), seed=710 + seed)}

    def alloc(self):
        import torch
        T = pkg().train_cnn_networks_hgru
        self.md = _md(CAM_NEAR)
        self.pm, self.wts = _pose_model(self.D, 2)
        self.pm.build(torch.zeros((self.N, self.D, self.D, 1), device="cuda"), 69, h2_init=self.inp["o0"])
        self.pipe = T.DetectorPosePipeline(self.pm, self.md, dsize=self.D, check_crops=False)
        self.pipe.run(self.inp["frames"], h2_init=self.inp["o0"])      # its buffers
        torch.cuda.synchronize()

    def invoke(self):
        return dict(zip(self.outputs, self.pipe.run(self.inp["frames"], h2_init=self.inp["o0"])))

    def check_plain(self, A, got):
        import torch
        from oracle import hgru_ref as R
        md = self.md
        patches, Ms, coms = md.crop_batch(A["frames"], coms=None, dsize=self.D)
        assert np.array_equal(got["coms"], coms) and np.array_equal(got["Ms"], Ms)
        out = self.pm.forward(torch.from_numpy(patches).cuda(), h2_init=torch.from_numpy(A["o0"]).cuda()).cpu().numpy()
        ref = R.hgru_pose_forward(patches, self.wts, A["o0"].astype(np.float64), 2, np.float64)
        err = rel_inf(out, ref)
        print(f"{self.name}: pose on the host crops rel_inf vs float64 {err:.3e}")
        assert err <= FP32_REL_TOL, err
        half = np.float32(md.cube[2] / 2.0)
        for i in range(self.N):
            x, u = md.getAbsoluteCoordinates(out[i].reshape(-1, 3) * half, coms[i])
            assert np.array_equal(got["xyz"][i], np.asarray(x)) and np.array_equal(got["uvd"][i], np.asarray(u))


class FramePipelineCase(Case):
    """FramePosePipeline.run with check_crops=False: attention net, device crop, pose (tests/test_attn.py's
    pipeline test pins this shape against float64)"""
    name = "frame_pipeline"
    covers = ("mp_attn_fwd", "mp_crop3d_dev_ex", "mp_hgru_pose_fwd")
    outputs = ("out", "coms", "Ms")
    may_coincide = ("Ms",)      # integer crop bounds: two nearby CoMs give one transform

    def make(self, seed):
        m = golden_meta()["attn_f424"]
        return {"frames": _W().synth_frames(m["n"], seed=m["frame_seed"] + 500 * seed, h=m["h"], w=m["w"]),
                "o0": _W().synth_hidden((m["n"], 64, 64, 64), seed=7 + 50 * seed)}

    def alloc(self):
        import torch
        T = pkg().train_cnn_networks_hgru
        m = golden_meta()["attn_f424"]
        attn = T.attn_model_struct()
        attn.load_weights(_W().attn_synth_weights(seed=m["weight_seed"]))
        self.pipe = T.FramePosePipeline(attn, _pose_model(128, 2)[0], _md(), check_crops=False)
        self.pipe.run(self.inp["frames"], h2_init=self.inp["o0"])
        torch.cuda.synchronize()

    def invoke(self):
        return dict(zip(self.outputs, self.pipe.run(self.inp["frames"], h2_init=self.inp["o0"])))


def _factories():
    f = []
    for dt in ("fp32_fft", "bf16"):
        f += [lambda dt=dt: PoseCase(dt, 3), lambda dt=dt: PoseCase(dt, 64)]
    f += [lambda m=m: PoseCase("fp32_fft", 64, m) for m in ("taps", "states", "zeros", "identity", "random")]
    f += [lambda: CircuitCase(66, "opts", states=True), lambda: CircuitCase(3, "ex"), lambda: CircuitCase(3, "plain"),
          CircuitVarCase, CircuitNhwcFftCase]
    f += [lambda k=k: RegressorCase(k) for k in ("dense", "hier", "dense_hier", "cnn")]
    f += [lambda: RegressorCase("dense", 3), lambda: RegressorCase("dense", use_graph=False),
          lambda: RegressorCase("hier", use_graph=False), AttnCase, AttnTapsCase]
    f += [lambda: ComCase(False), lambda: ComCase(True)]
    f += [lambda u=u, d=d: DetectCase(u, d) for u in (False, True) for d in (False, True)]
    f += [DetectRawCase, lambda: CropBatchCase(False), lambda: CropBatchCase(True), lambda: CropBatchCase(False, raw=True)]
    f += [AbsJointsCase, TransformJointsCase, ComFromJointsCase, RelLabelsCase, lambda: RealFramesCase(True),
          lambda: RealFramesCase(False), OverlayCase, ResizeCase, EvaluatorCase]
    f += [lambda: DetectorPipelineCase(False), lambda: DetectorPipelineCase(True), FramePipelineCase]
    return f


def all_cases():
    return [f() for f in _factories()]


CASES = {c.name: f for c, f in zip(all_cases(), _factories())}
# again in a child process each (the switches are read once): four slices of 16, so ev_pre is re-recorded three
# times; and the backbone unstaggered, where a side slice waits for ev_fork alone (staggered, its wait for
# ev_pre -- recorded on the caller's stream behind slice 0's backbone -- orders it as well)
CHILD_CASE = "pose-fp32_fft-n64-plain"
CHILD_ENVS = ({"MP_STREAMS": "4", "MP_SLICE_MIN": "16"}, {"MP_BB_STAGGER": "0"})
TWO_CONTEXTS = ("pose-fp32_fft-n64-plain", "regressor-dense-n2")

# ---- the classification of every exported function with a stream argument --------------------------
# ordered: asynchronous on the caller's stream, held to that by the named GPU cases.
ORDERED = {}
for _c in all_cases():
    for _fn in _c.covers:
        ORDERED.setdefault(_fn, []).append(_c.name)
# synchronous: takes a stream but waits on the host, with the reason (none today: the waits are in the
# Python facades -- ContextualCircuit.build's trailing sync, the status read under check=True,
# PoseEvaluator.summary_array's read -- not in an exported function)
SYNCHRONOUS = {}
# diagnostic: not on a product path; they take no stream and synchronise
DIAGNOSTIC = {"mp_hbm_probe": "allocates, times and frees its own buffers; synchronous by design",
              "mp_profile_enable": "profiling keeps every launch on one stream",
              "mp_profile_read": "reading synchronises the profile's events"}


# ------------------------------------------------------------------------------------------ the harness
class Delay:
    """a chain of in-place adds on a 256 MiB buffer queued on the caller's stream"""

    def __init__(self):
        import torch
        self.buf = torch.zeros(DELAY_BYTES // 4, dtype=torch.float32, device="cuda")
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        self.enqueue(8)
        torch.cuda.synchronize()
        a.record()
        self.enqueue(64)
        b.record()
        torch.cuda.synchronize()
        self.ms_per_op = max(a.elapsed_time(b) / 64.0, 1e-3)

    def enqueue(self, ops):
        for _ in range(int(ops)):
            self.buf.add_(1.0)

    def block(self, ms):
        self.enqueue(int(np.ceil(ms / self.ms_per_op)))


_delays = []


def delay(i=0):
    while len(_delays) <= i:
        _delays.append(Delay())
    return _delays[i]


def _to_dev(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()      # a copy: shared inputs are read-only


def _host(outs):
    return {k: v.detach().cpu().numpy().copy() for k, v in outs.items()}


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _poison(case):
    import torch
    for t in getattr(case, "out", {}).values():
        if t.dtype.is_floating_point:
            t.fill_(float("nan"))
        else:
            t.fill_(torch.iinfo(t.dtype).max)


class Prepared:
    """a case with its device inputs, staging copies and plain results"""

    def __init__(self, case):
        import torch
        self.case = case
        self.A, self.B = case.make(SEED_A), case.make(SEED_B)
        assert set(self.A) == set(self.B)
        self.stage = {s: {k: _to_dev(v) for k, v in d.items()} for s, d in (("A", self.A), ("B", self.B))}
        case.inp = {k: v.clone() for k, v in self.stage["B"].items()}
        case.alloc()
        torch.cuda.synchronize()
        self.plain("A")                          # warm-up: workspace growth, planning, side-stream creation
        self.pA, self.pB = self.plain("A"), self.plain("B")
        assert set(self.pA) == set(case.outputs), (sorted(self.pA), case.outputs)
        for k in case.outputs:
            if k not in case.may_coincide:
                assert not _same(self.pA[k], self.pB[k]), f"{case.name}: plain(A) and plain(B) give the same {k}"
        case.check_plain(self.A, self.pA)

    def load(self, which):
        for k, t in self.case.inp.items():
            t.copy_(self.stage[which][k])

    def plain(self, which):
        import torch
        self.load(which)
        torch.cuda.synchronize()
        outs = self.case.invoke()
        torch.cuda.synchronize()
        return _host(outs)

    def clones(self):
        return {k: v.clone() for k, v in self.case.invoke().items()}

    def sequence(self, back_to_back):
        """the enqueues of one hazard run on torch's current stream -> the clones of each invoke"""
        self.load("A")                                                   # H1
        got = [self.clones()]                                            # H2
        self.load("B")                                                   # H3
        if back_to_back:                                                 # H4
            got.append(self.clones())
            self.load("A")
        return got

    def close(self):
        self.case.close()


def hazard_run(preps, streams, back_to_back, delay_ms):
    """one delayed run of each prepared case on its stream, enqueued interleaved (one case: the plain
    sequence) -> (per case the list of clone dicts as numpy, conclusive)"""
    import torch
    for p in preps:
        p.load("B")
        _poison(p.case)
    torch.cuda.synchronize()
    events, got = [], []
    for i, (p, s) in enumerate(zip(preps, streams)):
        with torch.cuda.stream(s):
            delay(i).block(delay_ms)
            e = torch.cuda.Event()
            e.record(s)
            events.append(e)
    for p, s in zip(preps, streams):
        with torch.cuda.stream(s):
            got.append(p.sequence(back_to_back))
    conclusive = not any(e.query() for e in events)
    torch.cuda.synchronize()
    return [[_host(g) for g in gs] for gs in got], conclusive


def check_hazards(preps, streams, label):
    """H1-H3 and H4 for the prepared cases on the given streams; raises on a mismatch or an inconclusive run"""
    import torch
    delay(len(preps) - 1)                     # every delay buffer exists (its calibration synchronises)
    for s, p in zip(streams, preps):          # a rehearsal without delay: the allocator's blocks of this stream
        with torch.cuda.stream(s):
            p.sequence(True)
    torch.cuda.synchronize()
    report = []
    for b2b, what in ((False, "H1-H3"), (True, "H4")):
        for ms in (DELAY_MS, 4 * DELAY_MS):
            got, conclusive = hazard_run(preps, streams, b2b, ms)
            if conclusive:
                break
        assert conclusive, f"{label} {what}: inconclusive: the call waited on the host"
        for p, gs in zip(preps, got):
            for g, ref, which in zip(gs, (p.pA, p.pB), "AB"):
                for k in p.case.outputs:
                    assert _same(g[k], ref[k]), \
                        f"{p.case.name} on {label}, {what}: {k} of the call on {which} differs from the plain run"
        report.append(f"{what} conclusive at {ms:.0f} ms")
    print(f"{' + '.join(p.case.name for p in preps)} on {label}: " + ", ".join(report))
    return report


def caller_streams():
    import torch
    return (("a fresh stream", torch.cuda.Stream()), ("the default stream", torch.cuda.default_stream()))


def run_case(name):
    prep = Prepared(CASES[name]())
    try:
        return {label: check_hazards([prep], [s], label) for label, s in caller_streams()}
    finally:
        prep.close()


def run_two_contexts():
    """a pose context on s1 and a dense graph context on s2, each behind its own delayed producer, enqueued
    interleaved; each must equal its plain run"""
    import torch
    preps = [Prepared(CASES[n]()) for n in TWO_CONTEXTS]
    try:
        return check_hazards(preps, [torch.cuda.Stream(), torch.cuda.Stream()], "two streams")
    finally:
        for p in preps:
            p.close()


def enqueue_ms(name, reps=5):
    """host milliseconds for invoke to return (the figure DELAY_MS is sized on)"""
    import time
    import torch
    prep = Prepared(CASES[name]())
    try:
        best = 1e9
        for _ in range(reps):
            torch.cuda.synchronize()
            t = time.perf_counter()
            prep.case.invoke()
            best = min(best, (time.perf_counter() - t) * 1e3)
        torch.cuda.synchronize()
        return best
    finally:
        prep.close()


if __name__ == "__main__":      # a child process of CHILD_ENVS: python stream_order_cases.py NAME
    if sys.argv[1] == "--enqueue":
        print(json.dumps({n: enqueue_ms(n) for n in sys.argv[2:]}))
    else:
        print(json.dumps({"report": run_case(sys.argv[1]), "ms_per_op": delay().ms_per_op}))
