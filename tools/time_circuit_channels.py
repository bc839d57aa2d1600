"""Times the channel-general circuit loop at n = 64, 64 x 64 (--hw H or HxW), ssf = 15, T = 8, fp32_split, in one
process, for the hgru_pose aux and the module's default aux (both through mp_hgru_circuit_fwd_var):

  k32, k128     32 and 128 channels on the channel-general loop
  k64_nhwc      64 channels on the channel-general loop (mp_circuit_set_nhwc_loop)
  k64_general   64 channels on the general loop (k_conv64x3.hip + k_circuit_var.hip): the reference time
  k32_fft, k64_nhwc_fft, k128_fft   the same contexts with the FFT association-field conv
                (mp_circuit_set_nhwc_conv MP_CN_CONV_FFT, k_circuit_fft.hip)
  k32_fft_tiled, k64_nhwc_fft_tiled, k128_fft_tiled   the tiled FFT conv (MP_CN_CONV_FFT_TILED):
                maps of any size; on a map above 64 x 64 the forms that refuse it ('fft', the general
                loop's fp32_fft) are left out
  k64_general_fft   64 channels on the general loop's fp32_fft (k_fft.hip)

Device events around one forward, warm-up, then the median of --runs forwards per form, the forms
alternating in rounds so that drift of a shared host hits all of them alike.  A second pass with the
library's per-launch event profile on gives, for k = 32, 64 and 128 on the new loop, the time of the two
epilogue kernels (cn_in / cn_out), of the gate multiply (cn_gate) and of the convs (cn_conv,
cn_gate_conv; cn_fft_fwd, cn_spec_gemm, cn_fft_inv on the FFT forms) and the convs' share of the forward;
each epilogue kernel's algorithmic bytes (maps read + written, from the variant and the shapes) and each
FFT-conv kernel's (map + spectrum for the transforms, S + Y + weights for the product) over its time is
stated as a fraction of mp_hbm_probe's copy rate taken in the same process.  --forms limits the run to
some forms (ssf 3 and 5 are timed at k = 64 only).  One JSON goes to profiles/channels/, stamped with
bench.tree_stamp.

    python tools/time_circuit_channels.py [--runs 10] [--batch 64] [--out profiles/channels/time_channels.json]

--kernels-only runs a few forwards of each new-loop form and nothing else (the process to put under
rocprofv3 --kernel-trace --stats).
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
AUX = {"pose": {'gru_gates': True, 'adapation': True}, "defaults": {}}
# name, k, on the channel-general loop, its conv ('direct' / 'fft' / 'fft_tiled'), compute dtype
FORMS = (("k32", 32, True, "direct", "fp32_split"), ("k32_fft", 32, True, "fft", "fp32_split"),
         ("k32_fft_tiled", 32, True, "fft_tiled", "fp32_split"),
         ("k128", 128, True, "direct", "fp32_split"), ("k128_fft", 128, True, "fft", "fp32_split"),
         ("k128_fft_tiled", 128, True, "fft_tiled", "fp32_split"),
         ("k64_nhwc", 64, True, "direct", "fp32_split"), ("k64_nhwc_fft", 64, True, "fft", "fp32_split"),
         ("k64_nhwc_fft_tiled", 64, True, "fft_tiled", "fp32_split"),
         ("k64_general", 64, False, "direct", "fp32_split"), ("k64_general_fft", 64, False, "direct", "fp32_fft"))
PROFILE_KEYS = ("cn_in", "cn_out", "cn_gate", "cn_conv", "cn_gate_conv", "cn_fft_fwd", "cn_spec_gemm", "cn_fft_inv")
CONV_KEYS = ("cn_conv", "cn_gate_conv", "cn_fft_fwd", "cn_spec_gemm", "cn_fft_inv")
NF = 72 * 37


def tiles(L, ssf):
    """circuit_fft.hpp cnf_tiles: windows along an axis of length L"""
    return 1 if L <= 64 else -(-L // (64 - 2 * (ssf // 2)))


def fft_conv_bytes(n, h, w, k, T, ssf):
    """algorithmic bytes of the 2 T launches of each FFT-conv kernel in one forward (circuit_fft.hpp): the
    map and one spectrum per window for a transform; S, Y and the compact weights for the product"""
    m = n * h * w * k * 4
    spec = n * tiles(h, ssf) * tiles(w, ssf) * (k // 4) * NF * 32
    wts = NF * 2 * ((k // 4 + 1) // 2 * 2) * ((k + 31) // 32 * 32) * 16
    return {"cn_fft_fwd": 2 * T * (m + spec), "cn_fft_inv": 2 * T * (m + spec), "cn_spec_gemm": 2 * T * (2 * spec + wts)}


def fft_conv_flops(n, k, T):
    """real flops of the spectral product's 2 T launches as issued: 3 products (f16x3) of 2k x 2k x n per
    frequency, n the batch's windows"""
    return 2 * T * 3 * 2 * (2 * k) * (2 * k) * n * NF


def kernel_bytes(aux, n, h, w, k, T):
    """algorithmic bytes of the T launches of each epilogue kernel in one forward: fp32 maps read + written"""
    m = n * h * w * k * 4
    mely = aux['integration_type'] == 'mely'
    blend_in = aux['integration_type'] != 'control' and not aux['gru_gates']
    blend_out = mely or (aux['integration_type'] == 'alternate' and not aux['output_gru_gates'])
    rd_in = 2 + (0 if mely else 1) + (1 if blend_in or mely else 0) + (1 if blend_in else 0)   # P, X, O, I, g1p
    rd_out = 2 + (2 if blend_out else 0)                                                        # P, I', O, g2p
    return (rd_in + 1) * m * T, ((rd_out + 1) * T + 1) * m      # + I';  + O' and, on the last step, the result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--hw", default="64", help="map size: H (square) or HxW")
    ap.add_argument("--ssf", type=int, default=15)
    ap.add_argument("--timesteps", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "channels", "time_channels.json"))
    ap.add_argument("--forms", default="", help="comma-separated form names (default: all)")
    ap.add_argument("--kernels-only", action="store_true")
    a = ap.parse_args()
    import torch
    import bench
    mp = importlib.import_module("monkey-pose_amd")
    L, W, M = mp._lib, mp.weights, mp.hgru_module
    n, T = a.batch, a.timesteps
    h, w = (int(v) for v in (a.hw.split("x") if "x" in a.hw else (a.hw, a.hw)))
    ntile = tiles(h, a.ssf) * tiles(w, a.ssf)
    dev = torch.device("cuda", 0)
    st = L.current_stream(dev)
    bufs = {}
    chosen = [f for f in FORMS if not a.forms or f[0] in a.forms.split(",")]
    if max(h, w) > 64:      # 'fft' and the general loop's fp32_fft take maps up to 64 x 64
        chosen = [f for f in chosen if f[3] != "fft" and f[4] != "fp32_fft"]
    for k in sorted({f[1] for f in chosen}):
        x = torch.from_numpy(W.synth_hidden((n, h, w, k), seed=3, name="X", limit=1.0)).to(dev)
        o0 = torch.from_numpy(W.synth_hidden((n, h, w, k), seed=7)).to(dev)
        i0 = torch.from_numpy(W.synth_hidden((n, h, w, k), seed=1007)).to(dev)
        bufs[k] = (x, o0, i0, torch.empty_like(x), torch.empty_like(x))

    def context(aux_name, k, nhwc, conv, dtype):
        aux = M.merged_aux(AUX[aux_name])
        table = W.hgru_circuit_vars(k=k, ssf=a.ssf, timesteps=T, scope="contextual_circuit", **M.variable_flags(aux))
        ctx = L.Context(L.MP_MODEL_HGRU_CIRCUIT, 0)
        var = L.circuit_variant(aux)
        ctx.set_circuit_variant(var)
        if nhwc and k == 64:
            ctx.set_nhwc_loop(True)
        if conv != "direct":
            ctx.set_nhwc_conv(L.NHWC_CONVS[conv])
        for v in table:
            ctx.set_weight(v.name, W.synth_value(v, 1234, T))
        ctx.finalize(L.dtype_code(dtype))
        assert ctx.info("channels") == k and ctx.info("nhwc_loop") == int(nhwc)
        assert ctx.info("nhwc_conv") == L.NHWC_CONVS[conv]      # 0 direct, 1 fft, 2 fft_tiled
        x, o0, i0, out, iout = bufs[k]
        return ctx, aux, lambda: ctx.circuit_fwd_var(x, o0, i0, out, iout, T, st, var)

    forms = {f"{an}/{name}": context(an, k, nhwc, conv, dtype) + (k, nhwc)
             for an in AUX for name, k, nhwc, conv, dtype in chosen}
    if a.kernels_only:
        for name, f in forms.items():
            if f[4]:
                for _ in range(2):
                    f[2]()
        torch.cuda.synchronize()
        print("kernels-only: 2 forwards of each form of the channel-general loop")
        return
    for _ in range(a.warmup):
        for f in forms.values():
            f[2]()
    torch.cuda.synchronize()
    times = {k: [] for k in forms}
    for _ in range(a.runs):
        for k, f in forms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f[2]()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1))
    res = {"tree": bench.tree_stamp(), "batch": n, "hw": [h, w], "fft_tiles_per_image": ntile, "ssf": a.ssf, "timesteps": T,
           "dtype": {f[0]: f[4] for f in chosen},
           "runs": a.runs, "warmup": a.warmup, "device": torch.cuda.get_device_name(0), "forward_ms": {}}
    for k, ts in times.items():
        res["forward_ms"][k] = {"p50": round(float(np.median(ts)), 4), "min": round(min(ts), 4),
                                "max": round(max(ts), 4)}
    # the two loops' 64-channel outputs against each other (same inputs): the fp32-class gate's scale
    res["k64_vs_general_rel_inf"] = {}
    for an in AUX:
        if f"{an}/k64_general" not in forms:
            continue
        out = bufs[64][3]
        forms[f"{an}/k64_general"][2]()
        torch.cuda.synchronize()
        ref = out.clone()
        for other in ("k64_nhwc", "k64_nhwc_fft", "k64_nhwc_fft_tiled", "k64_general_fft"):
            if f"{an}/{other}" in forms:
                forms[f"{an}/{other}"][2]()
                torch.cuda.synchronize()
                res["k64_vs_general_rel_inf"][f"{an}/{other}"] = float((out - ref).abs().max() / ref.abs().max())
    # per-kernel times from the library's event profile (a pass of its own: the events serialise launches)
    probe = L.hbm_probe(0)
    res["hbm_probe"] = probe
    res["kernels"] = {}
    for name, (ctx, aux, fn, k, nhwc) in forms.items():
        if not nhwc:
            continue
        ctx.profile(True)
        per = {key: [] for key in PROFILE_KEYS}
        cnts = {}
        for _ in range(a.runs):
            fn()
            torch.cuda.synchronize()
            for key in per:
                ms, cnt = ctx.profile_read(key)
                per[key].append(ms)
                cnts[key] = cnt
        ctx.profile(False)
        fwd = {key: float(np.median(v)) for key, v in per.items()}      # ms per forward, all launches of the key
        total = sum(fwd.values())
        kk = {"launches_per_forward": cnts, "ms_per_forward": {key: round(v, 4) for key, v in fwd.items()},
              "profiled_forward_ms": round(total, 4),
              "conv_share_of_forward": round(sum(fwd[key] for key in CONV_KEYS) / total, 4)}
        b_in, b_out = kernel_bytes(aux, n, h, w, k, T)
        rated = [("cn_in", b_in, T), ("cn_out", b_out, T)]
        if fwd["cn_spec_gemm"] > 0:
            rated += [(key, nb, 2 * T) for key, nb in fft_conv_bytes(n, h, w, k, T, a.ssf).items()]
            kk["cn_spec_gemm_TFLOPs_issued"] = round(fft_conv_flops(n * ntile, k, T) / (fwd["cn_spec_gemm"] * 1e-3) / 1e12, 2)
        for key, nbytes, launches in rated:
            gbps = nbytes / (fwd[key] * 1e-3) / 1e9
            kk[key] = {"ms_per_launch_p50": round(fwd[key] / launches, 4), "algorithmic_bytes_per_forward": nbytes,
                       "GBps": round(gbps, 1), "fraction_of_probe_copy": round(gbps / probe["copy_GBps"], 3)}
        res["kernels"][name] = kk
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
