"""Times the standalone circuit at n = 256, 64 x 64, ssf = 15, T = 8, fp32_fft, in one process:

  fused            the hgru_pose aux on its fused four-step loop (mp_hgru_circuit_fwd_ex)
  general_pose     the same aux on the general loop (mp_hgru_circuit_fwd_var)
  general_defaults the module's default aux (no gru_gates, no adaptation) on the general loop

Device events around one forward, warm-up, then the median of --runs forwards per form, the forms
alternating in rounds so that drift of a shared host hits all of them alike.  A second pass with the
library's per-launch event profile on gives the two epilogue kernels' times (var_in / var_out) and
the convs' (var_conv); each kernel's algorithmic bytes (maps read + written, from the variant)
over its time is stated as a fraction of mp_hbm_probe's copy rate taken in the same process.
One JSON goes to profiles/variants/, stamped with bench.tree_stamp.

    python tools/time_circuit_variants.py [--runs 20] [--batch 256] [--out profiles/variants/time_variants.json]

--kernels-only runs a few general-loop forwards and nothing else (the process to put under
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
POSE = {'gru_gates': True, 'adapation': True}


def kernel_bytes(aux, n, h, w, last):
    """algorithmic bytes of one launch of each epilogue kernel: fp32 maps read + written"""
    m = n * h * w * 64 * 4
    mely = aux['integration_type'] == 'mely'
    blend_in = aux['integration_type'] != 'control' and not aux['gru_gates']
    blend_out = mely or (aux['integration_type'] == 'alternate' and not aux['output_gru_gates'])
    rd_in = 2 + (0 if mely and not blend_in else 1) + (1 if blend_in or mely else 0)      # P, X, O, I
    wr_in = 1 + (1 if aux['output_gru_gates'] else 0)                                      # I', B_in
    rd_out = 2 + (1 if blend_out else 0)                                                   # P, I', O
    wr_out = 1 + (1 if last or aux['gru_gates'] else 0)                                    # O', A_in | out
    return (rd_in + wr_in) * m, (rd_out + wr_out) * m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--hw", type=int, default=64)
    ap.add_argument("--ssf", type=int, default=15)
    ap.add_argument("--timesteps", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "variants", "time_variants.json"))
    ap.add_argument("--kernels-only", action="store_true")
    a = ap.parse_args()
    import torch
    import bench
    mp = importlib.import_module("monkey-pose_amd")
    L, W, M = mp._lib, mp.weights, mp.hgru_module
    n, hw, T = a.batch, a.hw, a.timesteps
    dev = torch.device("cuda", 0)
    st = L.current_stream(dev)
    x = torch.from_numpy(W.synth_hidden((n, hw, hw, 64), seed=3, name="X", limit=1.0)).to(dev)
    o0 = torch.from_numpy(W.synth_hidden((n, hw, hw, 64), seed=7)).to(dev)
    i0 = torch.from_numpy(W.synth_hidden((n, hw, hw, 64), seed=1007)).to(dev)
    out, iout = torch.empty_like(x), torch.empty_like(x)

    def context(aux_over, general):
        aux = M.merged_aux(aux_over)
        table = W.hgru_circuit_vars(k=64, ssf=a.ssf, timesteps=T, scope="contextual_circuit", **M.variable_flags(aux))
        ctx = L.Context(L.MP_MODEL_HGRU_CIRCUIT, 0)
        var = L.circuit_variant(aux) if general else None
        if general:
            ctx.set_circuit_variant(var)
        for v in table:
            ctx.set_weight(v.name, W.synth_value(v, 1234, T))
        ctx.finalize(L.MP_DTYPE_F32_FFT)
        ctx.reserve(n)
        if general:
            return ctx, aux, lambda: ctx.circuit_fwd_var(x, o0, i0, out, iout, T, st, var)
        return ctx, aux, lambda: ctx.circuit_fwd(x, o0, out, T, st)

    forms = {"fused": context(POSE, False), "general_pose": context(POSE, True),
             "general_defaults": context({}, True)}
    if a.kernels_only:
        for name in ("general_pose", "general_defaults"):
            for _ in range(3):
                forms[name][2]()
        torch.cuda.synchronize()
        print("kernels-only: 3 forwards of each general-loop form")
        return
    assert forms["fused"][0].info("fft_loop") == 4 and forms["general_pose"][0].info("fft_loop") == 6
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
    res = {"tree": bench.tree_stamp(), "batch": n, "hw": [hw, hw], "ssf": a.ssf, "timesteps": T, "dtype": "fp32_fft",
           "runs": a.runs, "warmup": a.warmup, "device": torch.cuda.get_device_name(0), "forward_ms": {}}
    for k, ts in times.items():
        res["forward_ms"][k] = {"p50": round(float(np.median(ts)), 4), "min": round(min(ts), 4),
                                "max": round(max(ts), 4)}
    # the general pose output against the fused one (same inputs): the fp32-class gate's scale
    forms["fused"][2]()
    torch.cuda.synchronize()
    ref = out.clone()
    forms["general_pose"][2]()
    torch.cuda.synchronize()
    res["general_vs_fused_rel_inf"] = float((out - ref).abs().max() / ref.abs().max())
    # per-kernel times from the library's event profile (a pass of its own: the events serialise launches)
    probe = L.hbm_probe(0)
    res["hbm_probe"] = probe
    res["kernels"] = {}
    for name in ("general_pose", "general_defaults"):
        ctx, aux, fn = forms[name]
        ctx.profile(True)
        per = {"var_in": [], "var_out": [], "var_conv": []}
        for _ in range(a.runs):
            fn()
            torch.cuda.synchronize()
            for key in per:
                ms, cnt = ctx.profile_read(key)
                per[key].append(ms / max(cnt, 1))
        ctx.profile(False)
        b_in, b_out = kernel_bytes(aux, n, hw, hw, last=False)
        k = {}
        for key, nbytes in (("var_in", b_in), ("var_out", b_out)):
            ms = float(np.median(per[key]))
            gbps = nbytes / (ms * 1e-3) / 1e9
            k[key] = {"ms_per_launch_p50": round(ms, 4), "algorithmic_bytes": nbytes, "GBps": round(gbps, 1),
                      "fraction_of_probe_copy": round(gbps / probe["copy_GBps"], 3)}
        k["var_conv"] = {"ms_per_conv_p50": round(float(np.median(per["var_conv"])), 4)}
        res["kernels"][name] = k
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
