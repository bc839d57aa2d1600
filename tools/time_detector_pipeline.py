"""Times the detector path (SURVEY config 5 for a batch) from host float32 frames
(weights.synth_frames), at B = 256 and B = 1, p50 over --calls calls after warm-up:

  (a) host chain  crop_batch (16 threads) -> H2D -> pose.forward -> D2H -> getAbsoluteCoordinates
                  per frame: the only way to run the detector path before DetectorPosePipeline
                  (at B = 1 also StreamPosePipeline, the product class for that case)
  (b) device      DetectorPosePipeline.run including the H2D of the frames (from the pageable numpy
                  array, and from a pinned staging buffer) and with the frames already resident
  (c) kernels     mp_center_of_mass_dev and resize_bilinear_kernel alone on the same resident frames
                  (device events), with GB/s over the n * h * w * 4 bytes both read, next to
                  mp_hbm_probe's read rate

--dtype u16 times the same rows from uint16 frames in mm (the camera's own dtype: the frames above
rounded to whole millimetres, frame_scale 1): the host chain is crop_batch on the uint16 frames,
the uploads carry half the bytes, and (c) times the uint16 CoM kernels.  The float32 pipeline
(pageable upload, and resident) and the float32 CoM kernels are timed in the same process and the
same alternating rounds on the same frames as float32 mm, as rows f32_*, so that each uint16 row
has its float32 counterpart from the same run; the resize kernel and the B = 1 step are left to
the float32 run.  Default output: profiles/detector/time_detector_u16_run.json.

Host-clock timings end in a device synchronise.  Every step runs in a child process of its own under
its own time limit, and the first failure stops the run; the parent never touches the GPU.  One JSON
goes to profiles/detector/, stamped with bench.tree_stamp.

    python tools/time_detector_pipeline.py [--calls 200] [--dtype {f32,u16}] [--out profiles/detector/time_detector.json]
"""
import argparse
import ctypes
import importlib
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CAM = (365.456, 365.456, 256, 212, [800, 800, 1200], 200, 2500)   # near range: the CoM is on the body
STEP_LIMIT_S = {"b256": 420, "b1": 240, "hbm": 180}


def p50(ts):
    return float(np.median(ts))


def host_timed(fn, calls, warm, sync):
    for _ in range(warm):
        fn()
    sync()
    ts = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        sync()
        ts.append((time.perf_counter() - t0) * 1e3)
    return ts


def event_timed(fn, calls, warm, torch):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(calls)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return p50([a.elapsed_time(b) for a, b in ev])


def step_batch(B, calls):
    import torch
    mp = importlib.import_module("monkey-pose_amd")
    W, L = mp.weights, mp._lib
    T = mp.train_cnn_networks_hgru
    dev = torch.device("cuda", 0)
    md = mp.monkeydetector.MonkeyDetector(*CAM)
    base = W.synth_frames(min(B, 16), seed=14)[..., 0]
    fn = np.ascontiguousarray(base[np.arange(B) % base.shape[0]])          # [B, 424, 512] normalised, pageable
    fmm = fn * np.float32(10000.0)
    n, h, w = fn.shape
    pm = mp.hgru_pose.model()
    pm.load_weights(W.synth_weights(W.hgru_pose_vars(output_shape=69, timesteps=8, crop=128), seed=21))
    o0 = torch.from_numpy(W.synth_hidden((B, 64, 64, 64), seed=3)).to(dev)
    pm.build(torch.zeros((B, 128, 128, 1), device=dev), 69, h2_init=o0)
    sync = lambda: torch.cuda.synchronize(dev)
    warm = max(10, calls // 10)
    res = {"batch": B, "calls": calls, "frame_hw": [h, w]}

    # (a) the host chain
    patches_host = np.empty((B, 128, 128, 1), np.float32)
    half = np.float32(md.cube[2] / 2.0)

    def host_chain():
        _, _, coms = md.crop_batch(fmm, None, dsize=128, nthreads=16, out=patches_host)
        out = pm.forward(torch.from_numpy(patches_host).to(dev), h2_init=o0).cpu().numpy()
        return [md.getAbsoluteCoordinates(out[i].reshape(23, 3) * half, coms[i]) for i in range(B)]

    # (b) the device pipeline
    pipe = T.DetectorPosePipeline(pm, md, frame_scale=10000.0)
    fn_t = torch.from_numpy(fn)
    pinned = torch.empty_like(fn_t).pin_memory()
    pinned.copy_(fn_t)
    stage = torch.empty((B, h, w), dtype=torch.float32, device=dev)
    resident = fn_t.to(dev)

    def dev_pageable():
        stage.copy_(fn_t)
        return pipe.run(stage, h2_init=o0)

    def dev_pinned():
        stage.copy_(pinned, non_blocking=True)
        return pipe.run(stage, h2_init=o0)

    def dev_resident():
        return pipe.run(resident, h2_init=o0)

    # the two chains agree before anything is timed
    ref = host_chain()
    xyz, uvd, _, _ = dev_pageable()
    xyz, uvd = xyz.cpu().numpy(), uvd.cpu().numpy()
    res["device_equals_host_chain"] = bool(all(np.array_equal(xyz[i], ref[i][0]) and np.array_equal(uvd[i], ref[i][1])
                                               for i in range(B)))
    # alternate the forms in rounds so that drift of the shared host hits all of them alike
    rounds = 4
    per = -(-calls // rounds)
    acc = {k: [] for k in ("host_chain", "device_h2d_pageable", "device_h2d_pinned", "device_resident")}
    fns = dict(host_chain=host_chain, device_h2d_pageable=dev_pageable, device_h2d_pinned=dev_pinned,
               device_resident=dev_resident)
    if B == 1:
        sp = T.StreamPosePipeline(pm, md, h2_init=o0)
        fns["stream_pose_pipeline"] = lambda: sp.run(fmm[0])
        acc["stream_pose_pipeline"] = []
    for r in range(rounds):
        for k, f in fns.items():
            acc[k].append(host_timed(f, per, warm if r == 0 else 3, sync))
    for k, v in acc.items():
        ms = p50(np.concatenate(v))
        res[k] = {"p50_ms": round(ms, 4), "frames_per_s": round(B / ms * 1e3, 1), "samples": int(sum(len(x) for x in v)),
                  "round_p50_ms": [round(p50(x), 4) for x in v]}
    res["gate_device_h2d_pageable_over_host_chain"] = round(res["host_chain"]["p50_ms"] /
                                                            res["device_h2d_pageable"]["p50_ms"], 3)
    res["device_h2d_pinned_over_host_chain"] = round(res["host_chain"]["p50_ms"] / res["device_h2d_pinned"]["p50_ms"], 3)
    res["device_resident_over_host_chain"] = round(res["host_chain"]["p50_ms"] / res["device_resident"]["p50_ms"], 3)

    # (c) the two kernels alone, device events
    b = md._detect_buffers(n, h, w, 128, dev)
    st = L.current_stream(dev)
    com_ms = event_timed(lambda: md._com_into(resident, 10000.0, b["coms0"], b["work"], b["work_bytes"], st), calls,
                         warm, torch)
    out = torch.empty((n, 128, 128, 1), dtype=torch.float32, device=dev)
    lib = L.load()
    rs_ms = event_timed(lambda: L.check(lib.mp_resize_bilinear(resident.data_ptr(), n, h, w, 1, 128, 128,
                                                                out.data_ptr(), ctypes.c_void_p(st))), calls, warm,
                        torch)
    nbytes = n * h * w * 4
    res["com_kernels"] = {"p50_ms": round(com_ms, 5), "GBps": round(nbytes / com_ms / 1e6, 1)}
    res["resize_bilinear_kernel"] = {"p50_ms": round(rs_ms, 5), "GBps_over_frame_bytes": round(nbytes / rs_ms / 1e6, 1)}
    res["com_over_resize"] = round(com_ms / rs_ms, 3)
    res["frame_bytes"] = nbytes
    return res


def step_batch_u16(B, calls):
    """step_batch from uint16 frames, each row beside its float32 counterpart of the same process"""
    import torch
    mp = importlib.import_module("monkey-pose_amd")
    W, L = mp.weights, mp._lib
    T = mp.train_cnn_networks_hgru
    dev = torch.device("cuda", 0)
    md = mp.monkeydetector.MonkeyDetector(*CAM)
    base = W.synth_frames(min(B, 16), seed=14)[..., 0]
    fn = np.ascontiguousarray(base[np.arange(B) % base.shape[0]])
    fu = np.round(fn * np.float32(10000.0)).astype(np.uint16)             # [B, 424, 512] whole mm, pageable
    ff = fu.astype(np.float32)                                             # the same frames as float32 mm
    n, h, w = fu.shape
    pm = mp.hgru_pose.model()
    pm.load_weights(W.synth_weights(W.hgru_pose_vars(output_shape=69, timesteps=8, crop=128), seed=21))
    o0 = torch.from_numpy(W.synth_hidden((B, 64, 64, 64), seed=3)).to(dev)
    pm.build(torch.zeros((B, 128, 128, 1), device=dev), 69, h2_init=o0)
    sync = lambda: torch.cuda.synchronize(dev)
    warm = max(10, calls // 10)
    res = {"batch": B, "calls": calls, "frame_hw": [h, w], "dtype": "u16"}

    patches_host = np.empty((B, 128, 128, 1), np.float32)
    half = np.float32(md.cube[2] / 2.0)

    def host_chain():
        _, _, coms = md.crop_batch(fu, None, dsize=128, nthreads=16, out=patches_host)
        out = pm.forward(torch.from_numpy(patches_host).to(dev), h2_init=o0).cpu().numpy()
        return [md.getAbsoluteCoordinates(out[i].reshape(23, 3) * half, coms[i]) for i in range(B)]

    pipe_u, pipe_f = T.DetectorPosePipeline(pm, md), T.DetectorPosePipeline(pm, md)   # frames in mm
    fu_t, ff_t = torch.from_numpy(fu), torch.from_numpy(ff)
    pinned = torch.empty_like(fu_t).pin_memory()
    pinned.copy_(fu_t)
    stage_u = torch.empty((B, h, w), dtype=torch.uint16, device=dev)
    stage_f = torch.empty((B, h, w), dtype=torch.float32, device=dev)
    res_u, res_f = fu_t.to(dev), ff_t.to(dev)

    def dev_pageable():
        stage_u.copy_(fu_t)
        return pipe_u.run(stage_u, h2_init=o0)

    def dev_pinned():
        stage_u.copy_(pinned, non_blocking=True)
        return pipe_u.run(stage_u, h2_init=o0)

    def f32_pageable():
        stage_f.copy_(ff_t)
        return pipe_f.run(stage_f, h2_init=o0)

    ref = host_chain()
    xyz, uvd, _, _ = dev_pageable()
    xyz, uvd = xyz.cpu().numpy(), uvd.cpu().numpy()
    res["device_equals_host_chain"] = bool(all(np.array_equal(xyz[i], ref[i][0]) and np.array_equal(uvd[i], ref[i][1])
                                               for i in range(B)))
    fns = dict(host_chain=host_chain, device_h2d_pageable=dev_pageable, device_h2d_pinned=dev_pinned,
               device_resident=lambda: pipe_u.run(res_u, h2_init=o0), f32_device_h2d_pageable=f32_pageable,
               f32_device_resident=lambda: pipe_f.run(res_f, h2_init=o0))
    rounds = 4
    per = -(-calls // rounds)
    acc = {k: [] for k in fns}
    for r in range(rounds):
        for k, f in fns.items():
            acc[k].append(host_timed(f, per, warm if r == 0 else 3, sync))
    for k, v in acc.items():
        ms = p50(np.concatenate(v))
        res[k] = {"p50_ms": round(ms, 4), "frames_per_s": round(B / ms * 1e3, 1), "samples": int(sum(len(x) for x in v)),
                  "round_p50_ms": [round(p50(x), 4) for x in v]}
    for k in ("device_h2d_pageable", "device_h2d_pinned", "device_resident"):
        res[k + "_over_host_chain"] = round(res["host_chain"]["p50_ms"] / res[k]["p50_ms"], 3)
    rp = res["f32_device_h2d_pageable"]["round_p50_ms"]
    saved = res["f32_device_h2d_pageable"]["p50_ms"] - res["device_h2d_pageable"]["p50_ms"]
    res["h2d_pageable_saved_ms_vs_f32"] = round(saved, 4)
    res["f32_h2d_pageable_round_spread_ms"] = round(max(rp) - min(rp), 4)
    res["h2d_pageable_gain_over_f32"] = bool(saved > max(rp) - min(rp))     # else a tie

    # (c) the CoM kernels alone, uint16 beside float32, device events
    st = L.current_stream(dev)
    bu = md._detect_buffers(n, h, w, 128, dev, mp.monkeydetector.DEPTH_U16)
    bf = md._detect_buffers(n, h, w, 128, dev)
    u_ms, f_ms = [], []
    for _ in range(2):                                                       # alternated
        u_ms.append(event_timed(lambda: md._com_into(res_u, 1.0, bu["coms0"], bu["work"], bu["work_bytes"], st,
                                                     mp.monkeydetector.DEPTH_U16), calls, warm, torch))
        f_ms.append(event_timed(lambda: md._com_into(res_f, 1.0, bf["coms0"], bf["work"], bf["work_bytes"], st),
                                calls, warm, torch))
    res["com_kernels_equal_host"] = bool(np.array_equal(bu["coms0"].cpu().numpy(),
                                                        np.stack([md.calculateCoM(f) for f in fu])))
    um, fm = min(u_ms), min(f_ms)
    res["com_kernels"] = {"p50_ms": round(um, 5), "GBps": round(n * h * w * 2 / um / 1e6, 1),
                          "pass_p50_ms": [round(x, 5) for x in u_ms]}
    res["f32_com_kernels"] = {"p50_ms": round(fm, 5), "GBps": round(n * h * w * 4 / fm / 1e6, 1),
                              "pass_p50_ms": [round(x, 5) for x in f_ms]}
    res["com_u16_over_f32_time"] = round(um / fm, 3)
    res["com_u16_not_slower"] = bool(um <= fm)
    res["frame_bytes"] = n * h * w * 2
    return res


def step_hbm():
    mp = importlib.import_module("monkey-pose_amd")
    return mp._lib.hbm_probe(0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--dtype", choices=("f32", "u16"), default="f32")
    ap.add_argument("--out")
    ap.add_argument("--step", choices=sorted(STEP_LIMIT_S))
    a = ap.parse_args()
    u16 = a.dtype == "u16"
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "detector", "time_detector_u16_run.json" if u16 else "time_detector.json")
    if a.step:                                   # a child: one step, one JSON line
        if a.step == "hbm":
            r = step_hbm()
        elif u16:
            r = step_batch_u16(256, a.calls)
        else:
            r = step_batch(256 if a.step == "b256" else 1, a.calls)
        print("RESULT " + json.dumps(r), flush=True)
        return 0
    import bench
    doc = {"tool": "tools/time_detector_pipeline.py", "tree_stamp": bench.tree_stamp(), "camera": list(CAM)}
    if u16:
        doc["dtype"] = "u16"
    for step in (("b256", "hbm") if u16 else ("b256", "b1", "hbm")):
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", step, "--calls", str(a.calls)] +
                               (["--dtype", "u16"] if u16 else []),
                               capture_output=True, text=True, timeout=STEP_LIMIT_S[step])
        except subprocess.TimeoutExpired:
            sys.stderr.write(f"step {step}: over its {STEP_LIMIT_S[step]} s limit; stopping\n")
            return 124
        lines = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
        if p.returncode != 0 or not lines:
            sys.stderr.write(f"step {step}: exit {p.returncode}; stopping\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}\n")
            return p.returncode or 1
        doc[step] = json.loads(lines[-1][7:])
        print(step, json.dumps(doc[step]), flush=True)
    g = doc["b256"]
    if u16:
        doc["gate_b256_met"] = bool(g["com_u16_not_slower"] and g["device_equals_host_chain"] and
                                    g["com_kernels_equal_host"])
    else:
        doc["gate_b256_met"] = bool(g["gate_device_h2d_pageable_over_host_chain"] > 1.0 and
                                    g["device_equals_host_chain"])
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", a.out, "gate_b256_met =", doc["gate_b256_met"])
    return 0


if __name__ == "__main__":
    sys.exit(main())
