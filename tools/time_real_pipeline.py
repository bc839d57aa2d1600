"""Times the real-data evaluation (eval_model_on_real_data's per-batch body) at B = 256 from host raw
frames: uint16 [B, 512, 424] as the recordings are stored, p50 over --calls calls after warm-up:

  (a) host chain  numpy transpose, gate and normalise (the host preprocess_real_frames) -> H2D of the
                  float32 frames -> FramePosePipeline.run -> getAbsoluteCoordinates_device: the only
                  way to run this path before RealDataPipeline
  (b) device      RealDataPipeline.run including the H2D of the raw uint16 frames (from the pageable
                  numpy array, and from a pinned staging buffer) and with the frames already resident
  (c) kernel      mp_real_frames_dev alone on resident frames (device events): uint16 and float32
                  stored frames (the LDS transpose) and uint16 frames already [h, w] (the plain pass),
                  with GB/s over the bytes read and written, beside its byte floor
                  read_bytes / read roof + write_bytes / write roof from mp_hbm_probe on the same box

The forms alternate in rounds, so that drift of the shared host hits all of them alike.  Host-clock
timings end in a device synchronise.  Every step runs in a child process of its own under its own
time limit, and the first failure stops the run; the parent never touches the GPU.  One JSON goes to
profiles/real/, stamped with bench.tree_stamp.

    python tools/time_real_pipeline.py [--calls 100] [--batch 256] [--model cnn|hgru] [--out profiles/real/time_real.json]
"""
import argparse
import importlib
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CAM = (365.456, 365.456, 256, 212, [800, 800, 1200], 200, 10000)   # train_cnn_networks_hgru.py:345
COM_NORM = (0.5, 0.5, 0.13)        # afc_out: zero weights, these biases -- every crop is valid
STEP_LIMIT_S = {"batch": 420, "hbm": 240}
HBM_MIB = (128, 512, 2048)


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


def step_batch(B, calls, model):
    import torch
    mp = importlib.import_module("monkey-pose_amd")
    W, T, M = mp.weights, mp.train_cnn_networks_hgru, mp.monkeydetector
    dev = torch.device("cuda", 0)
    md = M.MonkeyDetector(*CAM)
    cfg = T.InferenceConfig()
    base = W.synth_frames(min(B, 16), seed=14)[..., 0]
    mm = np.round(base * np.float32(10000.0)).astype(np.uint16)
    raw = np.ascontiguousarray(mm[np.arange(B) % mm.shape[0]].transpose(0, 2, 1))    # [B, 512, 424] as stored
    n, w, h = raw.shape
    aw = W.attn_synth_weights(seed=1234)
    aw["cnn/afc_out/afc_out_weights"] = np.zeros((1024, 3), np.float32)
    aw["cnn/afc_out/afc_out_biases"] = np.asarray(COM_NORM, np.float32)
    attn = T.attn_model_struct()
    attn.load_weights(aw)
    if model == "hgru":
        pose = mp.hgru_pose.model()
        pose.load_weights(W.synth_weights(W.hgru_pose_vars(output_shape=69, timesteps=8, crop=128), seed=21))
    else:
        pose = T.cnn_model_struct()
        pose.load_weights(W.synth_weights(W.cnn_vars(output_shape=69, crop=128), seed=77))
    sync = lambda: torch.cuda.synchronize(dev)
    warm = max(5, calls // 10)
    res = {"batch": B, "calls": calls, "stored_wh": [w, h], "pose_model": model}

    # (a) the host chain
    frame_pipe = T.FramePosePipeline(attn, pose, md, cfg)
    stage_f = torch.empty((B, h, w, 1), dtype=torch.float32, device=dev)
    out_host = tuple(torch.empty((B, 23, 3), dtype=torch.float32, device=dev) for _ in range(2))

    def host_chain():
        frames = M.preprocess_real_frames(raw)
        stage_f.copy_(torch.from_numpy(frames))
        out, coms, Ms = frame_pipe.run(stage_f)
        return md.getAbsoluteCoordinates_device(out, coms, 23, out=out_host) + (coms, Ms)

    def host_preprocess_only():
        return M.preprocess_real_frames(raw)

    # (b) the device pipeline
    pipe = T.RealDataPipeline(attn, pose, md, cfg)
    raw_t = torch.from_numpy(raw)
    pinned = torch.empty_like(raw_t).pin_memory()
    pinned.copy_(raw_t)
    stage_u = torch.empty((B, w, h), dtype=torch.uint16, device=dev)
    resident = raw_t.to(dev)

    def dev_pageable():
        stage_u.copy_(raw_t)
        return pipe.run(stage_u)

    def dev_pinned():
        stage_u.copy_(pinned, non_blocking=True)
        return pipe.run(stage_u)

    def dev_resident():
        return pipe.run(resident)

    ref = [t.cpu().numpy() for t in host_chain()]
    got = [t.cpu().numpy() for t in dev_pageable()[:4]]
    res["device_equals_host_chain"] = bool(all(np.array_equal(g, r) for g, r in zip(got, ref)))
    fns = dict(host_chain=host_chain, device_h2d_pageable=dev_pageable, device_h2d_pinned=dev_pinned,
               device_resident=dev_resident)
    rounds = 4
    per = -(-calls // rounds)
    acc = {k: [] for k in fns}
    for r in range(rounds):
        for k, f in fns.items():
            acc[k].append(host_timed(f, per, warm if r == 0 else 2, sync))
    for k, v in acc.items():
        ms = p50(np.concatenate(v))
        res[k] = {"p50_ms": round(ms, 4), "frames_per_s": round(B / ms * 1e3, 1), "samples": int(sum(len(x) for x in v)),
                  "round_p50_ms": [round(p50(x), 4) for x in v]}
    for k in ("device_h2d_pageable", "device_h2d_pinned", "device_resident"):
        res[k + "_over_host_chain"] = round(res["host_chain"]["p50_ms"] / res[k]["p50_ms"], 3)
    hp = host_timed(host_preprocess_only, max(5, calls // 5), 2, lambda: None)
    res["host_preprocess_numpy"] = {"p50_ms": round(p50(hp), 4), "samples": len(hp)}

    # (c) the kernel alone, device events; two alternated passes, the smaller median kept
    buf = torch.empty((B, h, w, 1), dtype=torch.float32, device=dev)
    res_f = torch.from_numpy(raw.astype(np.float32)).to(dev)
    plain_u = torch.from_numpy(np.ascontiguousarray(raw.transpose(0, 2, 1))).to(dev)
    forms = {"u16_stored": (lambda: M.preprocess_real_frames(resident, out=buf), 2),
             "f32_stored": (lambda: M.preprocess_real_frames(res_f, out=buf), 4),
             "u16_plain": (lambda: M.preprocess_real_frames(plain_u, transposed=False, out=buf), 2)}
    ms = {k: [] for k in forms}
    for _ in range(2):
        for k, (f, _b) in forms.items():
            ms[k].append(event_timed(f, calls, warm, torch))
    px = n * h * w
    res["kernel"] = {}
    for k, (_f, inb) in forms.items():
        t = min(ms[k])
        res["kernel"][k] = {"p50_ms": round(t, 5), "pass_p50_ms": [round(x, 5) for x in ms[k]],
                            "read_bytes": px * inb, "write_bytes": px * 4,
                            "GBps": round(px * (inb + 4) / t / 1e6, 1)}
    res["kernel_equals_host"] = bool(np.array_equal(M.preprocess_real_frames(resident).cpu().numpy(),
                                                    M.preprocess_real_frames(raw)))
    return res


def step_hbm():
    mp = importlib.import_module("monkey-pose_amd")
    return {str(mib): mp._lib.hbm_probe(0, mib << 20) for mib in HBM_MIB}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--model", choices=("cnn", "hgru"), default="cnn")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "real", "time_real.json"))
    ap.add_argument("--step", choices=sorted(STEP_LIMIT_S))
    a = ap.parse_args()
    if a.step:                                   # a child: one step, one JSON line
        r = step_hbm() if a.step == "hbm" else step_batch(a.batch, a.calls, a.model)
        print("RESULT " + json.dumps(r), flush=True)
        return 0
    import bench
    doc = {"tool": "tools/time_real_pipeline.py", "tree_stamp": bench.tree_stamp(), "camera": list(CAM)}
    for step in ("batch", "hbm"):
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", step, "--calls", str(a.calls),
                                "--batch", str(a.batch), "--model", a.model],
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
    # the kernel's byte floor under the box's own streaming roofs (per probe size)
    floors = {}
    for mib, r in doc["hbm"].items():
        floors[mib] = {}
        for k, v in doc["batch"]["kernel"].items():
            fl = v["read_bytes"] / r["read_GBps"] / 1e6 + v["write_bytes"] / r["write_GBps"] / 1e6
            floors[mib][k] = {"floor_ms": round(fl, 5), "kernel_over_floor": round(v["p50_ms"] / fl, 3)}
    doc["kernel_byte_floor_by_probe_MiB"] = floors
    doc["equal"] = bool(doc["batch"]["device_equals_host_chain"] and doc["batch"]["kernel_equals_host"])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", a.out, "equal =", doc["equal"])
    return 0


if __name__ == "__main__":
    sys.exit(main())
