"""Times the joint overlays (monkeydetector.render_overlays, mp_overlay_dev) at B = 256, 424 x 512,
J = 23, two joint sets and a 22-bone chain, p50 over --calls calls after warm-up:

  (a) kernel      mp_overlay_dev alone on resident frames (device events), uint16 and float32 frames,
                  with GB/s over the bytes read and written, beside its byte floor
                  read_bytes / read roof + write_bytes / write roof from mp_hbm_probe on the same box;
                  and mp_real_frames_dev's stored-layout transpose on the same frames, a byte mover
                  that predates this kernel, beside its own floor.  The scene's joints are chains
                  walking in steps of up to 30 px (limb-length bones); `scene_long` scatters them
                  instead, so that every bone is ~150 px long: the heavy case
  (b) colour map  the same call with J = 0 (no primitives): the difference is what the primitives cost
  (c) pipeline    RealDataPipeline.run alone, run + render + the D2H of the RGB bytes, and the host
                  route the render replaces: D2H of the float32 frames and uvd, then render_overlays_np

  (d) --png       the picture path's last step, after `run`, B frames a call: the host route (render, D2H
                  of the RGB into pinned memory, then tools/eval_real_data.py write_png's compress call per
                  frame on one thread; file writes excluded) against the device route (render_png, then
                  png.png_files: D2H of sizes and of the used columns); the encode alone and its two
                  kernels' sum from device events; the files' sizes against zlib levels 6 and 1; and the
                  encode against its byte floor (raw bytes read + file bytes written at the box's copy
                  rate).  Written to profiles/png/time_png.json

The forms alternate in rounds, so that drift of the shared host hits all of them alike.  Host-clock
timings end in a device synchronise.  Every step runs in a child process of its own under its own
time limit, and the first failure stops the run; the parent never touches the GPU.  One JSON goes to
profiles/overlay/, stamped with bench.tree_stamp.

    python tools/time_overlay.py [--calls 100] [--batch 256] [--out profiles/overlay/time_overlay.json]
    python tools/time_overlay.py --png [--calls 20] [--batch 256] [--out profiles/png/time_png.json]
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
STEP_LIMIT_S = {"batch": 540, "hbm": 240, "png": 540}
HBM_MIB = (128, 512, 2048)
BONES = [(k, k + 1) for k in range(22)]


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
    W, T, M = mp.weights, mp.train_cnn_networks_hgru, mp.monkeydetector
    dev = torch.device("cuda", 0)
    md = M.MonkeyDetector(*CAM)
    cfg = T.InferenceConfig()
    base = W.synth_frames(min(B, 16), seed=14)[..., 0]
    mm = np.round(base * np.float32(10000.0)).astype(np.uint16)
    mm = mm[np.arange(B) % mm.shape[0]]                                   # [B, 424, 512]
    raw = np.ascontiguousarray(mm.transpose(0, 2, 1))                    # as stored
    n, h, w = mm.shape
    px = n * h * w
    sync = lambda: torch.cuda.synchronize(dev)
    warm = max(5, calls // 10)
    res = {"batch": B, "calls": calls, "hw": [h, w], "joints": 23, "sets": 2, "bones": len(BONES)}

    # the scene: two sets of 23 joints, each a chain walking over the body region of its frame in steps
    # of up to 30 px a coordinate (bones the length of a limb segment); and the heavy form of it, the
    # joints scattered over that region independently, so that the 22 bones of a set are ~150 px long
    # and cross one another all over it
    rng = np.random.default_rng(5)
    ju = np.empty((B, 2, 23, 3), np.float32)
    start = np.stack([rng.uniform(200, 310, (B, 2)), rng.uniform(120, 300, (B, 2))], axis=-1)
    walk = start[:, :, None, :] + np.cumsum(rng.uniform(-30, 30, (B, 2, 23, 2)), axis=2)
    ju[..., 0] = np.clip(walk[..., 0], 0, w - 1)
    ju[..., 1] = np.clip(walk[..., 1], 0, h - 1)
    ju[..., 2] = rng.uniform(1000, 3000, (B, 2, 23))
    jl = ju.copy()
    jl[..., 0] = rng.uniform(150, 360, (B, 2, 23))
    jl[..., 1] = rng.uniform(60, 360, (B, 2, 23))
    jd, jld = torch.from_numpy(ju).to(dev), torch.from_numpy(jl).to(dev)
    blen = np.hypot(*np.moveaxis(np.diff(ju[..., :2], axis=2), -1, 0))
    res["scene_mean_bone_px"] = round(float(blen.mean()), 1)
    res["scene_long_mean_bone_px"] = round(float(np.hypot(*np.moveaxis(np.diff(jl[..., :2], axis=2), -1, 0)).mean()), 1)
    none = torch.zeros((B, 1, 0, 3), dtype=torch.float32, device=dev)
    fu = torch.from_numpy(mm).to(dev)
    ff = fu.float()
    out = torch.empty((B, h, w, 3), dtype=torch.uint8, device=dev)
    kw = dict(depth_range=(1000, 3000), lut="jet", out=out)

    # (a), (b): the kernel alone, device events; two alternated passes, the smaller median kept
    raw_d = torch.from_numpy(raw).to(dev)
    fbuf = torch.empty((B, h, w, 1), dtype=torch.float32, device=dev)
    forms = {"u16_scene": (lambda: M.render_overlays(fu, jd, bones=BONES, **kw), 2, 3),
             "f32_scene": (lambda: M.render_overlays(ff, jd, bones=BONES, **kw), 4, 3),
             "u16_scene_long": (lambda: M.render_overlays(fu, jld, bones=BONES, **kw), 2, 3),
             "u16_colour_map": (lambda: M.render_overlays(fu, none, **kw), 2, 3),
             "f32_colour_map": (lambda: M.render_overlays(ff, none, **kw), 4, 3),
             "real_transpose_u16": (lambda: M.preprocess_real_frames(raw_d, out=fbuf), 2, 4)}
    ms = {k: [] for k in forms}
    for _ in range(2):
        for k, (f, _i, _o) in forms.items():
            ms[k].append(event_timed(f, calls, warm, torch))
    res["kernel"] = {}
    for k, (_f, inb, outb) in forms.items():
        t = min(ms[k])
        res["kernel"][k] = {"p50_ms": round(t, 5), "pass_p50_ms": [round(x, 5) for x in ms[k]],
                            "read_bytes": px * inb, "write_bytes": px * outb,
                            "GBps": round(px * (inb + outb) / t / 1e6, 1)}
    for dt in ("u16", "f32"):
        res["kernel"][dt + "_primitives_ms"] = round(res["kernel"][dt + "_scene"]["p50_ms"]
                                                     - res["kernel"][dt + "_colour_map"]["p50_ms"], 5)
    few = slice(0, 4)
    ref = M.render_overlays_np(mm[few], ju[few], bones=BONES, depth_range=(1000, 3000), lut="jet")
    res["kernel_equals_numpy"] = bool(
        np.array_equal(M.render_overlays(fu, jd, bones=BONES, **kw)[few].cpu().numpy(), ref)
        and np.array_equal(M.render_overlays(ff, jd, bones=BONES, **kw)[few].cpu().numpy(), ref)
        and np.array_equal(M.render_overlays(fu, jld, bones=BONES, **kw)[few].cpu().numpy(),
                           M.render_overlays_np(mm[few], jl[few], bones=BONES, depth_range=(1000, 3000), lut="jet")))

    # (c) the pipeline
    aw = W.attn_synth_weights(seed=1234)
    aw["cnn/afc_out/afc_out_weights"] = np.zeros((1024, 3), np.float32)
    aw["cnn/afc_out/afc_out_biases"] = np.asarray(COM_NORM, np.float32)
    attn = T.attn_model_struct()
    attn.load_weights(aw)
    pose = T.cnn_model_struct()
    pose.load_weights(W.synth_weights(W.cnn_vars(output_shape=69, crop=128), seed=77))
    pipe = T.RealDataPipeline(attn, pose, md, cfg)
    rgb_host = torch.empty((B, h, w, 3), dtype=torch.uint8).pin_memory()
    frames_host = torch.empty((B, h, w, 1), dtype=torch.float32).pin_memory()
    uvd_host = torch.empty((B, 23, 3), dtype=torch.float32).pin_memory()

    def run_only():
        return pipe.run(raw_d)

    def run_render_d2h():
        pipe.run(raw_d)
        rgb_host.copy_(pipe.render(bones=BONES, lut="jet", out=out), non_blocking=True)

    def run_d2h_frames():
        res_ = pipe.run(raw_d)
        frames_host.copy_(pipe._frames, non_blocking=True)
        uvd_host.copy_(res_[1], non_blocking=True)

    fns = dict(run=run_only, run_render_d2h_rgb=run_render_d2h, run_d2h_frames_uvd=run_d2h_frames)
    rounds = 4
    per = -(-calls // rounds)
    acc = {k: [] for k in fns}
    for r in range(rounds):
        for k, f in fns.items():
            acc[k].append(host_timed(f, per, warm if r == 0 else 2, sync))
    res["pipeline"] = {}
    for k, v in acc.items():
        t = p50(np.concatenate(v))
        res["pipeline"][k] = {"p50_ms": round(t, 4), "frames_per_s": round(B / t * 1e3, 1),
                              "samples": int(sum(len(x) for x in v)), "round_p50_ms": [round(p50(x), 4) for x in v]}
    # the host route's drawing: numpy on the frames and joints copied back (a few calls: it is slow)
    run_d2h_frames()
    sync()
    fh, uh = frames_host.numpy(), uvd_host.numpy()
    hn = host_timed(lambda: M.render_overlays_np(fh, uh, bones=BONES, depth_range=(0.1, 0.3), lut="jet"), 3, 1,
                    lambda: None)
    res["pipeline"]["host_render_numpy"] = {"p50_ms": round(p50(hn), 2), "samples": len(hn),
                                            "all_ms": [round(x, 2) for x in hn]}
    res["pipeline"]["host_route_ms"] = round(res["pipeline"]["run_d2h_frames_uvd"]["p50_ms"] + p50(hn), 2)
    run_render_d2h()
    sync()
    res["pipeline_render_equals_numpy"] = bool(np.array_equal(
        rgb_host.numpy()[few], M.render_overlays_np(fh[few], uh[few], bones=BONES, depth_range=(0.1, 0.3), lut="jet")))
    return res


def step_png(B, calls):
    """(d): the host route and the device route of the PNG files of one batch, after `run`"""
    import zlib
    import torch
    mp = importlib.import_module("monkey-pose_amd")
    W, T, M, P = mp.weights, mp.train_cnn_networks_hgru, mp.monkeydetector, mp.png
    dev = torch.device("cuda", 0)
    md = M.MonkeyDetector(*CAM)
    base = W.synth_frames(min(B, 16), seed=14)[..., 0]
    mm = np.round(base * np.float32(10000.0)).astype(np.uint16)
    mm = mm[np.arange(B) % mm.shape[0]]
    raw_d = torch.from_numpy(np.ascontiguousarray(mm.transpose(0, 2, 1))).to(dev)
    n, h, w = mm.shape
    sync = lambda: torch.cuda.synchronize(dev)
    aw = W.attn_synth_weights(seed=1234)
    aw["cnn/afc_out/afc_out_weights"] = np.zeros((1024, 3), np.float32)
    aw["cnn/afc_out/afc_out_biases"] = np.asarray(COM_NORM, np.float32)
    attn = T.attn_model_struct()
    attn.load_weights(aw)
    pose = T.cnn_model_struct()
    pose.load_weights(W.synth_weights(W.cnn_vars(output_shape=69, crop=128), seed=77))
    pipe = T.RealDataPipeline(attn, pose, md, T.InferenceConfig())
    pipe.run(raw_d)
    sync()
    rgb_dev = torch.empty((B, h, w, 3), dtype=torch.uint8, device=dev)
    rgb_host = torch.empty((B, h, w, 3), dtype=torch.uint8).pin_memory()
    res = {"batch": B, "hw": [h, w], "joints": 23, "sets": 1, "bones": len(BONES), "luts": {}}
    for lut in ("gray", "jet"):
        kw = dict(bones=BONES, lut=lut)
        rows = np.zeros((h, 1 + 3 * w), np.uint8)
        z6 = []

        def host_route():
            rgb_host.copy_(pipe.render(out=rgb_dev, **kw), non_blocking=True)
            sync()
            z6.clear()
            for img in rgb_host.numpy():
                rows[:, 1:] = img.reshape(h, 3 * w)
                z6.append(len(zlib.compress(rows.tobytes(), 6)))          # write_png's IDAT body

        files = []

        def device_route():
            files[:] = P.png_files(*pipe.render_png(out=rgb_dev, **kw))

        acc = {"host": [], "device": []}
        for r in range(3):                                                 # alternated rounds
            acc["host"].append(host_timed(host_route, 1, 1 if r == 0 else 0, sync))
            acc["device"].append(host_timed(device_route, max(1, calls // 3), 2 if r == 0 else 0, sync))
        th, td = p50(np.concatenate(acc["host"])), p50(np.concatenate(acc["device"]))
        rgb = pipe.render(out=rgb_dev, **kw)
        enc = event_timed(lambda: P.encode_png(rgb), calls, 3, torch)
        ren = event_timed(lambda: pipe.render(out=rgb_dev, **kw), calls, 3, torch)
        few = rgb_host.numpy()[:4]
        hb, hs = P.encode_png(few)
        sizes = np.asarray([len(f) for f in files])
        z1 = []
        for img in few:
            rows[:, 1:] = img.reshape(h, 3 * w)
            z1.append(len(zlib.compress(rows.tobytes(), 1)))
        res["luts"][lut] = {
            "host_route_ms": round(th, 2), "host_route_all_ms": [round(float(x), 2) for x in np.concatenate(acc["host"])],
            "device_route_ms": round(td, 3), "device_route_samples": int(sum(len(x) for x in acc["device"])),
            "host_over_device": round(th / td, 1), "render_event_ms": round(ren, 4), "encode_event_ms": round(enc, 4),
            "raw_bytes": int(B * h * (1 + 3 * w)), "file_bytes": int(sizes.sum()),
            "file_bytes_per_frame": int(sizes.mean()), "bound_per_frame": P.png_bound(h, w),
            "zlib6_idat_bytes_per_frame": int(np.mean(z6)), "zlib1_idat_bytes_per_frame_first4": int(np.mean(z1)),
            "device_equals_host_first4": bool(files[:4] == P.png_files(hb, hs)),
        }
    return res


def step_hbm():
    mp = importlib.import_module("monkey-pose_amd")
    return {str(mib): mp._lib.hbm_probe(0, mib << 20) for mib in HBM_MIB}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--out")
    ap.add_argument("--png", action="store_true", help="the PNG leg (d) instead of (a)-(c)")
    ap.add_argument("--step", choices=sorted(STEP_LIMIT_S))
    a = ap.parse_args()
    if a.step:                                   # a child: one step, one JSON line
        r = step_hbm() if a.step == "hbm" else step_png(a.batch, a.calls) if a.step == "png" else step_batch(a.batch, a.calls)
        print("RESULT " + json.dumps(r), flush=True)
        return 0
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "png" if a.png else "overlay", "time_png.json" if a.png else "time_overlay.json")
    import bench
    doc = {"tool": "tools/time_overlay.py" + (" --png" if a.png else ""), "tree_stamp": bench.tree_stamp(), "camera": list(CAM)}
    for step in (("png", "hbm") if a.png else ("batch", "hbm")):
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", step, "--calls", str(a.calls),
                                "--batch", str(a.batch)], capture_output=True, text=True, timeout=STEP_LIMIT_S[step])
        except subprocess.TimeoutExpired:
            sys.stderr.write(f"step {step}: over its {STEP_LIMIT_S[step]} s limit; stopping\n")
            return 124
        lines = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
        if p.returncode != 0 or not lines:
            sys.stderr.write(f"step {step}: exit {p.returncode}; stopping\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}\n")
            return p.returncode or 1
        doc[step] = json.loads(lines[-1][7:])
        print(step, json.dumps(doc[step]), flush=True)
    if a.png:                                    # the encode against raw bytes in + file bytes out at the copy rate
        for lut, v in doc["png"]["luts"].items():
            v["encode_byte_floor_by_probe_MiB"] = {}
            for mib, r in doc["hbm"].items():
                fl = (v["raw_bytes"] + v["file_bytes"]) / r["copy_GBps"] / 1e6
                v["encode_byte_floor_by_probe_MiB"][mib] = {"floor_ms": round(fl, 5),
                                                            "encode_over_floor": round(v["encode_event_ms"] / fl, 2)}
        doc["faster"] = all(v["device_route_ms"] < v["host_route_ms"] for v in doc["png"]["luts"].values())
        doc["equal"] = all(v["device_equals_host_first4"] for v in doc["png"]["luts"].values())
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
        print("wrote", a.out, "device route faster =", doc["faster"], "equal =", doc["equal"])
        return 0 if doc["faster"] and doc["equal"] else 1
    # the kernels' byte floors under the box's own streaming roofs (per probe size)
    floors = {}
    for mib, r in doc["hbm"].items():
        floors[mib] = {}
        for k, v in doc["batch"]["kernel"].items():
            if not isinstance(v, dict):
                continue
            fl = v["read_bytes"] / r["read_GBps"] / 1e6 + v["write_bytes"] / r["write_GBps"] / 1e6
            floors[mib][k] = {"floor_ms": round(fl, 5), "kernel_over_floor": round(v["p50_ms"] / fl, 3)}
    doc["kernel_byte_floor_by_probe_MiB"] = floors
    doc["equal"] = bool(doc["batch"]["kernel_equals_numpy"] and doc["batch"]["pipeline_render_equals_numpy"])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", a.out, "equal =", doc["equal"])
    return 0


if __name__ == "__main__":
    sys.exit(main())
