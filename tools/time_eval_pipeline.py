"""Times the validation pass at B = 256 with frames and labels resident on the device, p50 after
warm-up, the three paths interleaved in one process over --rounds rounds:

  (a) frame_pose   FramePosePipeline.run alone (attention -> crop -> pose)
  (b) validation   ValidationPipeline.run: (a) plus relative labels, CoM from joints and the two
                   device evaluators, no host step
  (c) host_eval    the host evaluation (b) replaces: (a), then D2H of the pose output, the attention
                   output, the CoMs and the labels, the host label half of prepare_data, and the
                   numpy metrics (vectorised over the batch: joint distances, per-frame nanmean /
                   nanmax, per-joint sums, 100 thresholds, calculateCoMfrom3DJoints + calc_com_error)

and the device-event time of the new kernels alone (mp_rel_labels_dev, mp_com_from_joints_dev,
mp_eval_accumulate_dev for the pose and the CoM evaluator).  The condition is (b) - (a) <= (c) - (a),
reported next to the round-to-round spread of (a).

Host-clock timings end in a device synchronise.  The GPU step runs in a child process under its own
time limit, and a failure stops the run; the parent never touches the GPU.  One JSON with every
round goes to profiles/eval/, stamped with bench.tree_stamp.

    python tools/time_eval_pipeline.py [--calls 120] [--rounds 4] [--model hgru|cnn]
                                       [--out profiles/eval/time_eval.json]
"""
import argparse
import importlib
import json
import os
import subprocess
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CAM = (365.456, 365.456, 256, 212, [800, 800, 1200], 200, 10000)
STEP_LIMIT_S = 540
B = 256


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


class HostEvaluator:
    """the numpy accumulation a user writes around the `_np` functions, vectorised over the batch"""

    def __init__(self, J, T=100):
        self.thr = np.arange(T, dtype=np.float32)
        self.reset(J)

    def reset(self, J):
        self.frames, self.valid, self.sum_mean, self.max = 0, 0, 0.0, 0.0
        self.jsum, self.jcnt = np.zeros(J), np.zeros(J, np.int64)
        self.wmax, self.wmean = np.zeros(self.thr.size, np.int64), np.zeros(self.thr.size, np.int64)

    def update(self, lab, res):
        d = np.sqrt(np.square(lab - res).sum(axis=2))
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            fmean, fmax = np.nanmean(d, axis=1), np.nanmax(d, axis=1)
        ok = ~np.isnan(fmean)
        self.frames += d.shape[0]
        self.valid += int(ok.sum())
        self.sum_mean += float(fmean[ok].astype(np.float64).sum())
        if ok.any():
            self.max = max(self.max, float(fmax[ok].max()))
        self.jsum += np.nansum(d.astype(np.float64), axis=0)
        self.jcnt += (~np.isnan(d)).sum(axis=0)
        self.wmax += (fmax[:, None] <= self.thr[None, :]).sum(axis=0)
        self.wmean += (fmean[:, None] <= self.thr[None, :]).sum(axis=0)


def step(calls, rounds, model):
    import torch
    mp = importlib.import_module("monkey-pose_amd")
    W, T, L = mp.weights, mp.train_cnn_networks_hgru, mp._lib
    dev = torch.device("cuda", 0)
    md = mp.monkeydetector.MonkeyDetector(*CAM)
    cfg = T.InferenceConfig()
    J = cfg.num_joints
    base = W.synth_frames(16, seed=14)
    frames = torch.from_numpy(np.ascontiguousarray(base[np.arange(B) % 16])).to(dev)      # [B, 424, 512, 1] normalised
    c = md.uvdtoxyz(np.array([212., 256., 1500.]))
    lab_np = (c + np.random.RandomState(3).uniform(-700, 700, (B, J, 3))).astype(np.float32)
    labels = torch.from_numpy(lab_np).to(dev)
    attn = T.attn_model_struct()
    attn.load_weights(W.attn_synth_weights(seed=1234))
    kw = {}
    if model == "hgru":
        pose = mp.hgru_pose.model()
        pose.load_weights(W.synth_weights(W.hgru_pose_vars(output_shape=69, timesteps=8, crop=128), seed=21))
        kw["h2_init"] = torch.from_numpy(W.synth_hidden((B, 64, 64, 64), seed=3)).to(dev)
    else:
        pose = T.cnn_model_struct()
        pose.load_weights(W.synth_weights(W.cnn_vars(output_shape=69, crop=128), seed=21))
    fpp = T.FramePosePipeline(attn, pose, md, cfg, check_crops=False)
    val = T.ValidationPipeline(attn, pose, md, cfg, check_crops=False)
    half = np.float32(md.cube[2] / 2.)
    scale = (cfg.image_orig_size[0], cfg.image_orig_size[1], cfg.image_max_depth)
    hp, hc = HostEvaluator(J), HostEvaluator(1)

    def frame_pose():
        return fpp.run(frames, **kw)

    def validation():
        return val.run(frames, labels, **kw)

    def host_eval():
        out, coms, _ = fpp.run(frames, **kw)
        out_h, com_h, lab_h = out.cpu().numpy(), coms.cpu().numpy(), labels.cpu().numpy()
        attn_h = attn.out_put.cpu().numpy()
        rel = md.relative_labels(lab_h, com_h)
        hp.update((rel * half).reshape(B, J, 3), (out_h * half).reshape(B, J, 3))
        hc.update(md.calculateCoMfrom3DJoints(lab_h, scale=scale)[:, None, :], attn_h[:, None, :])

    sync = lambda: torch.cuda.synchronize(dev)
    # the two evaluations agree before anything is timed
    val.reset()
    validation()
    s = val.summary()
    hp.reset(J)
    hc.reset(1)
    host_eval()
    agree = bool(np.array_equal(np.rint(s["pose"]["within_mean"] * B / 100.), hp.wmean)
                 and np.array_equal(np.rint(s["pose"]["within_max"] * B / 100.), hp.wmax)
                 and s["pose"]["max_error"] == hp.max
                 and abs(s["pose"]["mean_error"] - hp.sum_mean / hp.valid) <= 1e-12 * s["pose"]["mean_error"]
                 and abs(s["com"]["mean_error"] - hc.sum_mean / hc.valid) <= 1e-12 * s["com"]["mean_error"])
    res = {"batch": B, "calls": calls, "rounds": rounds, "model": model, "device_equals_host_eval": agree,
           "pose_mean_error_mm": s["pose"]["mean_error"]}
    fns = dict(frame_pose=frame_pose, validation=validation, host_eval=host_eval)
    acc = {k: [] for k in fns}
    per = -(-calls // rounds)
    warm = max(10, calls // 10)
    for r in range(rounds):
        for k, f in fns.items():
            acc[k].append(host_timed(f, per, warm if r == 0 else 3, sync))
    for k, v in acc.items():
        res[k] = {"p50_ms": round(p50(np.concatenate(v)), 4), "round_p50_ms": [round(p50(x), 4) for x in v],
                  "samples": int(sum(len(x) for x in v))}
    a, b, c_ = (res[k]["p50_ms"] for k in ("frame_pose", "validation", "host_eval"))
    ra = res["frame_pose"]["round_p50_ms"]
    res["device_eval_cost_ms"] = round(b - a, 4)
    res["host_eval_cost_ms"] = round(c_ - a, 4)
    res["device_eval_cost_by_round_ms"] = [round(x - y, 4) for x, y in zip(res["validation"]["round_p50_ms"], ra)]
    res["host_eval_cost_by_round_ms"] = [round(x - y, 4) for x, y in zip(res["host_eval"]["round_p50_ms"], ra)]
    res["frame_pose_round_spread_ms"] = round(max(ra) - min(ra), 4)
    res["condition_device_cost_le_host_cost"] = bool(b - a <= c_ - a)
    res["device_cost_inside_frame_pose_spread"] = bool(abs(b - a) <= max(ra) - min(ra))

    # the new kernels alone, device events
    out, coms, _ = fpp.run(frames, **kw)
    com_norm = attn.out_put
    rel = torch.empty((B, 3 * J), dtype=torch.float32, device=dev)
    com2d = torch.empty((B, 3), dtype=torch.float32, device=dev)
    pe, ce = mp.pose_evaluation.PoseEvaluator(J), mp.pose_evaluation.PoseEvaluator(1)
    kern = {
        "rel_labels": lambda: md.relative_labels_device(labels, coms, out=rel),
        "com_from_joints": lambda: md.calculateCoMfrom3DJoints(labels, scale=scale, out=com2d),
        "eval_accumulate_pose": lambda: pe.update(rel, out, scale=float(half)),
        "eval_accumulate_com": lambda: ce.update(com2d[:, None, :], com_norm[:, None, :]),
    }
    res["kernels_event_p50_ms"] = {k: round(event_timed(f, calls, warm, torch), 5) for k, f in kern.items()}
    res["kernels_event_sum_ms"] = round(sum(res["kernels_event_p50_ms"].values()), 5)
    res["note"] = ("the events bracket the facade call on an idle GPU, so each figure is bounded below by the "
                   "host's launch path (argument checks, output allocation), not by the kernels' run time")
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=120)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--model", choices=["hgru", "cnn"], default="hgru")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval", "time_eval.json"))
    ap.add_argument("--step", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.rounds < 3:
        ap.error("--rounds must be at least 3")
    if a.step:                                   # the child: one JSON line
        print("RESULT " + json.dumps(step(a.calls, a.rounds, a.model)), flush=True)
        return 0
    import bench
    doc = {"tool": "tools/time_eval_pipeline.py", "tree_stamp": bench.tree_stamp(), "camera": list(CAM)}
    try:
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", "--calls", str(a.calls), "--rounds",
                            str(a.rounds), "--model", a.model], capture_output=True, text=True, timeout=STEP_LIMIT_S)
    except subprocess.TimeoutExpired:
        sys.stderr.write(f"the timing step ran over its {STEP_LIMIT_S} s limit; stopping\n")
        return 124
    lines = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
    if p.returncode != 0 or not lines:
        sys.stderr.write(f"the timing step failed (exit {p.returncode}); stopping\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}\n")
        return p.returncode or 1
    doc["b256"] = json.loads(lines[-1][7:])
    print(json.dumps(doc["b256"]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", a.out, "condition met =", doc["b256"]["condition_device_cost_le_host_cost"])
    return 0


if __name__ == "__main__":
    sys.exit(main())
