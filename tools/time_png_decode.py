"""Times PNG decoding of B = 256 depth frames of 424 x 512 gray16 (weights.synth_frames in whole mm, 16
distinct frames repeated; written by tests/pngdec_cases.py's writer with adaptive row filters, zlib
level 6, 8192-byte IDATs).  All forms alternate in rounds in one process; each reports the p50 over the
rounds' p50s and the spread between rounds (min .. max of the rounds' p50s), in ms per batch:

  (a) host chain    decode on 16 threads -> stack -> upload uint16: PIL where installed, else
                    mp_png_decode_host per thread (the JSON says which; both are timed where PIL is there)
  (b) device        upload the packed files (pageable, and from a pinned buffer) + decode_png
  (c) device alone  decode_png with the files resident; each kernel alone from torch.profiler's device
                    times of the same calls; symbols per second of the inflate kernel
  (d) side stream   DetectorPosePipeline.run (the pose forward, crop 128) alone, decode_png alone, and both
                    with the decode of the next batch on a second stream: what the pair costs against
                    the sum of the two

and the bytes crossed: the files against the raw uint16 frames.  Host-clock timings end in a device
synchronise.  The measuring runs in a child process under a time limit; the parent never touches the
GPU.  One JSON goes to profiles/pngdec/, stamped with bench.tree_stamp.

    python tools/time_png_decode.py [--batch 256] [--rounds 5] [--calls 5] [--out profiles/pngdec/time_png_decode.json]
"""
import argparse
import importlib
import io
import json
import os
import subprocess
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
CAM = (365.456, 365.456, 256, 212, [800, 800, 1200], 200, 2500)   # near range: the CoM is on the body
CHILD_LIMIT_S = 540
DISTINCT = 16
THREADS = 16


def count_symbols(z):
    """literal / length symbols and end-of-block codes of a zlib stream (a plain walk of RFC 1951)"""
    import pngdec_cases as C
    pos, n, done = 16, 0, False

    def bits(k):
        nonlocal pos
        v = 0
        for i in range(k):
            v |= ((z[pos >> 3] >> (pos & 7)) & 1) << i
            pos += 1
        return v

    def table(lens):
        return {(l, c): s for s, (c, l) in C.canonical(lens).items()}

    def sym(tab):
        c = 0
        for l in range(1, 16):
            c = (c << 1) | bits(1)
            if (l, c) in tab:
                return tab[(l, c)]
        raise ValueError("bad code")

    fixed = (table([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8), table([5] * 32))
    while not done:
        done, typ = bits(1), bits(2)
        if typ == 0:
            pos = (pos + 7) & ~7
            ln = bits(16)
            pos += 16 + 8 * ln
            n += ln
            continue
        if typ == 1:
            ll, dd = fixed
        else:
            nl, nd, nc = bits(5) + 257, bits(5) + 1, bits(4) + 4
            cl = [0] * 19
            for i in range(nc):
                cl[C.CL_ORDER[i]] = bits(3)
            ct, lens = table(cl), []
            while len(lens) < nl + nd:
                s = sym(ct)
                if s < 16:
                    lens.append(s)
                elif s == 16:
                    lens += [lens[-1]] * (3 + bits(2))
                else:
                    lens += [0] * ((3 + bits(3)) if s == 17 else (11 + bits(7)))
            ll, dd = table(lens[:nl]), table(lens[nl:])
        while True:
            s = sym(ll)
            n += 1
            if s == 256:
                break
            if s > 256:
                bits(C.LEN_EXTRA[s - 257])
                bits(C.DIST_EXTRA[sym(dd)])
    return n


def spread(rounds):
    p = [float(np.median(r)) for r in rounds]
    return {"p50_ms": float(np.median(p)), "rounds_min_ms": min(p), "rounds_max_ms": max(p), "rounds": len(p)}


def child(a):
    import torch
    import pngdec_cases as C
    mp = importlib.import_module("monkey-pose_amd")
    W, T, P = mp.weights, mp.train_cnn_networks_hgru, mp.png
    B = a.batch
    dev = torch.device("cuda", 0)
    sync = lambda: torch.cuda.synchronize(dev)
    base = np.round(W.synth_frames(DISTINCT, seed=14)[..., 0] * np.float32(10000.0)).astype(np.uint16)
    t0 = time.perf_counter()
    distinct = [C.write_png(f, "gray16", filters="adaptive", cuts=8192) for f in base]
    print(f"wrote {DISTINCT} files in {time.perf_counter() - t0:.1f} s", flush=True)
    files = [distinct[i % DISTINCT] for i in range(B)]
    frames = base[np.arange(B) % DISTINCT]
    n, h, w = frames.shape
    # counted on the first four files by a plain walk, scaled by the compressed bytes of the batch
    syms = int(sum(count_symbols(C.zstream(f)) for f in distinct[:4]) / sum(map(len, distinct[:4])) * sum(map(len, files)))
    res = {"batch": B, "frame_hw": [h, w], "rounds": a.rounds, "calls_per_round": a.calls, "distinct_files": DISTINCT,
           "bytes": {"files": int(sum(map(len, files))), "raw_u16": int(frames.nbytes),
                     "ratio": float(frames.nbytes / sum(map(len, files)))}, "inflate_symbols_estimated": syms}

    # ---- the forms
    try:
        from PIL import Image
    except ImportError:
        Image = None
    res["host_decoder"] = "PIL " + Image.__version__ if Image else "mp_png_decode_host per thread"
    pool = ThreadPoolExecutor(THREADS)
    stage = torch.empty((B, h, w), dtype=torch.uint16, device=dev)

    def pil_one(f):
        return np.asarray(Image.open(io.BytesIO(f)))

    def lib_one(f):
        return P.decode_png(*P.pack_files([f]), h, w, "gray16")[0]

    def host_chain(one):
        def run():
            batch = np.stack(list(pool.map(one, files)))
            stage.copy_(torch.from_numpy(batch))
            return stage
        return run

    buf_np, sizes_np = P.pack_files(files)
    buf_pin, _ = P.pack_files(files, pinned=True)
    d_buf = torch.empty(buf_np.shape, dtype=torch.uint8, device=dev)
    d_sizes = torch.from_numpy(sizes_np).to(dev)
    res["bytes"]["packed_upload"] = int(buf_np.nbytes)

    def dev_pageable():
        d_buf.copy_(torch.from_numpy(buf_np))
        return P.decode_png(d_buf, d_sizes, h, w, check=False)

    def dev_pinned():
        d_buf.copy_(buf_pin, non_blocking=True)
        return P.decode_png(d_buf, d_sizes, h, w, check=False)

    def dev_resident():
        return P.decode_png(d_buf, d_sizes, h, w, check=False)

    pm = mp.hgru_pose.model()
    pm.load_weights(W.synth_weights(W.hgru_pose_vars(output_shape=69, timesteps=8, crop=128), seed=21))
    o0 = torch.from_numpy(W.synth_hidden((B, 64, 64, 64), seed=3)).to(dev)
    pm.build(torch.zeros((B, 128, 128, 1), device=dev), 69, h2_init=o0)
    pipe = T.DetectorPosePipeline(pm, mp.monkeydetector.MonkeyDetector(*CAM))
    resident = torch.from_numpy(frames).to(dev)
    side = torch.cuda.Stream(dev)
    side_out = torch.empty((B, h, w), dtype=torch.uint16, device=dev)

    def forward():
        return pipe.run(resident, h2_init=o0)

    def forward_beside_decode():
        with torch.cuda.stream(side):
            P.decode_png(d_buf, d_sizes, h, w, out=side_out, check=False)
        return pipe.run(resident, h2_init=o0)

    forms = {"device_resident": dev_resident, "device_h2d_pageable": dev_pageable, "device_h2d_pinned": dev_pinned,
             "host_chain_lib": host_chain(lib_one), "forward_alone": forward, "forward_beside_decode": forward_beside_decode}
    if Image:
        forms["host_chain_pil"] = host_chain(pil_one)

    # correctness of what is timed, once
    d_buf.copy_(torch.from_numpy(buf_np))
    fr, st = dev_resident()
    sync()
    assert not st.cpu().numpy().any() and np.array_equal(fr.cpu().view(torch.int16).numpy().view(np.uint16), frames)
    for name, fn in forms.items():                       # warm-up: buffers, plans, the thread pool
        fn()
        sync()
    rounds = {k: [] for k in forms}
    for r in range(a.rounds):
        for name, fn in forms.items():
            ts = []
            for _ in range(a.calls):
                t0 = time.perf_counter()
                fn()
                sync()
                ts.append((time.perf_counter() - t0) * 1e3)
            rounds[name].append(ts)
        print(f"round {r}: " + ", ".join(f"{k} {np.median(v[-1]):.2f}" for k, v in rounds.items()), flush=True)
    res["ms"] = {k: spread(v) for k, v in rounds.items()}
    res["host_chain"] = "host_chain_pil" if Image else "host_chain_lib"

    # ---- each kernel alone: the device times torch.profiler records for the resident calls
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            for _ in range(a.calls):
                dev_resident()
            sync()
        ker = {}
        for e in prof.key_averages():
            if "pngdec_" in e.key:
                total = getattr(e, "device_time_total", None)
                if total is None:
                    total = e.cuda_time_total
                short = "parse" if "parse" in e.key else "inflate" if "inflate" in e.key else "unfilter"
                ker[short] = {"mean_ms": float(total) / e.count / 1e3, "count": int(e.count)}
        res["kernels"] = ker
        if syms and "inflate" in ker:
            res["inflate_symbols_per_s"] = syms / (ker["inflate"]["mean_ms"] * 1e-3)
            res["inflate_symbols_per_s_per_file"] = res["inflate_symbols_per_s"] / B
    except Exception as e:                               # the profiler is an extra: the host-clock rows stand without it
        res["kernels"] = None
        res["kernels_error"] = repr(e)
    m = res["ms"]
    res["side_stream"] = {"forward_alone_ms": m["forward_alone"]["p50_ms"], "decode_alone_ms": m["device_resident"]["p50_ms"],
                          "both_ms": m["forward_beside_decode"]["p50_ms"],
                          "hidden_ms": m["forward_alone"]["p50_ms"] + m["device_resident"]["p50_ms"]
                          - m["forward_beside_decode"]["p50_ms"]}
    print("RESULT " + json.dumps(res), flush=True)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pngdec", "time_png_decode.json"))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--batch", str(a.batch), "--rounds", str(a.rounds),
           "--calls", str(a.calls)]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=CHILD_LIMIT_S)
    sys.stdout.write(p.stdout)
    sys.stderr.write(p.stderr[-4000:])
    if p.returncode != 0:
        return p.returncode
    line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1]
    import bench
    doc = {"tool": "tools/time_png_decode.py", "tree_stamp": bench.tree_stamp(), **json.loads(line[7:])}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(f"wrote {a.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
