"""Times png.encode_depth_png (mp_png16_encode_dev, csrc/k_png16.hip) at B = 256 frames of 424 x 512
(weights.synth_frames at mm scale, 16 distinct frames repeated), p50 over --calls calls after warm-up:

  device   encode_depth_png on resident frames, then png.png_files: the D2H of sizes, of the used
           columns, and the bytes objects (host clock around work that ends in a host wait)
  host     the chain it replaces: D2H of the raw frames into pinned memory, then PIL's default
           Image.save of every frame on --threads threads (file writes excluded: BytesIO)
  kernels  encode_depth_png alone (device events around both kernels), beside its byte floor: the frames
           read and the files written at the copy rate a device-to-device copy of 512 MiB reaches here
  sizes    bytes per frame of the device's files and of PIL's

Writes one JSON document (default profiles/png16/time_depth_png.json).  With --repeat-only N it only
encodes N times (for a kernel trace of its own).

    python tools/time_depth_png.py [--calls 20] [--batch 256] [--threads 16] [--out FILE] [--repeat-only N]
"""
import argparse
import importlib
import io
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def p50(xs):
    return float(np.median(np.asarray(xs)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "png16", "time_depth_png.json"))
    ap.add_argument("--repeat-only", type=int, default=0)
    a = ap.parse_args()
    import torch
    from PIL import Image
    mp = importlib.import_module("monkey-pose_amd")
    P = mp.png
    mm = np.round(mp.weights.synth_frames(16, seed=14)[..., 0] * np.float32(10000.0)).astype(np.uint16)
    frames = np.ascontiguousarray(np.tile(mm, (-(-a.batch // 16), 1, 1))[:a.batch])
    n, h, w = frames.shape
    dev = torch.from_numpy(frames).cuda()
    if a.repeat_only:
        for _ in range(a.repeat_only):
            P.encode_depth_png(dev)
        torch.cuda.synchronize()
        return 0

    def device_route():
        return P.png_files(*P.encode_depth_png(dev))

    pinned = torch.empty(frames.shape, dtype=torch.uint16).pin_memory()
    pool = ThreadPoolExecutor(a.threads)

    def pil_save(fr):
        b = io.BytesIO()
        Image.fromarray(fr).save(b, "PNG")
        return b.getvalue()

    def host_route():
        pinned.copy_(dev)                            # synchronous: the frames are on the host when it returns
        return list(pool.map(pil_save, pinned.numpy()))

    def host_clock(fn, calls):
        for _ in range(2):
            fn()
        ts = []
        for _ in range(calls):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        return p50(ts), out

    def events(fn, calls):
        for _ in range(3):
            fn()
        ts = []
        for _ in range(calls):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        return p50(ts)

    dev_ms, files = host_clock(device_route, a.calls)
    host_ms, pil = host_clock(host_route, max(3, a.calls // 4))
    enc_ms = events(lambda: P.encode_depth_png(dev), a.calls)
    probe = torch.empty(512 << 20, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(probe)
    copy_ms = events(lambda: dst.copy_(probe), 10)
    rate = 2 * probe.numel() / (copy_ms * 1e-3)      # bytes read and written per second
    file_bytes = sum(map(len, files))
    floor_ms = (frames.nbytes + file_bytes) / rate * 1e3
    hb, hs = P.encode_depth_png(frames[:4])
    doc = {"tool": "tools/time_depth_png.py", "batch": n, "shape": [h, w], "calls": a.calls, "threads": a.threads,
           "device_encode_plus_d2h_ms": dev_ms, "host_d2h_plus_pil_save_ms": host_ms, "host_over_device": host_ms / dev_ms,
           "encode_kernels_ms": enc_ms, "copy_rate_GBps": rate / 1e9, "byte_floor_ms": floor_ms,
           "kernels_over_floor": enc_ms / floor_ms, "raw_bytes_per_frame": h * w * 2,
           "file_bytes_per_frame": file_bytes / n, "pil_bytes_per_frame": sum(map(len, pil)) / n,
           "device_equals_host_first4": bool(files[:4] == P.png_files(hb, hs)),
           "lib": os.environ.get("MP_LIB_PATH", "")}
    print(json.dumps(doc))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
