"""Converts a directory of recorded camera frames to 16-bit grayscale PNG files on the device.

Every ``*.npy`` frame of SRC (uint16, stored [w, h] as the recordings are) is uploaded as it is,
transposed on the device and encoded there (png.encode_depth_png: per-row filters, a dynamic Huffman
code per band; csrc/png16_rule.hpp), ``--batch`` frames a call: only the compressed bytes cross back
to the host, where they are written as DST/depth_%06d.png in the sorted order of the sources -- the
[h, w] files the importer's loadDepthMap, png.decode_png_files and eval_model_on_real_data (with a
``transposed=False`` pipeline) read.  DST/files.txt lists the sources, one per line, in that order.
``--host`` encodes on the host by the same rule instead: the same bytes, no GPU.

    python tools/npy_to_png.py SRC DST [--batch 16] [--host]
"""
import argparse
import glob
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def convert(src, dst, batch=16, host=False):
    """-> (the source files in order, raw bytes, PNG bytes)"""
    png = importlib.import_module("monkey-pose_amd").png
    files = sorted(glob.glob(os.path.join(src, "*.npy")))
    if not files:
        raise ValueError(f"no .npy frames in {src!r}")
    if batch <= 0:
        raise ValueError(f"--batch must be positive, got {batch}")
    first = None
    for f in files:                                  # the headers alone, before any frame is encoded
        a = np.load(f, mmap_mode="r", allow_pickle=False)
        if a.ndim != 2 or a.dtype != np.uint16:
            raise ValueError(f"{f}: expected a 2-D uint16 frame, got {a.dtype} {a.shape}")
        if first is None:
            first = a.shape
        elif a.shape != first:
            raise ValueError(f"{f}: frame is {a.shape}, but {files[0]} is {first}")
        del a
    os.makedirs(dst, exist_ok=True)
    raw = out = 0
    for i in range(0, len(files), batch):
        stack = np.stack([np.load(f, allow_pickle=False) for f in files[i:i + batch]])     # [n, w, h]
        if host:
            frames = np.ascontiguousarray(stack.transpose(0, 2, 1))
        else:
            import torch
            dev = torch.from_numpy(stack.view(np.int16)).cuda()       # the same bits: every torch copy takes int16
            frames = dev.transpose(1, 2).contiguous().view(torch.uint16)
        paths = [os.path.join(dst, f"depth_{i + k:06d}.png") for k in range(len(stack))]
        png.save_depth_maps(paths, frames)
        raw += stack.nbytes
        out += sum(os.path.getsize(p) for p in paths)
    with open(os.path.join(dst, "files.txt"), "w") as f:
        f.write("\n".join(files) + "\n")
    return files, raw, out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("src")
    ap.add_argument("dst")
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--host", action="store_true", help="encode on the host (the same bytes)")
    args = ap.parse_args(argv)
    files, raw, out = convert(args.src, args.dst, args.batch, args.host)
    print(f"{len(files)} frames: {raw} raw bytes -> {out} PNG bytes ({raw / out:.2f}x) in {args.dst}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
