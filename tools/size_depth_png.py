"""Bytes per frame of png.encode_depth_png's files (the host encoder: the device writes the same bytes)
for a few kinds of 424 x 512 depth frames, beside the raw frame, PIL's default save and zlib level 6 of
the rule's own filtered rows.  No GPU.  Prints a markdown table (profiles/png16/README.md).

    python tools/size_depth_png.py
"""
import importlib
import io
import os
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def kinds():
    mp = importlib.import_module("monkey-pose_amd")
    rng = np.random.default_rng(7)
    h, w = 424, 512
    synth = np.round(mp.weights.synth_frames(4, seed=14)[..., 0] * np.float32(10000.0)).astype(np.uint16)
    yy, xx = np.mgrid[:h, :w]
    smooth = 1500 + 0.8 * xx + 0.5 * yy + 60 * np.sin(xx / 40.0) * np.cos(yy / 55.0)
    gated = np.where((synth > 1000) & (synth < 3000), synth, 10000).astype(np.uint16)
    return {
        "synth_frames, mm": synth,
        "smooth surface, noise of +-4 mm": (smooth[None] + rng.integers(-4, 5, (2, h, w))).astype(np.uint16),
        "smooth surface, no noise": smooth[None].astype(np.uint16),
        "synth_frames gated to [1000, 3000], background 10000": gated,
        "constant": np.full((1, h, w), 2500, np.uint16),
        "uniform random": rng.integers(0, 65536, (1, h, w)).astype(np.uint16),
    }


def main():
    from PIL import Image
    import png16_cases as C
    P = importlib.import_module("monkey-pose_amd").png
    print("| frames | raw | this rule | of raw | PIL default | rule / PIL | zlib 6 of the rule's rows | dynamic / fixed / stored bands |")
    print("|---|---|---|---|---|---|---|---|")
    for name, x in kinds().items():
        _, sizes = P.encode_depth_png(x)
        st = P.depth_band_stats(x)
        pil, z6 = [], []
        for fr in x:
            b = io.BytesIO()
            Image.fromarray(fr).save(b, "PNG")
            pil.append(len(b.getvalue()))
            z6.append(len(zlib.compress(C.filtered_rows(fr).tobytes(), 6)))
        forms = np.bincount(st[..., 0].ravel(), minlength=3)
        ours, pilm = float(np.mean(sizes)), float(np.mean(pil))
        print(f"| {name} | {x[0].nbytes:,} | {ours:,.0f} | {100 * ours / x[0].nbytes:.1f} % | {pilm:,.0f} | {ours / pilm:.2f} | "
              f"{np.mean(z6):,.0f} | {forms[2]} / {forms[1]} / {forms[0]} |")
    return 0


if __name__ == "__main__":
    sys.exit(main())
