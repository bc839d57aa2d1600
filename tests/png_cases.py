"""The PNG encoder's cases (include/monkeypose_png.h, csrc/png_rule.hpp), shared by
tests/test_png_cpu.py (mp_png_encode_host, no GPU) and tests/test_gpu_png.py (mp_png_encode_dev against
it, byte for byte): the pictures, a reader that trusts nothing of the encoder, and the new header's
stream table.

Each picture is the smallest shape at which the thing its name says can go wrong:

    1x1                  4 raw bytes, below the minimum match
    zero-row-w86/87/88   one row of zeros, 259 / 262 / 265 raw bytes with the filter byte: a run either
                         side of the longest match (258) and a remainder below / at the minimum match
    const-zero-40        the filter byte joins the runs across rows
    const-colour-40      the filter byte breaks every run
    random-33x67         fixed Huffman expands: the stored form, sizes <= bound
    random-below-144     8-bit literals only: the fixed / stored tie region
    random-above-143     9-bit literals crossing word boundaries; larger than raw
    runs-1-260           runs of every length 1 .. 260 of two alternating values, width 700: every length
                         code 257 .. 285 and every extra-bit width
    rows3-wW             three identical random rows: the only matches are the pixel above (and its
                         neighbours), so the distance codes from 3 up are reached; from w = 1366 a band
                         is one row and has no row above (w = 1365 is the widest with two)
    bands-hH             heights of band rows - 1, band rows, band rows + 1 and 2 band rows + 1 at w = 100
    n3                   three different pictures in one call
    overlay-gray / -jet  render_overlays_np pictures, 424 x 512
"""
import functools
import os
import struct
import zlib

import numpy as np

import stream_order_cases as SO
from helpers import ROOT, pkg

PNG_HEADER = os.path.join(ROOT, "include", "monkeypose_png.h")
GOLDEN_DIR = os.path.join(ROOT, "tests", "golden", "png")
ROW_WIDTHS = (1, 2, 3, 5, 11, 22, 43, 86, 171, 342, 683, 1365, 1366, 2731, 4096)
BAND_W = 100
GOLDEN = ("1x1", "zero-row-w86", "zero-row-w87", "zero-row-w88", "const-colour-40", "random-above-143")
SIGNATURE = b"\x89PNG\r\n\x1a\n"


def P():
    return pkg().png


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def _runs():
    w, vals = 700, (7, 200)
    seq = np.concatenate([np.full(L, vals[L % 2], np.uint8) for L in range(1, 261)])
    rows = -(-seq.size // (3 * w))
    tail = np.resize(np.asarray(vals, np.uint8), rows * 3 * w - seq.size)      # alternating: runs of 1
    return np.concatenate([seq, tail]).reshape(1, rows, w, 3)


def _bands(name, h):
    rng = _rng(name)
    base = (rng.integers(0, 4, (1, h, BAND_W, 1)) * 60).astype(np.uint8)
    img = np.repeat(base, 3, axis=3)
    img[0, 1::3] = img[0, 0::3][: img[0, 1::3].shape[0]]                        # a third of the rows repeat the one above
    img[0, :, 5, 1] = rng.integers(0, 256, h)                                   # and some 9-bit literals
    return img


def _overlay(lut):
    Pk = pkg()
    fr = Pk.weights.synth_frames(1, seed=14)[..., 0]
    mm = np.round(fr * np.float32(10000.0)).astype(np.uint16)
    rng = np.random.default_rng(5)
    ju = np.empty((1, 2, 23, 3), np.float32)
    ju[..., 0] = np.clip(250 + np.cumsum(rng.uniform(-30, 30, (1, 2, 23)), axis=2), 0, 511)
    ju[..., 1] = np.clip(200 + np.cumsum(rng.uniform(-30, 30, (1, 2, 23)), axis=2), 0, 423)
    ju[..., 2] = rng.uniform(1000, 3000, (1, 2, 23))
    return Pk.monkeydetector.render_overlays_np(mm, ju, bones=[(k, k + 1) for k in range(22)],
                                                depth_range=(1000, 3000), lut=lut)


def _n3():
    rng = _rng("n3")
    h, w = 20, 30
    smooth = (np.add.outer(np.arange(h), np.arange(w))[..., None] * np.array([3, 5, 0]) % 256).astype(np.uint8)
    noise = rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
    const = np.broadcast_to(np.array([10, 200, 30], np.uint8), (h, w, 3))
    return np.stack([smooth, noise, const])


def _makers():
    m = {"1x1": lambda: _rng("1x1").integers(0, 256, (1, 1, 1, 3)).astype(np.uint8)}
    for w in (86, 87, 88):
        m[f"zero-row-w{w}"] = functools.partial(np.zeros, (1, 1, w, 3), np.uint8)
    m["const-zero-40"] = lambda: np.zeros((1, 40, 40, 3), np.uint8)
    m["const-colour-40"] = lambda: np.ascontiguousarray(np.broadcast_to(np.array([10, 200, 30], np.uint8), (1, 40, 40, 3)))
    m["random-33x67"] = lambda: _rng("random").integers(0, 256, (1, 33, 67, 3)).astype(np.uint8)
    m["random-below-144"] = lambda: _rng("below").integers(0, 144, (1, 33, 67, 3)).astype(np.uint8)
    m["random-above-143"] = lambda: _rng("above").integers(144, 256, (1, 9, 9, 3)).astype(np.uint8)
    m["runs-1-260"] = _runs
    for w in ROW_WIDTHS:
        m[f"rows3-w{w}"] = functools.partial(
            lambda w: np.repeat(_rng(f"rows{w}").integers(0, 256, (1, 1, w, 3)).astype(np.uint8), 3, axis=1), w)
    m["n3"] = _n3
    m["overlay-gray"] = functools.partial(_overlay, "gray")
    m["overlay-jet"] = functools.partial(_overlay, "jet")
    return m


BAND_CASES = ("bands-rows-1", "bands-rows", "bands-rows+1", "bands-2rows+1")
NAMES = tuple(_makers()) + BAND_CASES


@functools.lru_cache(maxsize=None)
def picture(name):
    """the case's pictures [n, h, w, 3] uint8, read-only and shared"""
    if name in BAND_CASES:
        rows = P().band_plan(1, BAND_W)[0]
        h = {"bands-rows-1": rows - 1, "bands-rows": rows, "bands-rows+1": rows + 1, "bands-2rows+1": 2 * rows + 1}[name]
        a = _bands(name, h)
    else:
        a = _makers()[name]()
    a = np.ascontiguousarray(a, np.uint8)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def host_files(name):
    """(buf, sizes) of the case through mp_png_encode_host, computed once: the reference of the device"""
    buf, sizes = P().encode_png(picture(name))
    buf.setflags(write=False)
    sizes.setflags(write=False)
    return buf, sizes


# ------------------------------------------------------------------------------------------ the reader
def chunks(data):
    """[(type, data)] of a PNG file; the signature and every chunk's CRC-32 are checked"""
    assert data[:8] == SIGNATURE
    out, p = [], 8
    while p < len(data):
        (n,) = struct.unpack(">I", data[p:p + 4])
        typ, body = data[p + 4:p + 8], data[p + 8:p + 8 + n]
        assert len(body) == n and p + 12 + n <= len(data), "a chunk runs past the file"
        assert struct.unpack(">I", data[p + 8 + n:p + 12 + n])[0] == zlib.crc32(typ + body), f"CRC of {typ}"
        out.append((typ, body))
        p += 12 + n
    assert p == len(data)
    return out


def read_png(data, h, w):
    """the pixels [h, w, 3] of an 8-bit RGB PNG file whose rows all carry filter 0; checks the chunk
    order and CRCs, the IHDR fields, the zlib stream (header 78 01, BFINAL reached exactly at its end,
    the Adler-32) and the raw size"""
    ch = chunks(data)
    types = [t for t, _ in ch]
    assert types[0] == b"IHDR" and types[-1] == b"IEND" and set(types[1:-1]) == {b"IDAT"}, types
    assert ch[0][1] == struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0) and ch[-1][1] == b""
    z = b"".join(b for t, b in ch if t == b"IDAT")
    assert z[:2] == b"\x78\x01"
    d = zlib.decompressobj()
    raw = d.decompress(z)                        # raises on a bad block or a wrong Adler-32
    assert d.eof and d.unused_data == b"", "BFINAL is not where the stream ends"
    assert struct.unpack(">I", z[-4:])[0] == zlib.adler32(raw)
    rows = np.frombuffer(raw, np.uint8)
    assert rows.size == h * (1 + 3 * w)
    rows = rows.reshape(h, 1 + 3 * w)
    assert not rows[:, 0].any(), "a row's filter byte is not 0"
    return rows[:, 1:].reshape(h, w, 3)


def band_data(data, h, w):
    """the raw bytes each band's IDAT inflates to by itself, with the band plan checked on the way: one
    IDAT a band and a 4-byte one for the Adler-32; a band's chunk (after 78 01 in band 0) is a complete
    run of deflate blocks that ends on its last byte with an empty stored block, BFINAL in the last alone"""
    rows, nb = P().band_plan(h, w)
    assert (rows, nb) == (max(1, 8192 // (1 + 3 * w)), -(-h // rows))
    idat = [b for t, b in chunks(data) if t == b"IDAT"]
    assert len(idat) == nb + 1 and len(idat[-1]) == 4
    out = []
    for k, body in enumerate(idat[:-1]):
        if k == 0:
            body = body[2:]
        assert body[-4:] == b"\x00\x00\xff\xff"
        d = zlib.decompressobj(-15)
        raw = d.decompress(body)
        assert d.unused_data == b"" and d.unconsumed_tail == b"" and d.eof == (k == nb - 1)
        assert len(raw) == min(rows, h - k * rows) * (1 + 3 * w), f"band {k} holds {len(raw)} raw bytes"
        first = body[0] & 7                      # BFINAL 0; BTYPE 01 (fixed) or 00 (stored)
        assert first in (0b010, 0b000)
        assert len(body) <= len(raw) + 10        # never longer than its stored form
        out.append(raw)
    return out


# ------------------------------------------------------------------------------------------ streams
class PngCase(SO.Case):
    """encode_png on the caller's stream into buffers the case owns; the bytes past each file's end are
    masked on the same stream, so an output is a function of the input alone"""
    name = "png_encode"
    covers = ("mp_png_encode_dev",)
    outputs = ("png", "sizes")
    SHAPE = (2, 40, 50, 3)

    def __init__(self, draw=0):
        self.draw = draw            # another draw of the pictures: the second of two concurrent calls
        self.name = f"png_encode-{draw}" if draw else "png_encode"

    def make(self, seed):
        rng = np.random.default_rng(910 + seed + 100 * self.draw)
        a = (rng.integers(0, 6, self.SHAPE) * 50).astype(np.uint8)
        a[:, 10:20] = a[:, 9:10]
        return {"rgb": a}

    def alloc(self):
        import torch
        n, h, w, _ = self.SHAPE
        self.out = {"png": torch.full((n, P().png_bound(h, w)), 255, dtype=torch.uint8, device="cuda"),
                    "sizes": torch.zeros(n, dtype=torch.int64, device="cuda")}

    def invoke(self):
        import torch
        buf, sizes = P().encode_png(self.inp["rgb"], out=(self.out["png"], self.out["sizes"]))
        col = torch.arange(buf.shape[1], device=buf.device)
        return {"png": torch.where(col[None, :] < sizes[:, None], buf, torch.zeros_like(buf)), "sizes": sizes}

    def check_plain(self, A, got):
        ref, rs = P().encode_png(A["rgb"])
        assert np.array_equal(got["sizes"], rs)
        for i, s in enumerate(rs):
            assert got["png"][i, :s].tobytes() == ref[i, :s].tobytes()


PNG_STREAM_CASES = (PngCase,)
PNG_ORDERED = {}
for _c in PNG_STREAM_CASES:
    for _fn in _c.covers:
        PNG_ORDERED.setdefault(_fn, []).append(_c.name)
