"""The 16-bit depth PNG encoder's cases (include/monkeypose_png16.h, csrc/png16_rule.hpp), shared by
tests/test_png16_cpu.py (mp_png16_encode_host, no GPU) and tests/test_gpu_png16.py (mp_png16_encode_dev
against it, byte for byte): the frames, a reader that trusts nothing of the encoder, a numpy
restatement of the filter rule, and the new header's stream case.

Each frame is the smallest shape at which the thing its name says can go wrong:

    1x1, 1x2, 3x1        a band of 3, 5 and 9 bytes; at w = 1 the distance rb - 2 equals 1
    2x4096, 2x4095       one row per band: the longest band (8193 bytes) and the one below 8192
    9x512                a full band of 7 rows and a short one of 2
    8x512-seam           row 7 repeats row 6 plus a plane: Up / Paeth of the second band's first row
                         read the first band's last row
    zero-424x512         every match at distance 1 and 258 long but a band's last: one distance symbol
    const-20x30          a constant that is not zero: row 0 takes Sub, the others Up
    no-match-4x20        no three bytes repeat at a candidate distance
    random-9x512         uniform random uint16: every band stored
    byte-order           0x0102, 0 and 65535
    five-filters         rows built so that each of None, Sub, Up, Average and Paeth wins one
    deep-tree            one row of 3381 pixels whose Sub residuals have Fibonacci counts and no match,
                         found on the CPU (_deep_tree): the unlimited tree is deeper than 15
    synth-424x512        two weights.synth_frames frames at mm scale
    n3                   three different frames in one call
"""
import functools
import os
import struct
import zlib

import numpy as np

import png_cases as PC
import stream_order_cases as SO
from helpers import ROOT, pkg

PNG16_HEADER = os.path.join(ROOT, "include", "monkeypose_png16.h")
GOLDEN_DIR = os.path.join(ROOT, "tests", "golden", "png16")
GOLDEN = ("1x1", "3x1", "const-20x30", "no-match-4x20", "byte-order", "five-filters")
FORM_STORED, FORM_FIXED, FORM_DYNAMIC = 0, 1, 2
S_FORM, S_FILTERS, S_MATCHES, S_DIST, S_DEPTH = 0, slice(1, 6), 6, 7, 8


def P():
    return pkg().png


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def _seam():
    rng = _rng("seam")
    a = rng.integers(0, 65536, (1, 8, 512)).astype(np.uint16)
    a[0, 7] = a[0, 6] + np.arange(512, dtype=np.uint16) // 64            # the row above, plus a slow ramp
    return a


def _five_filters():
    rng = _rng("five")
    w = 64
    x = np.arange(w)
    rows = [rng.integers(0, 65536, w)]                                     # 0: noise -- whatever wins
    rows.append(rng.integers(0, 3, w))                                     # 1: small values: None
    rows.append((1000 + 257 * 3 * x) % 65536)                              # 2: a steep ramp: Sub
    rows.append(rng.integers(0, 65536, w))                                 # 3: noise
    rows.append((rows[3] + 257 * rng.integers(0, 2, w)) % 65536)           # 4: the row above, nearly: Up
    rows.append(rng.integers(0, 256, w) * 257)                             # 5: noise, equal bytes
    avg = np.zeros(w, np.int64)                                            # 6: floor((left + up) / 2) bytewise: Average
    for j in range(w):
        hi = ((avg[j - 1] >> 8 if j else 0) + (rows[5][j] >> 8)) >> 1
        lo = ((avg[j - 1] & 255 if j else 0) + (rows[5][j] & 255)) >> 1
        avg[j] = hi << 8 | lo
    rows.append(avg)
    rows.append(rng.integers(0, 200, w) * 257)                             # 7: noise below 200, equal bytes
    rows.append(rows[7] + 257 * (x % 3) * 9)                               # 8: up + a sawtooth ..
    rows.append(rows[8] + 257 * rng.integers(0, 40, 1)[0] + 0 * x)         # 9: .. shifted: left + up - upleft: Paeth
    return np.stack(rows).astype(np.uint16)[None]


def _deep_tree():
    """A band whose symbol counts are 1, 1, 2, 3, 5, .. 2584 exactly, so that every Huffman merge takes
    the node made before it and the unlimited tree is a chain 17 deep.  One of the 1s is symbol 256; the
    others count the Sub residuals (bpp 2) -8, 8, -7, .. -1, 0, 1 of one row of 3381 pixels, the filter
    byte 1 among the 2584 ones.  The band positions 3, 6, 9, .. hold the values counted 13, 34, 610 and
    1597 times (2254 in all, as many as there are such positions) and the other positions the other
    values, each group shuffled.  A match of three bytes covers one position p = 0 mod 3 and compares
    it with p - 1, p - 2 or p - 4, none of which is: the band has no match and the counts stay as they
    are.  The raw bytes are the residuals' prefix sums, a random walk whose None cost is far above
    Sub's, so the residuals are what the rule's filter leaves."""
    fib = [1, 1]
    while len(fib) < 18:
        fib.append(fib[-1] + fib[-2])
    vals = [1, 0, -1, 2, -2, 3, -3, 4, -4, 5, -5, 6, -6, 7, -7, 8, -8][::-1]
    counts = fib[1:-1] + [fib[-1] - 1]                             # less symbol 256, less the filter byte
    third = (13, 34, 610, 1597)
    rng = np.random.default_rng(16)
    pools = [rng.permutation(np.concatenate([np.full(c, v, np.int64) for c, v in zip(counts, vals) if (c in third) == k]))
             for k in (True, False)]
    seq = np.ones(1 + sum(counts), np.int64)                       # position 0 is the filter byte
    at = np.arange(seq.size)
    seq[(at % 3 == 0) & (at > 0)], seq[at % 3 != 0] = pools
    res = seq[1:]
    raw = np.zeros(res.size, np.int64)
    raw[0::2] = np.cumsum(res[0::2]) % 256
    raw[1::2] = np.cumsum(res[1::2]) % 256
    return (raw[0::2] << 8 | raw[1::2]).astype(np.uint16).reshape(1, 1, res.size // 2)


def _synth():
    fr = pkg().weights.synth_frames(2, seed=14)[..., 0]
    return np.round(fr * np.float32(10000.0)).astype(np.uint16)


def _n3():
    rng = _rng("n3")
    h, w = 20, 30
    smooth = (1000 + 7 * np.add.outer(np.arange(h), np.arange(w)) + rng.integers(-4, 5, (h, w))).astype(np.uint16)
    noise = rng.integers(0, 65536, (h, w)).astype(np.uint16)
    const = np.full((h, w), 2500, np.uint16)
    return np.stack([smooth, noise, const])


def _makers():
    u16 = lambda a: np.asarray(a, np.uint16)
    return {
        "1x1": lambda: u16([[[0x0102]]]),
        "1x2": lambda: u16([[[0x0102, 0xfffe]]]),
        "3x1": lambda: u16([[[7], [7], [0x0102]]]),
        "2x4096": lambda: (3000 + _rng("4096").integers(-4, 5, (1, 2, 4096)).cumsum(axis=2)).astype(np.uint16),
        "2x4095": lambda: (_rng("4095").integers(0, 3, (1, 2, 4095)) * 500).astype(np.uint16),
        "9x512": lambda: (2000 + np.add.outer(3 * np.arange(9), np.arange(512) // 4)[None]
                          + _rng("9x512").integers(-4, 5, (1, 9, 512))).astype(np.uint16),
        "8x512-seam": _seam,
        "zero-424x512": lambda: np.zeros((1, 424, 512), np.uint16),
        "const-20x30": lambda: np.full((1, 20, 30), 0x1234, np.uint16),
        "no-match-4x20": lambda: _rng("nomatch").integers(0, 65536, (1, 4, 20)).astype(np.uint16),
        "random-9x512": lambda: _rng("random").integers(0, 65536, (1, 9, 512)).astype(np.uint16),
        "byte-order": lambda: u16([[[0x0102, 0, 65535, 0x0102], [65535, 0x0102, 0, 0], [0, 65535, 0x0102, 65535]]]),
        "five-filters": _five_filters,
        "deep-tree": _deep_tree,
        "synth-424x512": _synth,
        "n3": _n3,
    }


NAMES = tuple(_makers())


@functools.lru_cache(maxsize=None)
def frames(name):
    """the case's frames [n, h, w] uint16, read-only and shared"""
    a = np.ascontiguousarray(_makers()[name](), np.uint16)
    assert a.ndim == 3
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def host_files(name):
    """(buf, sizes) of the case through mp_png16_encode_host, computed once: the reference of the device"""
    buf, sizes = P().encode_depth_png(frames(name))
    buf.setflags(write=False)
    sizes.setflags(write=False)
    return buf, sizes


@functools.lru_cache(maxsize=None)
def stats(name):
    """mp_png16_band_stats_host of the case: int32 [n, bands, 9]"""
    s = P().depth_band_stats(frames(name))
    s.setflags(write=False)
    return s


# ------------------------------------------------------------------------------------------ the reader
def filtered_rows(frame):
    """the rule's raw stream of one frame [h, w] -> uint8 [h, 1 + 2 w], restated in numpy: big-endian
    bytes, the five filters with bpp 2 against the frame's row above (zeros above row 0), the smallest
    sum of |int8 residual|, ties to the smallest filter number"""
    h, w = frame.shape
    raw = np.zeros((h + 1, 2 * w + 2), np.int64)                  # a zero row above, two zero bytes to the left
    raw[1:, 2::2], raw[1:, 3::2] = frame >> 8, frame & 255
    out = np.zeros((h, 1 + 2 * w), np.uint8)
    for r in range(h):
        x, a, b, c = raw[r + 1, 2:], raw[r + 1, :-2], raw[r, 2:], raw[r, :-2]
        q = a + b - c
        pa, pb, pc = abs(q - a), abs(q - b), abs(q - c)
        paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
        res = [(x - p) & 255 for p in (0 * x, a, b, (a + b) >> 1, paeth)]
        cost = [int(np.where(v < 128, v, 256 - v).sum()) for v in res]
        f = int(np.argmin(cost))                                   # the first of equal minima
        out[r, 0], out[r, 1:] = f, res[f]
    return out


def unfiltered(rows, h, w):
    """uint8 [h, 1 + 2 w] of any filters -> the frame, by the PNG specification's reconstruction"""
    rec = np.zeros((h + 1, 2 * w + 2), np.int64)
    for r in range(h):
        f = int(rows[r, 0])
        assert f <= 4
        for j in range(2 * w):
            a, b, c = rec[r + 1, j], rec[r, j + 2], rec[r, j]
            q = a + b - c
            pa, pb, pc = abs(q - a), abs(q - b), abs(q - c)
            pred = (0, a, b, (a + b) >> 1, a if pa <= pb and pa <= pc else (b if pb <= pc else c))[f]
            rec[r + 1, j + 2] = (int(rows[r, 1 + j]) + pred) & 255
    return (rec[1:, 2::2] << 8 | rec[1:, 3::2]).astype(np.uint16)


def raw_stream(data, h, w):
    """the raw rows uint8 [h, 1 + 2 w] a file's joined IDAT data inflates to; checks the chunk order and
    CRCs, the IHDR fields (bit depth 16, colour type 0), the zlib stream (header 78 01, BFINAL reached
    exactly at its end, the Adler-32) and the band plan: one IDAT a band, each a complete run of deflate
    blocks that ends with an empty stored block, and a 4-byte one for the Adler-32"""
    ch = PC.chunks(data)
    types = [t for t, _ in ch]
    assert types[0] == b"IHDR" and types[-1] == b"IEND" and set(types[1:-1]) == {b"IDAT"}, types
    assert ch[0][1] == struct.pack(">IIBBBBB", w, h, 16, 0, 0, 0, 0) and ch[-1][1] == b""
    idat = [b for t, b in ch if t == b"IDAT"]
    rows, nb = P().depth_band_plan(h, w)
    assert (rows, nb) == (max(1, 8192 // (1 + 2 * w)), -(-h // rows))
    assert len(idat) == nb + 1 and len(idat[-1]) == 4
    for k, body in enumerate(idat[:-1]):
        body = body[2:] if k == 0 else body
        assert body[-4:] == b"\x00\x00\xff\xff"
        d = zlib.decompressobj(-15)
        part = d.decompress(body)
        assert d.unused_data == b"" and d.eof == (k == nb - 1)
        assert len(part) == min(rows, h - k * rows) * (1 + 2 * w), f"band {k} holds {len(part)} raw bytes"
        assert len(body) <= len(part) + 10                        # never longer than its stored form
    z = b"".join(idat)
    assert z[:2] == b"\x78\x01"
    d = zlib.decompressobj()
    raw = d.decompress(z)
    assert d.eof and d.unused_data == b""
    assert struct.unpack(">I", z[-4:])[0] == zlib.adler32(raw)
    assert len(raw) == h * (1 + 2 * w)
    return np.frombuffer(raw, np.uint8).reshape(h, 1 + 2 * w)


def band_forms(data, h, w):
    """BTYPE of each band's first block, as the stats count them: 0 stored, 1 fixed, 2 dynamic"""
    idat = [b for t, b in PC.chunks(data) if t == b"IDAT"][:-1]
    return [((body[2] if k == 0 else body[0]) >> 1) & 3 for k, body in enumerate(idat)]


# ------------------------------------------------------------------------------------------ streams
class Png16Case(SO.Case):
    """encode_depth_png on the caller's stream into buffers the case owns; the bytes past each file's end
    are masked on the same stream, so an output is a function of the input alone (png_cases.PngCase's
    method, with depth frames)"""
    name = "png16_encode"
    covers = ("mp_png16_encode_dev",)
    outputs = ("png", "sizes")
    SHAPE = (2, 40, 50)

    def __init__(self, draw=0):
        self.draw = draw            # another draw of the frames: the second of two concurrent calls
        self.name = f"png16_encode-{draw}" if draw else "png16_encode"

    def make(self, seed):
        rng = np.random.default_rng(1610 + seed + 100 * self.draw)
        a = (1500 + 11 * np.add.outer(np.arange(40), np.arange(50))[None] + rng.integers(-3, 4, self.SHAPE)).astype(np.uint16)
        a[:, 10:20] = a[:, 9:10]
        a[1, 25:] = rng.integers(0, 65536, (15, 50))
        return {"frames": a}

    def alloc(self):
        import torch
        n, h, w = self.SHAPE
        self.out = {"png": torch.full((n, P().depth_png_bound(h, w)), 255, dtype=torch.uint8, device="cuda"),
                    "sizes": torch.zeros(n, dtype=torch.int64, device="cuda")}

    def invoke(self):
        import torch
        buf, sizes = P().encode_depth_png(self.inp["frames"], out=(self.out["png"], self.out["sizes"]))
        col = torch.arange(buf.shape[1], device=buf.device)
        return {"png": torch.where(col[None, :] < sizes[:, None], buf, torch.zeros_like(buf)), "sizes": sizes}

    def check_plain(self, A, got):
        ref, rs = P().encode_depth_png(A["frames"])
        assert np.array_equal(got["sizes"], rs)
        for i, s in enumerate(rs):
            assert got["png"][i, :s].tobytes() == ref[i, :s].tobytes()


PNG16_STREAM_CASES = (Png16Case,)
PNG16_ORDERED = {}
for _c in PNG16_STREAM_CASES:
    for _fn in _c.covers:
        PNG16_ORDERED.setdefault(_fn, []).append(_c.name)
