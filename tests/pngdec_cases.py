"""The PNG decoder's corpus (include/monkeypose_pngdec.h, csrc/pngdec_rule.hpp), shared by
tests/test_pngdec_cpu.py (mp_png_decode_host, no GPU) and tests/test_gpu_pngdec.py (mp_png_decode_dev
against it).  The files are written here, so that no test needs PIL or cv2: a small PNG writer (a
chosen filter per row, filtered in numpy, compressed by zlib at a chosen level / strategy / window and
flush points, cut into IDAT chunks at chosen places) and a bit writer for hand-assembled deflate
blocks, each of which is first shown to inflate under zlib to the bytes it was assembled from.

tests/golden/pngdec/ holds three files written by PIL 12.2 (``Image.fromarray(pix).save(path)``, mode I;16
for the 16-bit one) from ``_smooth(40, 50, fmt, seed=2)``: files of the reference's own library, decoded
here where PIL is absent.

``good()``  name -> Good(data, h, w, fmt, pixels): the pixels are the writer's source (or, for a
            hand-assembled stream, zlib's output unfiltered by the plain reader below)
``bad()``   name -> Bad(data, h, w, fmt, status, zlib_refuses): one file per status code and per
            bullet of the rule; where zlib has a verdict on the stream it is asserted here
"""
import collections
import functools
import os
import struct
import zlib

import numpy as np

import stream_order_cases as SO
from helpers import ROOT, pkg

PNGDEC_HEADER = os.path.join(ROOT, "include", "monkeypose_pngdec.h")
GOLDEN_DIR = os.path.join(ROOT, "tests", "golden", "pngdec")
GOLDEN = ("pil-gray16-40x50", "pil-gray8-40x50", "pil-rgb8-40x50")
SIGNATURE = b"\x89PNG\r\n\x1a\n"
FORMATS = ("gray16", "gray8", "rgb8")
BPP = {"gray16": 2, "gray8": 1, "rgb8": 3}
IHDR_KIND = {"gray16": (16, 0), "gray8": (8, 0), "rgb8": (8, 2)}
UNFILTER_ROWS = 256                      # k_pngdec.hip's UNF_ROWS: rows of one pass of the unfilter kernel
ST_CONTAINER, ST_CRC, ST_UNSUPPORTED, ST_MISMATCH, ST_STREAM, ST_ADLER, ST_FILTER = range(1, 8)

Good = collections.namedtuple("Good", "data h w fmt pixels")
Bad = collections.namedtuple("Bad", "data h w fmt status zlib_refuses")


def P():
    return pkg().png


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


# ------------------------------------------------------------------------------------------ the writer
def chunk(typ, body=b""):
    return struct.pack(">I", len(body)) + typ + body + struct.pack(">I", zlib.crc32(typ + body))


def ihdr(h, w, fmt, interlace=0, depth=None, ctype=None, comp=0, filt=0):
    d, c = IHDR_KIND[fmt]
    return chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, d if depth is None else depth, c if ctype is None else ctype,
                                      comp, filt, interlace))


def row_bytes(pix, fmt):
    """the pixels as the file's rows [h, w * bpp] uint8 (16-bit samples big-endian)"""
    h = pix.shape[0]
    if fmt == "gray16":
        return pix.astype(">u2").view(np.uint8).reshape(h, -1)
    return np.ascontiguousarray(pix, np.uint8).reshape(h, -1)


def _paeth(a, b, c):
    a, b, c = a.astype(np.int32), b.astype(np.int32), c.astype(np.int32)
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    return np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c)).astype(np.uint8)


def _filtered(cur, up, bpp, t):
    a = np.concatenate([np.zeros(bpp, np.uint8), cur[:-bpp]]) if cur.size > bpp else np.zeros_like(cur)
    a = a[:cur.size]
    c = np.concatenate([np.zeros(bpp, np.uint8), up[:-bpp]])[:cur.size] if cur.size > bpp else np.zeros_like(cur)
    if t == 0:
        return cur
    if t == 1:
        return cur - a
    if t == 2:
        return cur - up
    if t == 3:
        return cur - ((a.astype(np.int32) + up.astype(np.int32)) >> 1).astype(np.uint8)
    return cur - _paeth(a, up, c)


def raw_stream(pix, fmt, filters):
    """the filtered rows with their filter bytes; ``filters`` an int, a sequence cycled over the rows,
    or 'adaptive' (the least sum of absolute values as signed bytes, ties to the lowest type)"""
    rows, bpp = row_bytes(pix, fmt), BPP[fmt]
    out, up = [], np.zeros(rows.shape[1], np.uint8)
    for r, cur in enumerate(rows):
        if isinstance(filters, str):
            cands = [_filtered(cur, up, bpp, t) for t in range(5)]
            t = int(np.argmin([np.abs(c.view(np.int8).astype(np.int32)).sum() for c in cands]))
            f = cands[t]
        else:
            t = filters if isinstance(filters, int) else filters[r % len(filters)]
            f = _filtered(cur, up, bpp, t)
        out.append(bytes([t]) + f.tobytes())
        up = cur
    return b"".join(out)


def deflate(raw, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, wbits=15, flush_at=()):
    co = zlib.compressobj(level, zlib.DEFLATED, wbits, 9, strategy)
    out, p = [], 0
    for q in flush_at:
        out += [co.compress(raw[p:q]), co.flush(zlib.Z_SYNC_FLUSH)]
        p = q
    return b"".join(out) + co.compress(raw[p:]) + co.flush()


def cut(z, cuts):
    """the IDAT chunks of the stream z: ``cuts`` an int (chunk size) or the cut positions"""
    if isinstance(cuts, int):
        cuts = range(cuts, len(z), cuts)
    edges = [0] + list(cuts) + [len(z)]
    return b"".join(chunk(b"IDAT", z[a:b]) for a, b in zip(edges[:-1], edges[1:]))


def wrap(z, h, w, fmt, cuts=(), before=b"", after=b""):
    return SIGNATURE + ihdr(h, w, fmt) + before + cut(z, cuts) + after + chunk(b"IEND")


def write_png(pix, fmt, filters=0, cuts=(), before=b"", after=b"", **kw):
    h, w = pix.shape[:2]
    return wrap(deflate(raw_stream(pix, fmt, filters), **kw), h, w, fmt, cuts, before, after)


# ------------------------------------------------------------------------------------------ a plain reader
def unfilter(raw, h, w, fmt):
    """the pixels of a raw stream, byte by byte as the specification words it"""
    bpp = BPP[fmt]
    rb = w * bpp
    assert len(raw) == h * (1 + rb)
    out = np.zeros((h, rb), np.int32)
    for r in range(h):
        t = raw[r * (1 + rb)]
        assert t <= 4
        x = raw[r * (1 + rb) + 1:(r + 1) * (1 + rb)]
        for i in range(rb):
            a = out[r, i - bpp] if i >= bpp else 0
            b = out[r - 1, i] if r else 0
            c = out[r - 1, i - bpp] if r and i >= bpp else 0
            if t == 0:
                v = 0
            elif t == 1:
                v = a
            elif t == 2:
                v = b
            elif t == 3:
                v = (a + b) >> 1
            else:
                p = a + b - c
                pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
                v = a if pa <= pb and pa <= pc else (b if pb <= pc else c)
            out[r, i] = (x[i] + v) & 255
    return from_rows(out.astype(np.uint8), h, w, fmt)


def from_rows(rows, h, w, fmt):
    if fmt == "gray16":
        return np.ascontiguousarray(rows).view(">u2").astype(np.uint16).reshape(h, w)
    return rows.reshape((h, w) if fmt == "gray8" else (h, w, 3)).copy()


# ------------------------------------------------------------------------------------------ the bit writer
class BitWriter:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def bits(self, v, n):
        """n bits of v, least significant first (header fields, extra bits)"""
        self.acc |= v << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, v, n):
        """a Huffman code of n bits, most significant first"""
        for k in range(n - 1, -1, -1):
            self.bits((v >> k) & 1, 1)

    def align(self):
        if self.n:
            self.bits(0, 8 - self.n)

    def bytes(self):
        self.align()
        return bytes(self.out)


def canonical(lens):
    """symbol -> (code, length) of the canonical code with these lengths (RFC 1951 3.2.2)"""
    count = collections.Counter(l for l in lens if l)
    code, nxt = 0, {}
    for b in range(1, 16):
        code = (code + count.get(b - 1, 0)) << 1
        nxt[b] = code
    out = {}
    for s, l in enumerate(lens):
        if l:
            out[s] = (nxt[l], l)
            nxt[l] += 1
    return out


FIXED_LL = canonical([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8)
FIXED_DD = canonical([5] * 32)
LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073,
             4097, 6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0] + [e for e in range(1, 14) for _ in (0, 1)]


def put_tokens(bw, tokens, ll, dd, len_code=None):
    """tokens ('lit', v) / ('match', length, dist) / ('eob',) in the codes ll / dd; ``len_code`` forces
    the length symbol (285 for 258, or 284 with all extra bits set)"""
    for t in tokens:
        if t[0] == "lit":
            bw.code(*ll[t[1]])
        elif t[0] == "eob":
            bw.code(*ll[256])
        else:
            _, L, D = t[:3]
            ls = t[3] if len(t) > 3 else max(i for i, b in enumerate(LEN_BASE) if b <= L and (i < 28 or L == 258))
            assert 0 <= L - LEN_BASE[ls] < (1 << LEN_EXTRA[ls]) or L == LEN_BASE[ls]
            bw.code(*ll[257 + ls])
            bw.bits(L - LEN_BASE[ls], LEN_EXTRA[ls])
            ds = max(i for i, b in enumerate(DIST_BASE) if b <= D)
            bw.code(*dd[ds])
            bw.bits(D - DIST_BASE[ds], DIST_EXTRA[ds])


def expand(tokens):
    out = bytearray()
    for t in tokens:
        if t[0] == "lit":
            out.append(t[1])
        elif t[0] == "match":
            for _ in range(t[1]):
                out.append(out[-t[2]])
    return bytes(out)


CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
CL_LENS = [4] * 13 + [5] * 6             # a complete code over all 19 code-length symbols


def dynamic_header(bw, ll_lens, dd_lens, final=1, cl_lens=CL_LENS):
    """BFINAL, BTYPE 10 and the code lengths, run-length coded greedily over the joined sequence (a
    repeat runs from the literal / length lengths into the distance lengths where the values allow)"""
    bw.bits(final, 1)
    bw.bits(2, 2)
    bw.bits(len(ll_lens) - 257, 5)
    bw.bits(len(dd_lens) - 1, 5)
    bw.bits(19 - 4, 4)
    for s in CL_ORDER:
        bw.bits(cl_lens[s], 3)
    cl = canonical(cl_lens)
    seq, i, used = list(ll_lens) + list(dd_lens), 0, set()
    while i < len(seq):
        v, run = seq[i], 1
        while i + run < len(seq) and seq[i + run] == v:
            run += 1
        if v == 0 and run >= 3:
            n = min(run, 138)
            s, extra, nb = (17, n - 3, 3) if n <= 10 else (18, n - 11, 7)
            bw.code(*cl[s])
            bw.bits(extra, nb)
            i += n
        elif v and run >= 4:
            bw.code(*cl[v])
            n = min(run - 1, 6)
            bw.code(*cl[16])
            bw.bits(n - 3, 2)
            s = 16
            i += 1 + n
        else:
            s = v
            bw.code(*cl[v])
            i += 1
        used.add(s)
    return used


def zwrap(deflated, raw):
    return b"\x78\x01" + deflated + struct.pack(">I", zlib.adler32(raw))


def _hand(tokens, h, w, ll=None, dd=None, ll_lens=None, dd_lens=None):
    """a gray8 file of one hand-assembled block (fixed unless code lengths are given) -> Good, after
    zlib has inflated the stream to the tokens' bytes"""
    raw = expand(tokens)
    assert len(raw) == h * (1 + w), (len(raw), h, w)
    bw = BitWriter()
    if ll_lens is None:
        bw.bits(1, 1)
        bw.bits(1, 2)
        put_tokens(bw, tokens + [("eob",)], FIXED_LL, FIXED_DD)
    else:
        dynamic_header(bw, ll_lens, dd_lens)
        put_tokens(bw, tokens + [("eob",)], canonical(ll_lens), canonical(dd_lens))
    z = zwrap(bw.bytes(), raw)
    assert zlib.decompress(z) == raw, "zlib does not inflate the hand-assembled block to its bytes"
    return Good(wrap(z, h, w, "gray8"), h, w, "gray8", unfilter(raw, h, w, "gray8"))


def _every_code():
    """a fixed block with every length code 257 .. 285 and every distance code 0 .. 29 at both ends of
    its extra-bit range: 40 rows of 1 + 1023 bytes, the first 32768 bytes literals 0 .. 4 (so any of them
    is a legal filter byte)"""
    rng = _rng("every-code")
    toks = [("lit", int(v)) for v in rng.integers(0, 5, 32768)]
    lens = []
    for i in range(29):
        lens += [(LEN_BASE[i], i), (LEN_BASE[i] + (1 << LEN_EXTRA[i]) - 1, i)]
    dists = []
    for i in range(30):
        dists += [DIST_BASE[i], DIST_BASE[i] + (1 << DIST_EXTRA[i]) - 1]
    for k, d in enumerate(dists):
        L, ls = lens[k % len(lens)]
        toks.append(("match", L, d, ls))
        toks.append(("lit", int(rng.integers(0, 5))))
    assert {t[3] for t in toks if t[0] == "match"} == set(range(29)) and max(dists) == 32768
    n = len(expand(toks))
    h, w = 40, 1023
    assert n <= h * (1 + w)
    toks += [("lit", int(v)) for v in rng.integers(0, 5, h * (1 + w) - n)]
    return _hand(toks, h, w)


def _lens_1_to_15():
    """a dynamic block whose literal / length code has the lengths 1, 2, ..., 14, 15, 15"""
    syms = [0, 1, 2, 3, 4, 256] + list(range(257, 267))
    ll = [0] * 267
    for s, l in zip(syms, list(range(1, 15)) + [15, 15]):
        ll[s] = l
    toks = [("lit", 0), ("lit", 3), ("lit", 4), ("lit", 1), ("lit", 2)]
    for L in range(3, 13):                       # symbols 257 .. 266, the two 15-bit codes among them
        toks += [("match", L, 1 + L % 2), ("lit", L % 5)]
    toks.append(("match", 13, 2))               # 266 with its extra bit 0
    n = len(expand(toks))
    return _hand(toks, 1, n - 1, ll_lens=ll, dd_lens=[1, 1])


def _one_dist_code():
    """a dynamic block with a single distance code of 1 bit: an incomplete set zlib accepts"""
    ll = [0] * 258
    ll[0] = ll[1] = 2
    ll[256] = ll[257] = 2
    toks = [("lit", 0), ("lit", 1), ("lit", 1), ("match", 3, 1), ("lit", 0), ("match", 3, 1)]
    return _hand(toks, 1, len(expand(toks)) - 1, ll_lens=ll, dd_lens=[1])


def _repeat_codes():
    """code-length symbols 16, 17 and 18, a 16-repeat running from the literal / length lengths into the
    distance lengths"""
    ll = [0] * 286
    for s in (0, 1, 5, 6, 7, 256, 257):
        ll[s] = 3
    ll[284] = ll[285] = 4
    dd = [4] * 16
    bw = BitWriter()
    used = dynamic_header(bw, ll, dd)
    assert {16, 17, 18} <= used
    toks = [("lit", 0), ("lit", 5), ("lit", 6), ("lit", 7), ("lit", 1), ("match", 3, 2), ("match", 258, 5),
            ("match", 257, 16, 27), ("lit", 7)]
    return _hand(toks, 1, len(expand(toks)) - 1, ll_lens=ll, dd_lens=dd)


# ------------------------------------------------------------------------------------------ pictures
def _pix(name, h, w, fmt):
    rng = _rng(name)
    if fmt == "gray16":
        return rng.integers(0, 65536, (h, w)).astype(np.uint16)
    return rng.integers(0, 256, (h, w) if fmt == "gray8" else (h, w, 3)).astype(np.uint8)


def _smooth(h, w, fmt, seed=0):
    """a picture with structure (matches, all filters useful): a cut of a synth depth frame"""
    from oracle import crop_ref as CR
    fr = CR.synth_frame(seed).astype(np.uint16)[100:100 + h, 200:200 + w]
    if fmt == "gray16":
        return np.ascontiguousarray(fr)
    g = (fr >> 4).astype(np.uint8)
    return g if fmt == "gray8" else np.stack([g, g // 2, 255 - g], axis=-1)


def _g(pix, fmt, **kw):
    h, w = pix.shape[:2]
    return Good(write_png(pix, fmt, **kw), h, w, fmt, pix)


@functools.lru_cache(maxsize=None)
def good():
    m = {}
    # filters: every (h, w) in {1, 2, 3}^2, each filter on every row, all formats
    for fmt in FORMATS:
        for h in (1, 2, 3):
            for w in (1, 2, 3):
                for t in range(5):
                    m[f"f{t}-{fmt}-{h}x{w}"] = _g(_pix(f"f{t}{fmt}{h}{w}", h, w, fmt), fmt, filters=t)
    m["avg-255"] = _g(np.full((3, 4), 255, np.uint8), "gray8", filters=3)          # the 9-bit sum
    # Paeth's ties: a b c chosen so that pa == pb, pb == pc, all equal (second row, second pixel)
    for k, (c, b, a) in enumerate(((10, 20, 20), (10, 30, 10), (7, 7, 7), (0, 255, 255), (100, 50, 150))):
        m[f"paeth-tie-{k}"] = _g(np.array([[c, b], [a, 77]], np.uint8), "gray8", filters=4)
    for fmt in FORMATS:
        m[f"paeth-5x7-{fmt}"] = _g(_pix("paeth57" + fmt, 5, 7, fmt), fmt, filters=4)
        m[f"rows-012344321-{fmt}"] = _g(_smooth(9, 11, fmt), fmt, filters=(0, 1, 2, 3, 4, 4, 3, 2, 1))
    R = UNFILTER_ROWS
    for h in (R - 1, R, R + 1, 2 * R + 1):
        m[f"pass-h{h}"] = _g(_pix(f"pass{h}", h, 3, "gray16"), "gray16", filters=(4, 3, 1, 2, 0))
    # block types
    big = _smooth(130, 260, "gray16")
    m["stored-two-blocks"] = _g(big, "gray16", filters=0, level=0)
    assert len(raw_stream(big, "gray16", 0)) == 67730
    m["stored-small"] = _g(_pix("stored-small", 3, 5, "gray16"), "gray16", filters=(0, 1, 4), level=0)
    m["fixed-small"] = _g(_smooth(5, 6, "gray8"), "gray8", filters=(3, 4), strategy=zlib.Z_FIXED)
    m["fixed"] = _g(_smooth(30, 40, "gray16"), "gray16", filters="adaptive", strategy=zlib.Z_FIXED)
    m["dynamic-9"] = _g(_smooth(60, 80, "gray16"), "gray16", filters="adaptive", level=9)
    m["sync-flush"] = _g(_smooth(60, 80, "gray8"), "gray8", filters=1, level=9, flush_at=(1000, 1001, 3001))
    # skewed random bytes at level 9: a dynamic block that is all literals (zlib itself still sends two
    # one-bit distance codes; the block with no distance code at all is hand-assembled below)
    m["random-literals"] = _g((_rng("literals").integers(0, 8, (20, 31)) ** 2 * 5).astype(np.uint8), "gray8", filters=0,
                              level=9)
    m["wbits-9"] = _g(_smooth(40, 50, "gray16"), "gray16", filters="adaptive", wbits=9)
    # hand-assembled blocks
    m["hand-every-code"] = _every_code()
    toks = [("lit", 0), ("lit", 9), ("match", 3, 1), ("lit", 200), ("match", 258, 1), ("lit", 1)]
    m["hand-dist1-runs"] = _hand(toks, 1, len(expand(toks)) - 1)
    m["hand-lens-1-15"] = _lens_1_to_15()
    m["hand-one-dist-code"] = _one_dist_code()
    m["hand-repeat-codes"] = _repeat_codes()
    ll = [0] * 257
    ll[0] = 1
    ll[7], ll[256] = 2, 2
    toks = [("lit", 0), ("lit", 7), ("lit", 7), ("lit", 0), ("lit", 7)]
    m["hand-no-dist-code"] = _hand(toks, 1, 4, ll_lens=ll, dd_lens=[0])
    # container
    small = _smooth(12, 13, "gray16")
    z = deflate(raw_stream(small, "gray16", "adaptive"))
    m["idat-1-byte"] = Good(wrap(z, 12, 13, "gray16", 1), 12, 13, "gray16", small)
    m["idat-empty-middle"] = Good(wrap(z, 12, 13, "gray16", (20, 20, 40)), 12, 13, "gray16", small)
    m["idat-cut-header-adler"] = Good(wrap(z, 12, 13, "gray16", (1, len(z) - 2)), 12, 13, "gray16", small)
    m["ancillary"] = Good(wrap(z, 12, 13, "gray16", 30, before=chunk(b"tEXt", b"Comment\0depth") + chunk(b"pHYs", bytes(9)),
                               after=chunk(b"tIME", bytes(7))), 12, 13, "gray16", small)
    rgb = _smooth(12, 13, "rgb8")
    m["plte-in-rgb"] = Good(wrap(deflate(raw_stream(rgb, "rgb8", 4)), 12, 13, "rgb8", before=chunk(b"PLTE", bytes(6))),
                            12, 13, "rgb8", rgb)
    for name in GOLDEN:
        fmt = name.split("-")[1]
        with open(os.path.join(GOLDEN_DIR, name + ".png"), "rb") as f:
            m[name] = Good(f.read(), 40, 50, fmt, _smooth(40, 50, fmt, seed=2))
    return m


SWEEP = ("hand-repeat-codes", "fixed-small", "stored-small")     # a dynamic, a fixed and a stored stream


def zstream(data):
    return b"".join(data[a:b] for a, b in _idat_spans(data))


def first_btype(data):
    return (zstream(data)[2] >> 1) & 3


@functools.lru_cache(maxsize=None)
def real_frames():
    """(files, frames): n = 4 frames 424 x 512 gray16, adaptive filters, level 6, 8192-byte IDATs"""
    from oracle import crop_ref as CR
    frames = np.stack([CR.synth_frame(s).astype(np.uint16) for s in range(4)])
    files = [write_png(f, "gray16", filters="adaptive", cuts=8192) for f in frames]
    frames.setflags(write=False)
    return files, frames


def _zbad(z, h=1, w=3, status=ST_STREAM, refuses=True):
    if refuses:
        try:
            zlib.decompress(z)
        except zlib.error:
            pass
        else:
            raise AssertionError("zlib accepts a stream the corpus lists as refused")
    return Bad(wrap(z, h, w, "gray8"), h, w, "gray8", status, refuses)


def _set_crcs(data):
    """the file with every chunk's CRC recomputed"""
    out, p = bytearray(data[:8]), 8
    while p < len(data):
        (n,) = struct.unpack(">I", data[p:p + 4])
        out += chunk(data[p + 4:p + 8], data[p + 8:p + 8 + n])
        p += 12 + n
    return bytes(out)


@functools.lru_cache(maxsize=None)
def bad():
    m = {}
    pix = _smooth(6, 7, "gray16")
    raw = raw_stream(pix, "gray16", (1, 2, 4))
    z = deflate(raw)
    ok = wrap(z, 6, 7, "gray16", 20, before=chunk(b"tEXt", b"k\0v"))
    B = lambda data, st, zr=None, h=6, w=7, fmt="gray16": Bad(data, h, w, fmt, st, zr)
    # container
    edges, p = [8], 8
    while p < len(ok):
        p += 12 + struct.unpack(">I", ok[p:p + 4])[0]
        edges.append(p)
    for k, e in enumerate(edges[:-1]):
        m[f"cut-at-chunk-{k}"] = B(ok[:e], ST_CONTAINER)
        m[f"cut-in-chunk-{k}"] = B(ok[:e + 5], ST_CONTAINER)
    m["cut-in-signature"] = B(ok[:5], ST_CONTAINER)
    m["size-0"] = B(b"", ST_CONTAINER)
    m["bad-signature"] = B(b"\x89PNG\r\n\x1a\r" + ok[8:], ST_CONTAINER)
    m["after-iend"] = B(ok + b"\0", ST_CONTAINER)
    m["no-idat"] = B(SIGNATURE + ihdr(6, 7, "gray16") + chunk(b"IEND"), ST_CONTAINER)
    m["idat-split-by-chunk"] = B(SIGNATURE + ihdr(6, 7, "gray16") + chunk(b"IDAT", z[:9]) + chunk(b"tEXt", b"k\0v") +
                                 chunk(b"IDAT", z[9:]) + chunk(b"IEND"), ST_CONTAINER)
    m["unknown-critical"] = B(wrap(z, 6, 7, "gray16", before=chunk(b"ABCD", b"x")), ST_CONTAINER)
    m["ihdr-12-bytes"] = B(SIGNATURE + chunk(b"IHDR", bytes(12)) + cut(z, ()) + chunk(b"IEND"), ST_CONTAINER)
    m["length-past-file"] = B(ok[:8 + 25] + struct.pack(">I", 1 << 20) + ok[8 + 25 + 4:], ST_CONTAINER)
    # CRC
    flip = bytearray(ok)
    flip[8 + 8 + 13 + 1] ^= 1                    # a byte of the IHDR's CRC
    m["crc-flipped"] = B(bytes(flip), ST_CRC)
    flip = bytearray(ok)
    flip[-5 - 12] ^= 0x40                        # a data byte of the last IDAT, its CRC left alone
    m["data-flipped-crc-kept"] = B(bytes(flip), ST_CRC)
    # unsupported
    m["interlace-1"] = B(SIGNATURE + ihdr(6, 7, "gray16", interlace=1) + cut(z, ()) + chunk(b"IEND"), ST_UNSUPPORTED)
    m["palette"] = B(SIGNATURE + ihdr(6, 7, "gray8", ctype=3) + chunk(b"PLTE", bytes(12)) + cut(z, ()) + chunk(b"IEND"),
                     ST_UNSUPPORTED, fmt="gray8")
    m["gray-alpha"] = B(SIGNATURE + ihdr(6, 7, "gray8", ctype=4) + cut(z, ()) + chunk(b"IEND"), ST_UNSUPPORTED, fmt="gray8")
    m["depth-4"] = B(SIGNATURE + ihdr(6, 7, "gray8", depth=4) + cut(z, ()) + chunk(b"IEND"), ST_UNSUPPORTED, fmt="gray8")
    m["rgb-16"] = B(SIGNATURE + ihdr(6, 7, "rgb8", depth=16) + cut(z, ()) + chunk(b"IEND"), ST_UNSUPPORTED, fmt="rgb8")
    m["compression-1"] = B(SIGNATURE + ihdr(6, 7, "gray16", comp=1) + cut(z, ()) + chunk(b"IEND"), ST_UNSUPPORTED)
    m["filter-method-1"] = B(SIGNATURE + ihdr(6, 7, "gray16", filt=1) + cut(z, ()) + chunk(b"IEND"), ST_UNSUPPORTED)
    # not the call's
    m["wrong-h"] = B(ok, ST_MISMATCH, h=7)
    m["wrong-w"] = B(ok, ST_MISMATCH, w=6)
    m["wrong-format"] = B(ok, ST_MISMATCH, fmt="gray8")
    # the stream
    flip = bytearray(ok)
    flip[-5 - 12 - 8] ^= 0x10                    # a byte of the deflate data in the last IDAT
    fixed = _set_crcs(bytes(flip))
    zf = b"".join(fixed[a:b] for a, b in _idat_spans(fixed))
    try:
        zlib.decompress(zf)
        raise AssertionError("zlib accepts the flipped stream")
    except zlib.error:
        pass
    m["data-flipped-crc-repaired"] = B(fixed, None, True)        # a stream or an Adler error
    flip = bytearray(z)
    flip[-1] ^= 1
    m["adler-flipped"] = B(wrap(bytes(flip), 6, 7, "gray16"), ST_ADLER, True)
    for name, head in (("cm-7", b"\x77\x09"), ("cinfo-8", b"\x88\x1c"), ("fcheck", b"\x78\x02"), ("fdict", b"\x78\x20")):
        m["zlib-" + name] = B(wrap(head + z[2:], 6, 7, "gray16"), ST_STREAM, True)
    r4 = b"\0abc"
    bw = BitWriter()
    bw.bits(1, 1), bw.bits(3, 2)
    m["btype-3"] = _zbad(zwrap(bw.bytes(), r4))
    m["len-nlen"] = _zbad(zwrap(b"\x01\x04\x00\xfb\xfe" + r4, r4))
    bw = BitWriter()
    ll = [0] * 257
    ll[0] = ll[1] = ll[256] = 1                  # three codes of one bit
    dynamic_header(bw, ll, [1])
    m["over-subscribed"] = _zbad(zwrap(bw.bytes() + bytes(4), r4))
    bw = BitWriter()
    ll = [0] * 257
    ll[0] = ll[256] = 2                          # half of the code space is unused and the longest code is 2 bits
    dynamic_header(bw, ll, [1])
    m["incomplete-set"] = _zbad(zwrap(bw.bytes() + bytes(4), r4))
    bw = BitWriter()
    bw.bits(1, 1), bw.bits(1, 2)
    put_tokens(bw, [("lit", 0), ("lit", 7), ("match", 3, 3), ("eob",)], FIXED_LL, FIXED_DD)
    m["distance-too-far"] = _zbad(zwrap(bw.bytes(), b"\0\7\7\7\7"), w=4)
    for name, sym in (("symbol-286", 286), ("symbol-287", 287)):
        bw = BitWriter()
        bw.bits(1, 1), bw.bits(1, 2)
        bw.code(*FIXED_LL[0]), bw.code(*FIXED_LL[sym]), bw.code(*FIXED_LL[256])
        m[name] = _zbad(zwrap(bw.bytes(), r4))
    for name, ds in (("distance-code-30", 30), ("distance-code-31", 31)):
        bw = BitWriter()
        bw.bits(1, 1), bw.bits(1, 2)
        bw.code(*FIXED_LL[0]), bw.code(*FIXED_LL[257]), bw.code(*FIXED_DD[ds]), bw.code(*FIXED_LL[256])
        m[name] = _zbad(zwrap(bw.bytes(), r4))
    m["no-bfinal"] = _zbad(zwrap(b"\x00\x04\x00\xfb\xff" + r4, r4)[:-4] + b"")      # one block, BFINAL 0, then the end
    m["ends-in-block"] = _zbad(z[: len(z) // 2], 6, 14)
    m["tail-5-bytes"] = _zbad(z + b"\0", 6, 14, refuses=None)      # zlib.decompress lets trailing bytes pass
    m["tail-3-bytes"] = _zbad(z[:-1], 6, 14)
    short, long_ = raw[:-15], raw + b"\0"
    m["one-row-short"] = Bad(wrap(deflate(short), 6, 7, "gray16"), 6, 7, "gray16", ST_STREAM, None)
    m["one-byte-long"] = Bad(wrap(deflate(long_), 6, 7, "gray16"), 6, 7, "gray16", ST_STREAM, None)
    # the filter byte
    bad_f = bytearray(raw)
    bad_f[3 * 15] = 5
    m["filter-5"] = B(wrap(deflate(bytes(bad_f)), 6, 7, "gray16"), ST_FILTER)
    return m


def _idat_spans(data):
    p = 8
    while p < len(data):
        (n,) = struct.unpack(">I", data[p:p + 4])
        if data[p + 4:p + 8] == b"IDAT":
            yield p + 8, p + 8 + n
        p += 12 + n


FMT_ID = {"gray16": 0, "gray8": 1, "rgb8": 2}
DTYPE = {"gray16": np.uint16, "gray8": np.uint8, "rgb8": np.uint8}


def groups(cases):
    """the cases grouped by (h, w, fmt): one decode call each -> [((h, w, fmt), [names])]"""
    g = collections.OrderedDict()
    for name, c in cases.items():
        g.setdefault((c.h, c.w, c.fmt), []).append(name)
    return list(g.items())


@functools.lru_cache(maxsize=None)
def host_decoded(which):
    """name -> (frame, status) of every case of good() / bad() through mp_png_decode_host, computed
    once: the device's reference"""
    cases = good() if which == "good" else bad()
    out = {}
    for (h, w, fmt), names in groups(cases):
        buf, sizes = P().pack_files([cases[n].data for n in names])
        frames, status = P().decode_png(buf, sizes, h, w, format=fmt, check=False)
        for i, n in enumerate(names):
            out[n] = (frames[i].copy(), int(status[i]))
    return out


# ------------------------------------------------------------------------------------------ streams
class PngDecodeCase(SO.Case):
    """decode_png on the caller's stream into frames the case owns (kept as bytes, so that the harness
    can poison them); its input sets are two different valid files of one shape"""
    name = "png_decode"
    covers = ("mp_png_decode_dev",)
    outputs = ("frames", "status")
    may_coincide = ("status",)
    SHAPE = (2, 40, 50)
    STRIDE = 4096

    def make(self, seed):
        rng = np.random.default_rng(920 + seed)
        n, h, w = self.SHAPE
        pix = (rng.integers(0, 6, self.SHAPE) * 9000).astype(np.uint16)
        pix[:, 10:20] = pix[:, 9:10]
        buf = np.zeros((n, self.STRIDE), np.uint8)
        sizes = np.zeros(n, np.int64)
        for i in range(n):
            f = write_png(pix[i], "gray16", filters="adaptive", cuts=700)
            buf[i, :len(f)] = np.frombuffer(f, np.uint8)
            sizes[i] = len(f)
        return {"buf": buf, "sizes": sizes}

    def alloc(self):
        import torch
        n, h, w = self.SHAPE
        self.out = {"frames": torch.zeros((n, h, 2 * w), dtype=torch.uint8, device="cuda")}

    def invoke(self):
        import torch
        _, status = P().decode_png(self.inp["buf"], self.inp["sizes"], *self.SHAPE[1:], format="gray16",
                                   out=self.out["frames"].view(torch.uint16), check=False)
        return {"frames": self.out["frames"], "status": status}

    def check_plain(self, A, got):
        ref = P().decode_png(A["buf"], A["sizes"], *self.SHAPE[1:], format="gray16")
        assert not got["status"].any()
        assert np.array_equal(got["frames"].view(np.uint16), ref)


PNGDEC_STREAM_CASES = (PngDecodeCase,)
PNGDEC_ORDERED = {}
for _c in PNGDEC_STREAM_CASES:
    for _fn in _c.covers:
        PNGDEC_ORDERED.setdefault(_fn, []).append(_c.name)
