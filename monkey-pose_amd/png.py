"""PNG files from RGB pictures (include/monkeypose_png.h): the last step of the picture path.

``render_overlays`` leaves uint8 RGB on the device; ``encode_png`` turns it into finished PNG files
there (``mp_png_encode_dev``, two kernels on the caller's stream), so that only the compressed bytes
cross to the host.  The format is fixed to the byte by csrc/png_rule.hpp -- bands of whole rows, one
fixed-Huffman or stored deflate block a band, matches at six fixed distances -- and a numpy input goes
through the same rule on the host (``mp_png_encode_host``), which is what the kernels are compared with.

The other direction is ``decode_png`` (include/monkeypose_pngdec.h, csrc/pngdec_rule.hpp): PNG files
-- the reference's ``depth_*.png`` are 16-bit grayscale -- to pixels, on the device from CUDA tensors
(``mp_png_decode_dev``, three kernels on the caller's stream) and on the host from numpy arrays
(``mp_png_decode_host``, the same rule on one thread, no zlib, no PIL).  ``decode_png_files`` packs,
uploads and decodes a list of files or paths; ``load_depth_map`` is ``loadDepthMap`` of the
reference's importer.

``encode_depth_png`` writes such depth frames (include/monkeypose_png16.h, csrc/png16_rule.hpp): uint16
[n, h, w] to 16-bit grayscale files with per-row filters and a dynamic Huffman code per band, on the
device (``mp_png16_encode_dev``) or on the host by the same rule; ``save_depth_maps`` writes the files.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib

MAX_HW, MAX_N = 4096, 65535

# every function include/monkeypose_png.h declares, with its ctypes signature
_PNG_SIGS = {
    "mp_png_bound": (ctypes.c_size_t, [ctypes.c_int64, ctypes.c_int64]),
    "mp_png_work_bytes": (ctypes.c_size_t, [ctypes.c_int64, ctypes.c_int64, ctypes.c_int64]),
    "mp_png_band_rows": (ctypes.c_int, [ctypes.c_int64]),
    "mp_png_band_count": (ctypes.c_int, [ctypes.c_int64, ctypes.c_int64]),
    "mp_png_encode_host": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64,
                                          ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]),
    "mp_png_encode_dev": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64,
                                         ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p,
                                         ctypes.c_void_p]),
}

# every function include/monkeypose_pngdec.h declares
_PNGDEC_SIGS = {
    "mp_png_decode_work_bytes": (ctypes.c_size_t, [ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_int,
                                                   ctypes.c_int64]),
    "mp_png_decode_host": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64,
                                          ctypes.c_int64, ctypes.c_int64, ctypes.c_int, ctypes.c_void_p,
                                          ctypes.c_void_p]),
    "mp_png_decode_dev": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64,
                                         ctypes.c_int64, ctypes.c_int64, ctypes.c_int, ctypes.c_void_p,
                                         ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
}
# every function include/monkeypose_png16.h declares
_PNG16_SIGS = {
    "mp_png16_bound": (ctypes.c_size_t, [ctypes.c_int64, ctypes.c_int64]),
    "mp_png16_work_bytes": (ctypes.c_size_t, [ctypes.c_int64, ctypes.c_int64, ctypes.c_int64]),
    "mp_png16_band_rows": (ctypes.c_int, [ctypes.c_int64]),
    "mp_png16_band_count": (ctypes.c_int, [ctypes.c_int64, ctypes.c_int64]),
    "mp_png16_encode_host": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64,
                                            ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]),
    "mp_png16_encode_dev": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64,
                                           ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p,
                                           ctypes.c_void_p]),
    "mp_png16_band_stats_host": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64,
                                                ctypes.c_void_p]),
}
STAT_INTS = 9      # MP_PNG16_STAT_INTS: form, five filter counts, matches, distance symbols, tree depth
FORMATS = {"gray16": 0, "gray8": 1, "rgb8": 2}
MAX_FILE_STRIDE = 1 << 30
STATUS_NAMES = {0: "decoded", 1: "container", 2: "CRC", 3: "unsupported", 4: "h, w or format is not the call's",
                5: "deflate / zlib stream", 6: "Adler-32", 7: "filter byte"}
_SIGNATURE = b"\x89PNG\r\n\x1a\n"



def _lib_png():
    lib = _lib.load()
    if not getattr(lib, "_png_bound", False):
        for name, (res, args) in list(_PNG_SIGS.items()) + list(_PNGDEC_SIGS.items()) + list(_PNG16_SIGS.items()):
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
        lib._png_bound = True
    return lib


def _shape(shape):
    if len(shape) != 4 or shape[3] != 3:
        raise ValueError(f"rgb must be [n, h, w, 3], got {tuple(shape)}")
    n, h, w = (int(v) for v in shape[:3])
    if not (1 <= n <= MAX_N and 1 <= h <= MAX_HW and 1 <= w <= MAX_HW):
        raise ValueError(f"rgb must have 1 <= n <= {MAX_N} and 1 <= h, w <= {MAX_HW}, got n = {n}, h = {h}, w = {w}")
    return n, h, w


class _Format:
    """What one encoder differs from the other in: the input's name in messages (and how they call a host
    input), its dtype (numpy's; torch's has the same name), its shape check, and the library's four
    functions ``<prefix>_bound``, ``_work_bytes``, ``_encode_host`` and ``_encode_dev``."""

    def __init__(self, word, host_word, dtype, shape, prefix):
        self.word, self.host_word, self.dtype, self.shape, self.prefix = word, host_word, np.dtype(dtype), shape, prefix
        self.buffers = {}           # (n, h, w, device) -> {stream: (buf, sizes, work)}


def _encode(fmt, x, stream, out):
    """``encode_png`` and ``encode_depth_png``: ``x`` of the format ``fmt`` -> ``(buf, sizes)``"""
    import torch
    lib = _lib_png()
    fn = {k: getattr(lib, f"{fmt.prefix}_{k}") for k in ("bound", "work_bytes", "encode_host", "encode_dev")}
    if isinstance(x, np.ndarray):
        if x.dtype != fmt.dtype:
            raise TypeError(f"{fmt.word} must be {fmt.dtype}, got {x.dtype}")
        n, h, w = fmt.shape(x.shape)
        if out is not None:
            raise ValueError("out= is for CUDA input")
        a = np.ascontiguousarray(x)
        bound = int(fn["bound"](h, w))
        buf, sizes = np.zeros((n, bound), np.uint8), np.zeros(n, np.int64)
        _lib.check(fn["encode_host"](a.ctypes.data_as(ctypes.c_void_p), n, h, w, buf.ctypes.data_as(ctypes.c_void_p),
                                     bound, sizes.ctypes.data_as(ctypes.c_void_p)))
        return buf, sizes
    if not isinstance(x, torch.Tensor):
        raise TypeError(f"{fmt.word} must be a CUDA (ROCm) {fmt.dtype} tensor or a numpy {fmt.dtype} array")
    if x.dtype != getattr(torch, fmt.dtype.name):
        raise TypeError(f"{fmt.word} must be {fmt.dtype}, got {x.dtype}")
    n, h, w = fmt.shape(x.shape)
    if not x.is_cuda:
        raise TypeError(f"{fmt.word} must be a CUDA (ROCm) tensor ({fmt.host_word}: pass a numpy array)")
    dev = x.device
    bound = int(fn["bound"](h, w))
    stp = _lib.current_stream(dev) if stream is None else stream
    key = (n, h, w, dev)
    if key not in fmt.buffers:
        fmt.buffers.clear()         # one shape's buffers at a time, as the pipelines keep theirs
        fmt.buffers[key] = {}
    held = fmt.buffers[key].get(stp)
    if held is None:                # .. and one set per stream: two streams' calls share no scratch
        held = fmt.buffers[key][stp] = (
            torch.empty((n, bound), dtype=torch.uint8, device=dev), torch.empty(n, dtype=torch.int64, device=dev),
            torch.empty(int(fn["work_bytes"](n, h, w)), dtype=torch.uint8, device=dev))
    buf, sizes, work = held
    if out is not None:
        buf, sizes = out
        if not (isinstance(buf, torch.Tensor) and buf.is_cuda and buf.dtype == torch.uint8 and buf.dim() == 2
                and buf.shape[0] == n and buf.shape[1] >= bound and buf.stride(1) == 1 and buf.device == dev):
            raise ValueError(f"out[0] must be a CUDA uint8 tensor [{n}, >= {bound}] with unit column stride")
        if not (isinstance(sizes, torch.Tensor) and sizes.is_cuda and sizes.dtype == torch.int64
                and tuple(sizes.shape) == (n,) and sizes.is_contiguous() and sizes.device == dev):
            raise ValueError(f"out[1] must be a contiguous CUDA int64 tensor [{n}]")
    src = x.detach().contiguous()
    _lib.check(fn["encode_dev"](ctypes.c_void_p(src.data_ptr()), n, h, w, ctypes.c_void_p(buf.data_ptr()),
                                int(buf.stride(0)) if n > 1 else max(int(buf.stride(0)), bound),
                                ctypes.c_void_p(sizes.data_ptr()), ctypes.c_void_p(work.data_ptr()),
                                ctypes.c_void_p(stp)))
    return buf, sizes


_RGB = _Format("rgb", "a host picture", np.uint8, _shape, "mp_png")


def png_bound(h, w):
    """Bytes of the largest file ``encode_png`` writes for an h x w picture (every band stored)."""
    h, w = int(h), int(w)
    if not (1 <= h <= MAX_HW and 1 <= w <= MAX_HW):
        raise ValueError(f"1 <= h, w <= {MAX_HW}, got h = {h}, w = {w}")
    return int(_lib_png().mp_png_bound(h, w))


def band_plan(h, w):
    """(rows of a band, number of bands) of an h x w picture: the plan the files' IDAT chunks follow."""
    png_bound(h, w)
    lib = _lib_png()
    return int(lib.mp_png_band_rows(int(w))), int(lib.mp_png_band_count(int(h), int(w)))


def encode_png(rgb, stream=None, out=None):
    """PNG files of the pictures ``rgb`` [n, h, w, 3] uint8 -> ``(buf [n, bound] uint8, sizes [n] int64)``:
    picture i's file is ``buf[i, :sizes[i]]`` and ``bound = png_bound(h, w)``.

    A CUDA (ROCm) tensor is encoded on the device, on ``stream`` (default: the current one), without a
    host wait; the pair is CUDA tensors, reused by the next call of the same shape on that device and
    stream unless ``out = (buf, sizes)`` is given (contiguous CUDA tensors, ``buf`` [n, >= bound] uint8).  A
    numpy array is encoded on the host by the same rule and the pair is numpy arrays.  ``png_files``
    turns either pair into ``bytes``."""
    return _encode(_RGB, rgb, stream, out)


def png_files(buf, sizes):
    """The files of ``encode_png``'s pair as a list of ``bytes``.  For CUDA tensors ``sizes`` is read
    back first (the only host wait), then the first ``max(sizes)`` columns of ``buf`` are copied."""
    if isinstance(buf, np.ndarray):
        return [buf[i, :int(s)].tobytes() for i, s in enumerate(sizes)]
    sz = sizes.cpu().numpy()
    host = buf[:, :int(sz.max())].cpu().numpy()
    return [host[i, :int(s)].tobytes() for i, s in enumerate(sz)]


# ------------------------------------------------------------------------------------------ depth frames
def _depth_shape(shape):
    if len(shape) != 3:
        raise ValueError(f"frames must be [n, h, w], got {tuple(shape)}")
    n, h, w = (int(v) for v in shape)
    if not (1 <= n <= MAX_N and 1 <= h <= MAX_HW and 1 <= w <= MAX_HW):
        raise ValueError(f"frames must have 1 <= n <= {MAX_N} and 1 <= h, w <= {MAX_HW}, got n = {n}, h = {h}, w = {w}")
    return n, h, w


_DEPTH = _Format("frames", "host frames", np.uint16, _depth_shape, "mp_png16")


def depth_png_bound(h, w):
    """Bytes of the largest file ``encode_depth_png`` writes for an h x w frame (every band stored)."""
    h, w = int(h), int(w)
    if not (1 <= h <= MAX_HW and 1 <= w <= MAX_HW):
        raise ValueError(f"1 <= h, w <= {MAX_HW}, got h = {h}, w = {w}")
    return int(_lib_png().mp_png16_bound(h, w))


def depth_band_plan(h, w):
    """(rows of a band, number of bands) of an h x w depth frame: the plan the files' IDAT chunks follow."""
    depth_png_bound(h, w)
    lib = _lib_png()
    return int(lib.mp_png16_band_rows(int(w))), int(lib.mp_png16_band_count(int(h), int(w)))


def depth_band_stats(frames):
    """What the rule did with each band of the numpy uint16 frames [n, h, w]: int32 [n, bands, 9] --
    the form chosen (0 stored, 1 fixed, 2 dynamic), the rows that took each of the five filters, the
    matches, the distinct distance symbols and the depth of the Huffman tree before the 15-bit limit
    (``mp_png16_band_stats_host``)."""
    if not isinstance(frames, np.ndarray) or frames.dtype != np.uint16:
        raise TypeError("frames must be a numpy uint16 array")
    n, h, w = _depth_shape(frames.shape)
    lib = _lib_png()
    a = np.ascontiguousarray(frames)
    stats = np.zeros((n, int(lib.mp_png16_band_count(h, w)), STAT_INTS), np.int32)
    _lib.check(lib.mp_png16_band_stats_host(a.ctypes.data_as(ctypes.c_void_p), n, h, w,
                                            stats.ctypes.data_as(ctypes.c_void_p)))
    return stats


def encode_depth_png(frames, stream=None, out=None):
    """16-bit grayscale PNG files of the depth frames ``frames`` [n, h, w] uint16 -> ``(buf [n, bound]
    uint8, sizes [n] int64)``: frame i's file is ``buf[i, :sizes[i]]`` and ``bound = depth_png_bound(h, w)``.
    ``decode_png`` (and PIL, and the importer's ``loadDepthMap``) read them back bit for bit.

    A CUDA (ROCm) ``torch.uint16`` tensor is encoded on the device, on ``stream`` (default: the current
    one), without a host wait; the pair is CUDA tensors, reused by the next call of the same shape on
    that device and stream unless ``out = (buf, sizes)`` is given (contiguous CUDA tensors, ``buf`` [n, >= bound]
    uint8).  A numpy array is encoded on the host by the same rule (csrc/png16_rule.hpp: per-row
    filters, bands of whole rows, a stored, fixed or dynamic Huffman block a band) and the pair is
    numpy arrays.  ``png_files`` turns either pair into ``bytes``."""
    return _encode(_DEPTH, frames, stream, out)


def save_depth_maps(paths, frames):
    """One 16-bit grayscale PNG file per frame: ``frames`` [n, h, w] uint16 (a CUDA tensor is encoded on
    the device, a numpy array on the host) to the n ``paths``.  The inverse of ``load_depth_map`` and
    ``decode_png_files``."""
    paths = list(paths)
    if len(paths) != int(frames.shape[0]):
        raise ValueError(f"{len(paths)} paths for {int(frames.shape[0])} frames")
    for path, data in zip(paths, png_files(*encode_depth_png(frames))):
        with open(path, "wb") as f:
            f.write(data)


# ------------------------------------------------------------------------------------------ decoding
_DEC_BUFFERS = {}  # (n, h, w, format, stride, device) -> (frames, status, work)


def png_info(data):
    """(h, w, format name or None) of a PNG file's IHDR, read on the host from its first 33 bytes;
    the name is None for a kind ``decode_png`` does not take.  ValueError if they are not a
    signature and an IHDR chunk."""
    import struct
    head = bytes(data[:33])
    if len(head) < 33 or head[:8] != _SIGNATURE or head[8:16] != b"\0\0\0\rIHDR":
        raise ValueError("not a PNG file: no signature and IHDR chunk in its first 33 bytes")
    w, h, depth, ctype, comp, filt, lace = struct.unpack(">IIBBBBB", head[16:29])
    name = {(0, 16): "gray16", (0, 8): "gray8", (2, 8): "rgb8"}.get((ctype, depth))
    return h, w, (name if (comp, filt, lace) == (0, 0, 0) else None)


def pack_files(files, pinned=False):
    """A list of ``bytes`` -> ``(buf [n, stride] uint8, sizes [n] int64)``, file i in ``buf[i, :sizes[i]]``
    and ``stride`` the longest file rounded up to 16: numpy arrays, or with ``pinned=True`` host
    tensors in pinned memory (for an asynchronous upload)."""
    files = list(files)
    if not files:
        raise ValueError("pack_files: no files")
    sizes = np.asarray([len(f) for f in files], np.int64)
    stride = max(16, (int(sizes.max()) + 15) // 16 * 16)
    if pinned:
        import torch
        tb = torch.zeros((len(files), stride), dtype=torch.uint8).pin_memory()
        buf = tb.numpy()
    else:
        buf = np.zeros((len(files), stride), np.uint8)
    for i, f in enumerate(files):
        buf[i, :len(f)] = np.frombuffer(f, np.uint8)
    if pinned:
        import torch
        return tb, torch.from_numpy(sizes).pin_memory()
    return buf, sizes


def _dec_shape(n, h, w, stride, fmt):
    if fmt not in FORMATS:
        raise ValueError(f"format must be one of {sorted(FORMATS)}, got {fmt!r}")
    n, h, w, stride = int(n), int(h), int(w), int(stride)
    if not (1 <= n <= MAX_N and 1 <= h <= MAX_HW and 1 <= w <= MAX_HW and 1 <= stride <= MAX_FILE_STRIDE):
        raise ValueError(f"1 <= n <= {MAX_N}, 1 <= h, w <= {MAX_HW} and 1 <= stride <= 2^30, got n = {n}, h = {h}, "
                         f"w = {w}, stride = {stride}")
    return n, h, w, stride, ((h, w, 3) if fmt == "rgb8" else (h, w))


def _raise_status(status):
    bad = np.flatnonzero(status)
    if bad.size:
        i = int(bad[0])
        raise ValueError(f"file {i} does not decode: status {int(status[i])} ({STATUS_NAMES[int(status[i])]})"
                         + (f"; {bad.size - 1} more fail" if bad.size > 1 else ""))


def decode_png(buf, sizes, h, w, format="gray16", stream=None, out=None, check=True):
    """The pixels of the PNG files ``buf`` [n, stride] uint8 (file i is ``buf[i, :sizes[i]]``, ``sizes``
    [n] int64; ``pack_files`` makes the pair), all ``h`` x ``w`` and of one ``format``: 'gray16' ->
    uint16 [n, h, w], 'gray8' -> uint8 [n, h, w], 'rgb8' -> uint8 [n, h, w, 3].

    CUDA (ROCm) tensors are decoded on the device, on ``stream`` (default: the current one); the
    frames are a CUDA tensor, reused by the next call of the same shape on that device unless ``out``
    (a contiguous CUDA tensor of that shape and dtype) is given.  numpy arrays are decoded on the
    host by the same rule.  There is no quiet fallback from one to the other.

    ``check=True`` reads the per-file statuses back (the only host wait) and raises ``ValueError``
    naming the first file that did not decode; ``check=False`` returns ``(frames, status)``, ``status``
    int32 [n] (0 = decoded, else include/monkeypose_pngdec.h's code; that file's frame is zeros),
    without waiting."""
    import torch
    lib = _lib_png()
    if isinstance(buf, np.ndarray):
        if buf.dtype != np.uint8 or buf.ndim != 2:
            raise TypeError(f"buf must be uint8 [n, stride], got {buf.dtype} {buf.shape}")
        if out is not None:
            raise ValueError("out= is for CUDA input")
        n, h, w, stride, shape = _dec_shape(buf.shape[0], h, w, buf.shape[1], format)
        b = np.ascontiguousarray(buf)
        sz = np.ascontiguousarray(sizes, np.int64)
        if sz.shape != (n,):
            raise ValueError(f"sizes must be [{n}], got {sz.shape}")
        frames = np.zeros((n,) + shape, np.uint16 if format == "gray16" else np.uint8)
        status = np.zeros(n, np.int32)
        _lib.check(lib.mp_png_decode_host(b.ctypes.data_as(ctypes.c_void_p), stride, sz.ctypes.data_as(ctypes.c_void_p),
                                          n, h, w, FORMATS[format], frames.ctypes.data_as(ctypes.c_void_p),
                                          status.ctypes.data_as(ctypes.c_void_p)))
        if not check:
            return frames, status
        _raise_status(status)
        return frames
    if not (isinstance(buf, torch.Tensor) and isinstance(sizes, torch.Tensor)):
        raise TypeError("buf and sizes must both be CUDA (ROCm) tensors or both numpy arrays")
    if not (buf.is_cuda and sizes.is_cuda):
        raise TypeError("buf and sizes must be CUDA (ROCm) tensors (host files: pass numpy arrays)")
    if buf.dtype != torch.uint8 or buf.dim() != 2 or buf.stride(1) != 1:
        raise TypeError(f"buf must be uint8 [n, stride] with unit column stride, got {buf.dtype} {tuple(buf.shape)}")
    n, h, w, stride, shape = _dec_shape(buf.shape[0], h, w, max(int(buf.stride(0)), int(buf.shape[1])), format)
    dev = buf.device
    if sizes.dtype != torch.int64 or tuple(sizes.shape) != (n,) or not sizes.is_contiguous() or sizes.device != dev:
        raise ValueError(f"sizes must be a contiguous CUDA int64 tensor [{n}] on {dev}")
    dtype = torch.uint16 if format == "gray16" else torch.uint8
    key = (n, h, w, format, stride, dev)
    held = _DEC_BUFFERS.get(key)
    if held is None:
        _DEC_BUFFERS.clear()        # one shape's buffers at a time, as encode_png keeps its
        held = _DEC_BUFFERS[key] = (torch.empty((n,) + shape, dtype=dtype, device=dev),
                                    torch.empty(n, dtype=torch.int32, device=dev),
                                    torch.empty(int(lib.mp_png_decode_work_bytes(n, h, w, FORMATS[format], stride)),
                                                dtype=torch.uint8, device=dev))
    frames, status, work = held
    if out is not None:
        if not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == dtype and out.device == dev
                and tuple(out.shape) == (n,) + shape and out.is_contiguous()):
            raise ValueError(f"out must be a contiguous CUDA {dtype} tensor {(n,) + shape} on {dev}")
        frames = out
    stp = _lib.current_stream(dev) if stream is None else stream
    _lib.check(lib.mp_png_decode_dev(ctypes.c_void_p(buf.data_ptr()), stride, ctypes.c_void_p(sizes.data_ptr()), n, h, w,
                                     FORMATS[format], ctypes.c_void_p(frames.data_ptr()),
                                     ctypes.c_void_p(status.data_ptr()), ctypes.c_void_p(work.data_ptr()),
                                     ctypes.c_void_p(stp)))
    if not check:
        return frames, status
    _raise_status(status.cpu().numpy())
    return frames


def _read_all(files_or_paths):
    out = []
    for f in files_or_paths:
        if isinstance(f, (bytes, bytearray, memoryview)):
            out.append(bytes(f))
        else:
            with open(f, "rb") as fh:
                out.append(fh.read())
    return out


def decode_png_files(files_or_paths, device=None, format=None, stream=None, check=True):
    """PNG files (``bytes``) or their paths -> frames: ``png_info`` of the first file gives h, w and
    (unless given) the format, then the files are packed (``pack_files``), uploaded to ``device`` and
    decoded there (``decode_png``).  ``device=None`` decodes on the host and returns numpy arrays."""
    files = _read_all(files_or_paths)
    if not files:
        raise ValueError("decode_png_files: no files")
    h, w, fmt = png_info(files[0])
    fmt = format or fmt
    if fmt is None:
        raise ValueError("the first file is of a kind decode_png does not take (gray16, gray8, rgb8; not interlaced)")
    buf, sizes = pack_files(files)
    if device is None:
        return decode_png(buf, sizes, h, w, fmt, check=check)
    import torch
    dev = torch.device(device)
    return decode_png(torch.from_numpy(buf).to(dev), torch.from_numpy(sizes).to(dev), h, w, fmt, stream=stream,
                      check=check)


def load_depth_map(filename):
    """``MonkeyRendersImporter.loadDepthMap`` (Importer.py:92-100) without PIL: the depth PNG ``filename``
    -> float32 [h, w], decoded on the host (``mp_png_decode_host``).  8-bit grayscale files are read too."""
    with open(filename, "rb") as f:
        data = f.read()
    h, w, fmt = png_info(data)
    if fmt not in ("gray16", "gray8"):
        raise ValueError(f"{filename}: a depth map is a grayscale PNG, 16 or 8 bits, not interlaced")
    return decode_png(*pack_files([data]), h, w, fmt)[0].astype(np.float32)
