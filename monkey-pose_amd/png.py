"""PNG files from RGB pictures (include/monkeypose_png.h): the last step of the picture path.

``render_overlays`` leaves uint8 RGB on the device; ``encode_png`` turns it into finished PNG files
there (``mp_png_encode_dev``, two kernels on the caller's stream), so that only the compressed bytes
cross to the host.  The format is fixed to the byte by csrc/png_rule.hpp -- bands of whole rows, one
fixed-Huffman or stored deflate block a band, matches at six fixed distances -- and a numpy input goes
through the same rule on the host (``mp_png_encode_host``), which is what the kernels are compared with.
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

_BUFFERS = {}      # (n, h, w, device) -> (buf, sizes, work): reused by the next call of the same shape


def _lib_png():
    lib = _lib.load()
    if not getattr(lib, "_png_bound", False):
        for name, (res, args) in _PNG_SIGS.items():
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
    host wait; the pair is CUDA tensors, reused by the next call of the same shape on that device
    unless ``out = (buf, sizes)`` is given (contiguous CUDA tensors, ``buf`` [n, >= bound] uint8).  A
    numpy array is encoded on the host by the same rule and the pair is numpy arrays.  ``png_files``
    turns either pair into ``bytes``."""
    import torch
    lib = _lib_png()
    if isinstance(rgb, np.ndarray):
        if rgb.dtype != np.uint8:
            raise TypeError(f"rgb must be uint8, got {rgb.dtype}")
        n, h, w = _shape(rgb.shape)
        if out is not None:
            raise ValueError("out= is for CUDA input")
        a = np.ascontiguousarray(rgb)
        bound = int(lib.mp_png_bound(h, w))
        buf, sizes = np.zeros((n, bound), np.uint8), np.zeros(n, np.int64)
        _lib.check(lib.mp_png_encode_host(a.ctypes.data_as(ctypes.c_void_p), n, h, w,
                                          buf.ctypes.data_as(ctypes.c_void_p), bound,
                                          sizes.ctypes.data_as(ctypes.c_void_p)))
        return buf, sizes
    if not isinstance(rgb, torch.Tensor):
        raise TypeError("rgb must be a CUDA (ROCm) uint8 tensor or a numpy uint8 array")
    if rgb.dtype != torch.uint8:
        raise TypeError(f"rgb must be uint8, got {rgb.dtype}")
    n, h, w = _shape(rgb.shape)
    if not rgb.is_cuda:
        raise TypeError("rgb must be a CUDA (ROCm) tensor (a host picture: pass a numpy array)")
    dev = rgb.device
    bound = int(lib.mp_png_bound(h, w))
    key = (n, h, w, dev)
    held = _BUFFERS.get(key)
    if held is None:
        _BUFFERS.clear()            # one shape's buffers at a time, as the pipelines keep theirs
        held = _BUFFERS[key] = (torch.empty((n, bound), dtype=torch.uint8, device=dev),
                                torch.empty(n, dtype=torch.int64, device=dev),
                                torch.empty(int(lib.mp_png_work_bytes(n, h, w)), dtype=torch.uint8, device=dev))
    buf, sizes, work = held
    if out is not None:
        buf, sizes = out
        if not (isinstance(buf, torch.Tensor) and buf.is_cuda and buf.dtype == torch.uint8 and buf.dim() == 2
                and buf.shape[0] == n and buf.shape[1] >= bound and buf.stride(1) == 1 and buf.device == dev):
            raise ValueError(f"out[0] must be a CUDA uint8 tensor [{n}, >= {bound}] with unit column stride")
        if not (isinstance(sizes, torch.Tensor) and sizes.is_cuda and sizes.dtype == torch.int64
                and tuple(sizes.shape) == (n,) and sizes.is_contiguous() and sizes.device == dev):
            raise ValueError(f"out[1] must be a contiguous CUDA int64 tensor [{n}]")
    src = rgb.detach().contiguous()
    stp = _lib.current_stream(dev) if stream is None else stream
    _lib.check(lib.mp_png_encode_dev(ctypes.c_void_p(src.data_ptr()), n, h, w, ctypes.c_void_p(buf.data_ptr()),
                                     int(buf.stride(0)) if n > 1 else max(int(buf.stride(0)), bound),
                                     ctypes.c_void_p(sizes.data_ptr()), ctypes.c_void_p(work.data_ptr()),
                                     ctypes.c_void_p(stp)))
    return buf, sizes


def png_files(buf, sizes):
    """The files of ``encode_png``'s pair as a list of ``bytes``.  For CUDA tensors ``sizes`` is read
    back first (the only host wait), then the first ``max(sizes)`` columns of ``buf`` are copied."""
    if isinstance(buf, np.ndarray):
        return [buf[i, :int(s)].tobytes() for i, s in enumerate(sizes)]
    sz = sizes.cpu().numpy()
    host = buf[:, :int(sz.max())].cpu().numpy()
    return [host[i, :int(s)].tobytes() for i, s in enumerate(sz)]
