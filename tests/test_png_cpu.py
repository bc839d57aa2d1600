"""mp_png_encode_host (include/monkeypose_png.h; the rule is csrc/png_rule.hpp) on this machine, no GPU:
every case of tests/png_cases.py decodes to its pixels through a reader built on zlib alone and through
PIL, stays within mp_png_bound, follows the band plan the header states, and a handful of small cases
equal committed files byte for byte.  Also the refusals, and the new header's invariants: it compiles
as C99, the library exports what it declares, png.py's ctypes table is its function list, and its
stream prototypes are the ones tests/test_gpu_png.py orders."""
import ctypes
import hashlib
import io
import json
import os
import re
import subprocess

import numpy as np
import pytest

import png_cases as C
import stream_order_cases as SO
from helpers import pkg

MP_ERR_ARG, MP_ERR_SHAPE = -1, -5


def _files(name):
    buf, sizes = C.host_files(name)
    return [buf[i, :s].tobytes() for i, s in enumerate(sizes)]


@pytest.mark.parametrize("name", C.NAMES)
def test_host_files_decode_to_the_pixels(name):
    pic = C.picture(name)
    n, h, w, _ = pic.shape
    buf, sizes = C.host_files(name)
    assert buf.shape == (n, C.P().png_bound(h, w)) and (sizes <= buf.shape[1]).all() and (sizes > 0).all()
    for i, f in enumerate(_files(name)):
        assert np.array_equal(C.read_png(f, h, w), pic[i])
        assert not buf[i, sizes[i]:].any()                       # nothing written past the file


@pytest.mark.parametrize("name", C.NAMES)
def test_pil_reads_the_same_pixels(name):
    Image = pytest.importorskip("PIL.Image")
    pic = C.picture(name)
    for i, f in enumerate(_files(name)):
        im = Image.open(io.BytesIO(f))
        assert im.mode == "RGB" and im.size == (pic.shape[2], pic.shape[1])
        assert np.array_equal(np.asarray(im), pic[i])


@pytest.mark.parametrize("name", C.NAMES)
def test_bytes_follow_the_band_plan(name):
    pic = C.picture(name)
    n, h, w, _ = pic.shape
    rows = C.P().band_plan(h, w)[0]
    for i, f in enumerate(_files(name)):
        raw = np.concatenate([np.zeros((h, 1), np.uint8), pic[i].reshape(h, 3 * w)], axis=1)
        bands = C.band_data(f, h, w)
        for k, b in enumerate(bands):
            assert b == raw[k * rows:(k + 1) * rows].tobytes(), f"band {k}"


def test_bound_is_reached_and_random_bytes_grow():
    P = C.P()
    # every band stored: the file is exactly the bound
    for name in ("random-33x67", "random-above-143"):
        pic = C.picture(name)
        _, h, w, _ = pic.shape
        assert C.host_files(name)[1][0] == P.png_bound(h, w)
        assert C.host_files(name)[1][0] > h * (1 + 3 * w)
    # the bound by the rule's own count: head, 78 01, per band a chunk and 10 bytes, the rows, the tail
    for h, w in ((1, 1), (33, 67), (424, 512), (4096, 4096), (3, 4096), (4096, 1)):
        rows, nb = P.band_plan(h, w)
        assert P.png_bound(h, w) == 33 + 2 + 28 + nb * 22 + h * (1 + 3 * w)
    # 8-bit literals with no match: fixed is one byte under stored at 33 x 67 -- the tie region
    f = _files("random-below-144")[0]
    assert len(f) <= P.png_bound(33, 67)
    # a constant picture is a few tokens a band
    assert C.host_files("const-zero-40")[1][0] < 200


def test_encode_png_numpy_equals_the_c_call():
    P = C.P()
    lib = P._lib_png()
    pic = C.picture("n3")
    n, h, w, _ = pic.shape
    bound = lib.mp_png_bound(h, w)
    out, sizes = np.zeros((n, bound), np.uint8), np.zeros(n, np.int64)
    assert lib.mp_png_encode_host(pic.ctypes.data, n, h, w, out.ctypes.data, bound, sizes.ctypes.data) == 0
    buf, sz = C.host_files("n3")
    assert np.array_equal(sizes, sz) and np.array_equal(out, buf)
    assert P.png_files(buf, sz) == _files("n3")
    # image i's bytes do not depend on the batch it is in
    for i in range(n):
        b1, s1 = P.encode_png(pic[i:i + 1])
        assert s1[0] == sz[i] and b1[0, :s1[0]].tobytes() == _files("n3")[i]


def test_odd_addresses_and_a_wider_stride():
    lib = C.P()._lib_png()
    pic = C.picture("n3")
    n, h, w, _ = pic.shape
    bound = lib.mp_png_bound(h, w)
    stride = bound + 3
    src = np.zeros(pic.size + 1, np.uint8)
    src[1:] = pic.ravel()
    dst = np.full(n * stride + 2, 0xA5, np.uint8)
    sizes = np.zeros(n, np.int64)
    assert lib.mp_png_encode_host(src.ctypes.data + 1, n, h, w, dst.ctypes.data + 1, stride, sizes.ctypes.data) == 0
    buf, sz = C.host_files("n3")
    assert np.array_equal(sizes, sz)
    assert dst[0] == 0xA5 and dst[-1] == 0xA5
    body = dst[1:-1].reshape(n, stride)
    for i in range(n):
        assert body[i, :sz[i]].tobytes() == buf[i, :sz[i]].tobytes()
        assert (body[i, sz[i]:] == 0xA5).all()


def test_refusals():
    P = C.P()
    lib = P._lib_png()
    pic = np.zeros((1, 4, 4, 3), np.uint8)
    bound = lib.mp_png_bound(4, 4)
    out, sizes = np.full(bound, 0x5A, np.uint8), np.full(1, -7, np.int64)
    p, o, s = pic.ctypes.data, out.ctypes.data, sizes.ctypes.data
    for n, h, w, stride in ((0, 4, 4, bound), (65536, 4, 4, bound), (1, 0, 4, bound), (1, 4, 0, bound),
                            (1, 4097, 4, 1 << 30), (1, 4, 4097, 1 << 30), (1, 4, 4, bound - 1)):
        assert lib.mp_png_encode_host(p, n, h, w, o, stride, s) == MP_ERR_SHAPE, (n, h, w, stride)
        assert lib.mp_png_encode_dev(p, n, h, w, o, stride, s, o, None) == MP_ERR_SHAPE, (n, h, w, stride)
    for args in ((None, 1, 4, 4, o, bound, s), (p, 1, 4, 4, None, bound, s), (p, 1, 4, 4, o, bound, None)):
        assert lib.mp_png_encode_host(*args) == MP_ERR_ARG
        assert lib.mp_png_encode_dev(*args, o, None) == MP_ERR_ARG
    assert lib.mp_png_encode_dev(p, 1, 4, 4, o, bound, s, None, None) == MP_ERR_ARG        # no launch: host pointers
    assert (out == 0x5A).all() and sizes[0] == -7
    assert b"mp_png_encode_dev" in pkg()._lib.load().mp_last_error()
    assert lib.mp_png_bound(0, 4) == 0 and lib.mp_png_bound(4, 4097) == 0 and lib.mp_png_work_bytes(0, 4, 4) == 0
    with pytest.raises(ValueError):
        P.png_bound(4097, 1)
    with pytest.raises(ValueError):
        P.encode_png(np.zeros((1, 4, 4, 4), np.uint8))
    with pytest.raises(TypeError):
        P.encode_png(np.zeros((1, 4, 4, 3), np.float32))
    import torch
    with pytest.raises(TypeError):
        P.encode_png(torch.zeros((1, 4, 4, 3), dtype=torch.uint8))          # a host tensor: no quiet fallback


@pytest.mark.parametrize("name", C.GOLDEN)
def test_golden_files(name):
    with open(os.path.join(C.GOLDEN_DIR, name + ".png"), "rb") as f:
        assert _files(name)[0] == f.read()


def test_host_files_equal_the_recorded_bytes():
    """every case's size and SHA-256 (tests/golden/png/digests.json), and the whole files where they are kept"""
    with open(os.path.join(C.GOLDEN_DIR, "digests.json")) as f:
        table = json.load(f)
    assert sorted(table) == sorted(C.NAMES)
    for name in C.NAMES:
        got = [{"sha256": hashlib.sha256(f).hexdigest(), "size": len(f)} for f in _files(name)]
        assert got == table[name], name
    for name in C.GOLDEN:
        with open(os.path.join(C.GOLDEN_DIR, name + ".png"), "rb") as f:
            assert _files(name) == [f.read()], name


# ------------------------------------------------------------------------------------------ the header
def _declared():
    return SO.exported_functions(C.PNG_HEADER)


def test_header_compiles_as_c99():
    src = '#include "monkeypose_png.h"\nint main(void){ return MP_OK + (int)sizeof(&mp_png_encode_dev) * 0; }\n'
    p = subprocess.run(["gcc", "-x", "c", "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-I",
                        os.path.dirname(C.PNG_HEADER), "-"], input=src, text=True, capture_output=True)
    assert p.returncode == 0, p.stderr


def test_library_exports_what_the_header_declares():
    out = subprocess.run(["nm", "-D", "--defined-only", pkg()._lib.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = set(re.findall(r" T (mp_[a-z0-9_]+)", out))
    assert _declared() and not set(_declared()) - exported


def test_ctypes_table_is_the_function_list():
    assert sorted(C.P()._PNG_SIGS) == _declared()
    assert C.P()._PNG_SIGS["mp_png_encode_dev"][1][-1] is ctypes.c_void_p


def test_stream_prototypes_are_the_ordered_cases():
    assert sorted(SO.stream_prototypes(C.PNG_HEADER)) == sorted(C.PNG_ORDERED) == ["mp_png_encode_dev"]
    assert all(C.PNG_ORDERED.values())
    # and the old header's classification is untouched by the new one
    assert not set(C.PNG_ORDERED) & (set(SO.ORDERED) | set(SO.SYNCHRONOUS) | set(SO.DIAGNOSTIC))
