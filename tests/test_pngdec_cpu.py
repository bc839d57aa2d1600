"""mp_png_decode_host (include/monkeypose_pngdec.h; the rule is csrc/pngdec_rule.hpp) on this machine, no
GPU: every good file of tests/pngdec_cases.py decodes to its writer's pixels (and to PIL's reading where
PIL is installed), every refusal gives its status, a zero image and untouched neighbours, entry refusals
touch nothing, and the rule alone -- built as a host program with the address and undefined-behaviour
sanitizers -- runs the whole corpus and a seeded sweep of corruptions and truncations cleanly and with
the library's statuses.  Also the Python layer on numpy input, and the new header's invariants."""
import ctypes
import io
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import png_cases as PC
import pngdec_cases as C
import stream_order_cases as SO
from helpers import ROOT, pkg

MP_ERR_ARG, MP_ERR_SHAPE = -1, -5
GOOD, BAD = tuple(C.good()), tuple(C.bad())


@pytest.mark.parametrize("name", GOOD)
def test_host_decodes_to_the_source_pixels(name):
    c = C.good()[name]
    frame, status = C.host_decoded("good")[name]
    assert status == 0
    assert frame.dtype == C.DTYPE[c.fmt] and frame.shape == c.pixels.shape
    assert np.array_equal(frame, c.pixels)


@pytest.mark.parametrize("name", GOOD)
def test_pil_reads_the_same_pixels(name):
    Image = pytest.importorskip("PIL.Image")
    c = C.good()[name]
    im = Image.open(io.BytesIO(c.data))
    assert im.size == (c.w, c.h)
    assert np.array_equal(np.asarray(im).astype(C.DTYPE[c.fmt]), C.host_decoded("good")[name][0])


def test_the_corpus_holds_every_block_type():
    g = C.good()
    assert C.first_btype(g["stored-two-blocks"].data) == 0 and C.first_btype(g["fixed"].data) == 1
    assert C.first_btype(g["dynamic-9"].data) == 2 and C.first_btype(g["random-literals"].data) == 2
    z = C.zstream(g["sync-flush"].data)
    assert z.count(b"\x00\x00\xff\xff") >= 3                      # the empty stored blocks of Z_SYNC_FLUSH
    assert C.zstream(g["wbits-9"].data)[0] >> 4 == 1              # CINFO 1
    assert [C.first_btype(g[n].data) for n in C.SWEEP] == [2, 1, 0]


def _neighbour(h, w, fmt):
    return C.write_png(C._pix(f"neighbour{h}{w}{fmt}", h, w, fmt), fmt, filters=4), C._pix(f"neighbour{h}{w}{fmt}", h, w, fmt)


@pytest.mark.parametrize("name", BAD)
def test_refusal_status_zero_image_and_neighbours(name):
    c = C.bad()[name]
    frame, status = C.host_decoded("bad")[name]
    assert status == c.status if c.status is not None else status in (C.ST_STREAM, C.ST_ADLER)
    assert not frame.any()
    good, pix = _neighbour(c.h, c.w, c.fmt)
    buf, sizes = C.P().pack_files([good, c.data, good])
    frames, st = C.P().decode_png(buf, sizes, c.h, c.w, format=c.fmt, check=False)
    assert list(st) == [0, status, 0]
    assert np.array_equal(frames[0], pix) and np.array_equal(frames[2], pix) and not frames[1].any()
    with pytest.raises(ValueError, match=f"file 1 .*status {status}"):
        C.P().decode_png(buf, sizes, c.h, c.w, format=c.fmt)


def test_every_status_code_is_reached():
    got = {st for _, st in C.host_decoded("bad").values()}
    assert got == set(range(1, 8))
    assert {c.zlib_refuses for c in C.bad().values()} == {True, None}


def test_a_size_out_of_range_is_an_empty_file():
    good, pix = _neighbour(6, 7, "gray16")
    buf, sizes = C.P().pack_files([good, good, good])
    sizes[0], sizes[1] = -1, buf.shape[1] + 1
    frames, st = C.P().decode_png(buf, sizes, 6, 7, check=False)
    assert list(st) == [1, 1, 0] and not frames[:2].any() and np.array_equal(frames[2], pix)


def _entry_args():
    good, _ = _neighbour(4, 4, "gray16")
    files = np.frombuffer(good, np.uint8).copy()
    sizes = np.asarray([files.size], np.int64)
    out, status = np.full(4 * 4 + 1, 0x5A5A, np.uint16), np.full(1, -7, np.int32)
    return files, sizes, out, status


def test_entry_refusals_touch_nothing():
    lib = C.P()._lib_png()
    files, sizes, out, status = _entry_args()
    f, s, o, t, stride = files.ctypes.data, sizes.ctypes.data, out.ctypes.data, status.ctypes.data, files.size
    for n, h, w, fmt, st in ((0, 4, 4, 0, stride), (65536, 4, 4, 0, stride), (1, 0, 4, 0, stride), (1, 4, 0, 0, stride),
                             (1, 4097, 4, 0, stride), (1, 4, 4097, 0, stride), (1, 4, 4, 3, stride), (1, 4, 4, -1, stride),
                             (1, 4, 4, 0, 0), (1, 4, 4, 0, (1 << 30) + 1)):
        assert lib.mp_png_decode_host(f, st, s, n, h, w, fmt, o, t) == MP_ERR_SHAPE, (n, h, w, fmt, st)
        assert lib.mp_png_decode_dev(f, st, s, n, h, w, fmt, o, t, o, None) == MP_ERR_SHAPE, (n, h, w, fmt, st)
        assert lib.mp_png_decode_work_bytes(n, h, w, fmt, st) == 0
    for args in ((None, stride, s, 1, 4, 4, 0, o, t), (f, stride, None, 1, 4, 4, 0, o, t), (f, stride, s, 1, 4, 4, 0, None, t),
                 (f, stride, s, 1, 4, 4, 0, o, None), (f, stride, s, 1, 4, 4, 0, o + 1, t), (f, stride, s + 4, 1, 4, 4, 0, o, t),
                 (f, stride, s, 1, 4, 4, 0, o, t + 2)):
        assert lib.mp_png_decode_host(*args) == MP_ERR_ARG
        assert lib.mp_png_decode_dev(*args, o, None) == MP_ERR_ARG
    assert lib.mp_png_decode_dev(f, stride, s, 1, 4, 4, 0, o, t, None, None) == MP_ERR_ARG     # no launch: host pointers
    assert lib.mp_png_decode_dev(f, stride, s, 1, 4, 4, 0, o, t, o + 2, None) == MP_ERR_ARG
    assert b"mp_png_decode_dev" in pkg()._lib.load().mp_last_error()
    assert (out == 0x5A5A).all() and status[0] == -7
    assert lib.mp_png_decode_work_bytes(1, 4, 4, 0, stride) >= 16 + stride + 4 * 9
    # an odd out address is fine for the byte formats
    good8, pix8 = _neighbour(4, 4, "gray8")
    b8 = np.frombuffer(good8, np.uint8).copy()
    o8 = np.zeros(17, np.uint8)
    assert lib.mp_png_decode_host(b8.ctypes.data, b8.size, np.asarray([b8.size], np.int64).ctypes.data, 1, 4, 4, 1,
                                  o8.ctypes.data + 1, t) == 0
    assert status[0] == 0 and np.array_equal(o8[1:].reshape(4, 4), pix8) and o8[0] == 0


def test_python_layer_refusals():
    P = C.P()
    import torch
    buf, sizes = P.pack_files([C.good()["fixed-small"].data])
    with pytest.raises(ValueError):
        P.decode_png(buf, sizes, 5, 6, format="gray4")
    with pytest.raises(ValueError):
        P.decode_png(buf, sizes, 4097, 6, format="gray8")
    with pytest.raises(TypeError):
        P.decode_png(buf.astype(np.int8), sizes, 5, 6, format="gray8")
    with pytest.raises(TypeError):
        P.decode_png(torch.from_numpy(buf), torch.from_numpy(sizes), 5, 6, format="gray8")   # host tensors: no quiet fallback
    with pytest.raises(ValueError):
        P.pack_files([])
    with pytest.raises(ValueError):
        P.png_info(b"GIF89a" + bytes(40))


def test_odd_addresses_a_wider_stride_and_guards():
    lib = C.P()._lib_png()
    names = [n for n in GOOD if (C.good()[n].h, C.good()[n].w, C.good()[n].fmt) == (12, 13, "gray16")]
    assert len(names) >= 4
    files = [C.good()[n].data for n in names]
    n, stride, guard = len(files), max(map(len, files)) + 5, 32
    src = np.full(guard + 1 + n * stride + guard, 0xA5, np.uint8)
    for i, f in enumerate(files):
        src[guard + 1 + i * stride:guard + 1 + i * stride + len(f)] = np.frombuffer(f, np.uint8)
    keep = src.copy()
    sizes = np.asarray([len(f) for f in files], np.int64)
    out = np.full(guard + n * 12 * 13 + guard, 0xA5A5, np.uint16)
    status = np.full(n + 2, -7, np.int32)
    assert lib.mp_png_decode_host(src.ctypes.data + guard + 1, stride, sizes.ctypes.data, n, 12, 13, 0,
                                  out.ctypes.data + 2 * guard, status.ctypes.data + 4) == 0
    assert np.array_equal(src, keep)
    assert (out[:guard] == 0xA5A5).all() and (out[-guard:] == 0xA5A5).all()
    assert list(status) == [-7] + [0] * n + [-7]
    for i, name in enumerate(names):
        assert np.array_equal(out[guard + i * 156:guard + (i + 1) * 156].reshape(12, 13), C.good()[name].pixels)


def test_real_shape_frames():
    files, frames = C.real_frames()
    assert all(len(f) < 424 * 512 for f in files)                 # well below the raw 434,176 bytes
    got = C.P().decode_png_files(files)
    assert got.dtype == np.uint16 and np.array_equal(got, frames)
    assert C.P().png_info(files[0]) == (424, 512, "gray16")


def test_load_depth_map(tmp_path):
    files, frames = C.real_frames()
    p = tmp_path / "depth_000000.png"
    p.write_bytes(files[1])
    dm = C.P().load_depth_map(str(p))
    assert dm.dtype == np.float32 and np.array_equal(dm, frames[1].astype(np.float32))
    p8 = tmp_path / "gray8.png"
    p8.write_bytes(C.good()["fixed-small"].data)
    assert np.array_equal(C.P().load_depth_map(str(p8)), C.good()["fixed-small"].pixels.astype(np.float32))
    prgb = tmp_path / "rgb.png"
    prgb.write_bytes(C.good()["plte-in-rgb"].data)
    with pytest.raises(ValueError):
        C.P().load_depth_map(str(prgb))


def test_load_depth_map_equals_pil(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    for name in ("pil-gray16-40x50", "dynamic-9"):
        p = tmp_path / (name + ".png")
        p.write_bytes(C.good()[name].data)
        assert np.array_equal(C.P().load_depth_map(str(p)), np.asarray(Image.open(str(p)), np.float32))   # Importer.py:92-100


@pytest.mark.parametrize("name", ("n3",) + PC.BAND_CASES + ("overlay-jet",))
def test_decode_of_encode_is_the_picture(name):
    pic = PC.picture(name)
    buf, sizes = PC.host_files(name)
    got = C.P().decode_png(buf, sizes, pic.shape[1], pic.shape[2], format="rgb8")
    assert got.dtype == np.uint8 and np.array_equal(got, pic)


# ------------------------------------------------------------------------------------------ the rule alone
@pytest.fixture(scope="module")
def rule_program(tmp_path_factory):
    """tests/pngdec_rule_main.cpp with the address and undefined-behaviour sanitizers: a host program"""
    if not shutil.which("g++"):
        pytest.fail("g++ is needed to build the rule's host program")
    exe = str(tmp_path_factory.mktemp("rule") / "pngdec_rule_main")
    p = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "pngdec_rule_main.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    return exe


def _fnv(a):
    h = 1469598103934665603
    for x in np.ascontiguousarray(a).tobytes():
        h = ((h ^ x) * 1099511628211) & (2 ** 64 - 1)
    return h


def _run_rule(exe, tmp, items):
    """items [(data, h, w, fmt)] -> [(status, hash)] from the sanitizer-built program, one run"""
    lines = []
    for k, (data, h, w, fmt) in enumerate(items):
        path = os.path.join(tmp, f"{k}.png")
        with open(path, "wb") as f:
            f.write(data)
        lines.append(f"{path} {h} {w} {C.FMT_ID[fmt]}")
    man = os.path.join(tmp, "manifest.txt")
    with open(man, "w") as f:
        f.write("\n".join(lines) + "\n")
    p = subprocess.run([exe, man], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and not p.stderr, p.stderr[-4000:]          # a sanitizer report ends the program
    rows = [r.split() for r in p.stdout.splitlines()]
    assert len(rows) == len(items)
    return [(int(s), int(h, 16)) for s, h in rows]


def _library(items):
    """the same items through mp_png_decode_host, one call a shape -> [(status, hash)]"""
    out = [None] * len(items)
    by = {}
    for k, (data, h, w, fmt) in enumerate(items):
        by.setdefault((h, w, fmt), []).append(k)
    for (h, w, fmt), ks in by.items():
        buf, sizes = C.P().pack_files([items[k][0] for k in ks])
        frames, status = C.P().decode_png(buf, sizes, h, w, format=fmt, check=False)
        for i, k in enumerate(ks):
            out[k] = (int(status[i]), _fnv(frames[i]))
    return out


def test_sanitized_rule_runs_the_whole_corpus(rule_program, tmp_path):
    cases = list(C.good().values()) + list(C.bad().values())
    items = [(c.data, c.h, c.w, c.fmt) for c in cases]
    got = _run_rule(rule_program, str(tmp_path), items)
    assert got == _library(items)
    for c, (st, hsh) in zip(C.good().values(), got):
        assert st == 0 and hsh == _fnv(c.pixels)


def test_sanitized_rule_survives_a_corruption_sweep(rule_program, tmp_path):
    """single-byte and single-bit corruptions and truncations of three small files (a dynamic, a fixed
    and a stored stream): of the file as it is (most end at the container or the CRC), and of its zlib
    stream with the file rebuilt around it (they reach the decoder proper)"""
    rng = np.random.default_rng(20240521)
    items = []
    for name in C.SWEEP:
        c = C.good()[name]
        z = C.zstream(c.data)
        for data, rebuild in ((c.data, lambda b: b), (z, lambda b, c=c: C.wrap(b, c.h, c.w, c.fmt))):
            for cutlen in range(len(data)):
                items.append((rebuild(data[:cutlen]), c.h, c.w, c.fmt))
            for pos in range(len(data)):
                b = bytearray(data)
                b[pos] = (b[pos] + int(rng.integers(1, 256))) & 255
                items.append((rebuild(bytes(b)), c.h, c.w, c.fmt))
                b = bytearray(data)
                b[pos] ^= 1 << int(rng.integers(0, 8))
                items.append((rebuild(bytes(b)), c.h, c.w, c.fmt))
    assert len(items) > 1000
    got = _run_rule(rule_program, str(tmp_path), items)          # terminates, no sanitizer report
    assert got == _library(items)
    statuses = {s for s, _ in got}
    assert {1, 2, 5, 6} <= statuses                              # the sweep reaches the container, the CRC and the stream
    zeros = {(c.h, c.w, c.fmt): _fnv(np.zeros(c.pixels.nbytes, np.uint8)) for c in map(C.good().get, C.SWEEP)}
    assert all(s == 0 or h == zeros[it[1:]] for (s, h), it in zip(got, items))     # a failed file's image is zeros


# ------------------------------------------------------------------------------------------ the header
def _declared():
    return SO.exported_functions(C.PNGDEC_HEADER)


def test_header_compiles_as_c99():
    src = ('#include "monkeypose_pngdec.h"\nint main(void){ return MP_OK + MP_PNG_GRAY16 + '
           '(int)sizeof(&mp_png_decode_dev) * 0; }\n')
    p = subprocess.run(["gcc", "-x", "c", "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-I",
                        os.path.dirname(C.PNGDEC_HEADER), "-"], input=src, text=True, capture_output=True)
    assert p.returncode == 0, p.stderr


def test_library_exports_what_the_header_declares():
    out = subprocess.run(["nm", "-D", "--defined-only", pkg()._lib.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = set(re.findall(r" T (mp_[a-z0-9_]+)", out))
    assert _declared() == ["mp_png_decode_dev", "mp_png_decode_host", "mp_png_decode_work_bytes"]
    assert not set(_declared()) - exported


def test_ctypes_tables_are_the_function_lists():
    P = C.P()
    assert sorted(P._PNGDEC_SIGS) == _declared()
    assert P._PNGDEC_SIGS["mp_png_decode_dev"][1][-1] is ctypes.c_void_p
    assert sorted(P._PNG_SIGS) == SO.exported_functions(PC.PNG_HEADER)           # the encoder's table is unchanged
    assert P.FORMATS == {"gray16": 0, "gray8": 1, "rgb8": 2} == C.FMT_ID


def test_stream_prototypes_are_the_ordered_cases():
    assert sorted(SO.stream_prototypes(C.PNGDEC_HEADER)) == sorted(C.PNGDEC_ORDERED) == ["mp_png_decode_dev"]
    assert all(C.PNGDEC_ORDERED.values())
    assert not set(C.PNGDEC_ORDERED) & (set(SO.ORDERED) | set(SO.SYNCHRONOUS) | set(SO.DIAGNOSTIC) | set(PC.PNG_ORDERED))


def test_rows_per_pass_is_the_kernels():
    with open(os.path.join(ROOT, "monkey-pose_amd", "csrc", "k_pngdec.hip")) as f:
        assert re.search(r"constexpr int UNF_ROWS = (\d+);", f.read()).group(1) == str(C.UNFILTER_ROWS)
