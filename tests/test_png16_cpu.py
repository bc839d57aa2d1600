"""mp_png16_encode_host (include/monkeypose_png16.h; the rule is csrc/png16_rule.hpp) on this machine, no
GPU: the case list of tests/png16_cases.py reaches every corner of the rule (mp_png16_band_stats_host),
every file decodes to its frame bit for bit with three decoders that share no code with the encoder
(PIL, zlib plus a numpy restatement of the filter rule, and the library's own mp_png_decode_host), the
two size bounds hold, refusals come before anything is written, and the rule alone -- built as a host
program with the address and undefined-behaviour sanitizers -- writes the library's bytes."""
import ctypes
import hashlib
import io
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import png16_cases as C
import png_cases as PC
import pngdec_cases as DC
import stream_order_cases as SO
from helpers import ROOT, pkg

MP_ERR_ARG, MP_ERR_SHAPE = -1, -5


def _files(name):
    buf, sizes = C.host_files(name)
    return [buf[i, :s].tobytes() for i, s in enumerate(sizes)]


# ------------------------------------------------------------------------------------------ coverage
def _all_stats():
    return np.concatenate([C.stats(n).reshape(-1, 9) for n in C.NAMES])


def test_the_cases_reach_every_corner_of_the_rule():
    st = _all_stats()
    assert set(st[:, C.S_FORM]) == {C.FORM_STORED, C.FORM_FIXED, C.FORM_DYNAMIC}
    assert (st[:, C.S_FILTERS].sum(axis=0) > 0).all(), st[:, C.S_FILTERS].sum(axis=0)
    assert st[:, C.S_DEPTH].max() > 15
    dyn = st[st[:, C.S_FORM] == C.FORM_DYNAMIC]
    assert dyn[:, C.S_DEPTH].max() > 15                          # .. in a band that is written with that code
    assert ((dyn[:, C.S_MATCHES] == 0) & (dyn[:, C.S_DIST] == 0)).any()          # no distance code at all
    assert ((dyn[:, C.S_MATCHES] > 0) & (dyn[:, C.S_DIST] == 1)).any()           # one code of one bit
    assert dyn[:, C.S_DIST].max() >= 3


def test_the_named_cases_are_what_their_names_say():
    assert (C.stats("random-9x512")[..., C.S_FORM] == C.FORM_STORED).all()
    z = C.stats("zero-424x512")[0]
    assert (z[:, C.S_DIST] == 1).all() and (z[:, C.S_FORM] == C.FORM_DYNAMIC).all()
    assert (z[:-1, C.S_MATCHES] == -(-(7 * 1025 - 1) // 258)).all()              # 258 long, but a band's last
    assert (C.stats("no-match-4x20")[..., C.S_MATCHES] == 0).all()
    d = C.stats("deep-tree")[0, 0]
    assert (d[C.S_DEPTH], d[C.S_MATCHES], d[C.S_FORM]) == (17, 0, C.FORM_DYNAMIC)
    assert (C.stats("five-filters")[0, 0, C.S_FILTERS] > 0).all()
    assert [s.shape[1] for s in map(C.stats, ("2x4096", "2x4095", "9x512", "8x512-seam"))] == [2, 2, 2, 2]
    assert C.stats("8x512-seam")[0, 1, C.S_FILTERS][[2, 4]].sum() == 1            # the seam row takes Up or Paeth
    assert C.P().depth_band_plan(9, 512) == (7, 2) and C.P().depth_band_plan(2, 4096) == (1, 2)
    assert C.P().depth_band_plan(3, 1) == (2730, 1)


@pytest.mark.parametrize("name", C.NAMES)
def test_stats_are_what_the_files_hold(name):
    x, st = C.frames(name), C.stats(name)
    for i, f in enumerate(_files(name)):
        assert C.band_forms(f, *x.shape[1:]) == list(st[i, :, C.S_FORM])
        rows = C.raw_stream(f, *x.shape[1:])
        assert list(np.bincount(rows[:, 0], minlength=5)) == list(st[i, :, C.S_FILTERS].sum(axis=0))


# ------------------------------------------------------------------------------------------ decoders
@pytest.mark.parametrize("name", C.NAMES)
def test_pil_reads_the_frames(name):
    from PIL import Image
    x = C.frames(name)
    for i, f in enumerate(_files(name)):
        im = Image.open(io.BytesIO(f))
        assert im.mode == "I;16" and im.size == (x.shape[2], x.shape[1])
        got = np.asarray(im)
        assert got.dtype == np.uint16 and np.array_equal(got, x[i])


@pytest.mark.parametrize("name", C.NAMES)
def test_zlib_inflates_to_the_filter_rule(name):
    x = C.frames(name)
    for i, f in enumerate(_files(name)):
        rows = C.raw_stream(f, *x.shape[1:])
        assert np.array_equal(rows, C.filtered_rows(x[i])), f"frame {i}"


def test_the_filtered_rows_reconstruct_by_the_specification():
    for name in ("five-filters", "byte-order", "3x1", "n3", "8x512-seam"):
        x = C.frames(name)
        for i in range(x.shape[0]):
            assert np.array_equal(C.unfiltered(C.filtered_rows(x[i]), *x.shape[1:]), x[i])


@pytest.mark.parametrize("name", C.NAMES)
def test_the_library_decoder_reads_the_frames(name):
    x = C.frames(name)
    buf, sizes = C.host_files(name)
    got, status = C.P().decode_png(np.ascontiguousarray(buf), np.array(sizes), x.shape[1], x.shape[2], check=False)
    assert not status.any()
    assert got.dtype == np.uint16 and np.array_equal(got, x)


def test_save_and_load_depth_maps(tmp_path):
    x = C.frames("n3")
    paths = [str(tmp_path / f"depth_{i:06d}.png") for i in range(3)]
    C.P().save_depth_maps(paths, x)
    for i, p in enumerate(paths):
        assert np.array_equal(C.P().load_depth_map(p), x[i].astype(np.float32))
    assert np.array_equal(C.P().decode_png_files(paths), x)
    with pytest.raises(ValueError):
        C.P().save_depth_maps(paths[:2], x)


def test_a_file_does_not_depend_on_its_batch():
    x = C.frames("n3")
    for i, f in enumerate(_files("n3")):
        assert C.P().png_files(*C.P().encode_depth_png(x[i:i + 1])) == [f]


def test_host_files_equal_the_recorded_bytes():
    """every case's size and SHA-256 (tests/golden/png16/digests.json), and the whole files where they are kept"""
    with open(os.path.join(C.GOLDEN_DIR, "digests.json")) as f:
        table = json.load(f)
    assert sorted(table) == sorted(C.NAMES)
    for name in C.NAMES:
        got = [{"sha256": hashlib.sha256(f).hexdigest(), "size": len(f)} for f in _files(name)]
        assert got == table[name], name
    for name in C.GOLDEN:
        with open(os.path.join(C.GOLDEN_DIR, name + ".png"), "rb") as f:
            assert _files(name) == [f.read()], name


# ------------------------------------------------------------------------------------------ sizes
@pytest.mark.parametrize("name", C.NAMES)
def test_sizes_are_within_the_bound(name):
    x = C.frames(name)
    _, sizes = C.host_files(name)
    bound = C.P().depth_png_bound(*x.shape[1:])
    rows, nb = C.P().depth_band_plan(*x.shape[1:])
    assert bound == 33 + 2 + 28 + nb * 22 + x.shape[1] * (1 + 2 * x.shape[2])
    assert (sizes <= bound).all() and (sizes > 0).all()


def test_a_constant_frame_is_below_a_thirty_second_of_its_raw_bytes():
    x = C.frames("zero-424x512")
    _, sizes = C.host_files("zero-424x512")
    print("constant 424 x 512:", int(sizes[0]), "bytes of", x[0].nbytes)
    assert sizes[0] * 32 < x[0].nbytes
    const = np.full((1, 424, 512), 2500, np.uint16)
    _, cs = C.P().encode_depth_png(const)
    print("constant 2500:", int(cs[0]))
    assert cs[0] * 32 < const.nbytes


# ------------------------------------------------------------------------------------------ errors
def test_entry_refusals_touch_nothing():
    lib = C.P()._lib_png()
    frames = np.arange(16, dtype=np.uint16).reshape(1, 4, 4)
    bound = C.P().depth_png_bound(4, 4)
    out, sizes = np.full(bound + 2, 0xA5, np.uint8), np.full(2, -7, np.int64)
    stats = np.full(9, -7, np.int32)
    f, o, s, t = frames.ctypes.data, out.ctypes.data, sizes.ctypes.data, stats.ctypes.data
    for n, h, w, stride in ((0, 4, 4, bound), (65536, 4, 4, bound), (1, 0, 4, bound), (1, 4, 0, bound),
                            (1, 4097, 4, 1 << 30), (1, 4, 4097, 1 << 30), (1, 4, 4, bound - 1)):
        assert lib.mp_png16_encode_host(f, n, h, w, o, stride, s) == MP_ERR_SHAPE, (n, h, w, stride)
        assert lib.mp_png16_encode_dev(f, n, h, w, o, stride, s, o, None) == MP_ERR_SHAPE, (n, h, w, stride)
        if stride != bound - 1:
            assert lib.mp_png16_band_stats_host(f, n, h, w, t) == MP_ERR_SHAPE
            assert lib.mp_png16_work_bytes(n, h, w) == 0
    assert lib.mp_png16_bound(0, 4) == 0 and lib.mp_png16_bound(4, 4097) == 0
    assert lib.mp_png16_band_rows(0) == 0 and lib.mp_png16_band_count(4097, 4) == 0
    for args in ((None, 1, 4, 4, o, bound, s), (f, 1, 4, 4, None, bound, s), (f, 1, 4, 4, o, bound, None),
                 (f + 1, 1, 4, 4, o, bound, s), (f, 1, 4, 4, o, bound, s + 4)):
        assert lib.mp_png16_encode_host(*args) == MP_ERR_ARG
        assert lib.mp_png16_encode_dev(*args, o, None) == MP_ERR_ARG
    aligned = o + (-o) % 16
    assert lib.mp_png16_encode_dev(f, 1, 4, 4, o, bound, s, None, None) == MP_ERR_ARG        # no launch: host pointers
    assert lib.mp_png16_encode_dev(f, 1, 4, 4, o, bound, s, aligned + 4, None) == MP_ERR_ARG
    assert b"mp_png16_encode_dev" in pkg()._lib.load().mp_last_error()
    for args in ((None, 1, 4, 4, t), (f, 1, 4, 4, None), (f + 1, 1, 4, 4, t), (f, 1, 4, 4, t + 2)):
        assert lib.mp_png16_band_stats_host(*args) == MP_ERR_ARG
    assert (out == 0xA5).all() and (sizes == -7).all() and (stats == -7).all()
    # an odd out address and a wider stride are fine
    x = C.frames("n3")
    n, h, w = x.shape
    b3 = C.P().depth_png_bound(h, w)
    stride, guard = b3 + 3, 32
    dst = np.full(guard + 1 + n * stride + guard, 0xA5, np.uint8)
    sz = np.zeros(n, np.int64)
    assert lib.mp_png16_encode_host(x.ctypes.data, n, h, w, dst.ctypes.data + guard + 1, stride, sz.ctypes.data) == 0
    ref, rs = C.host_files("n3")
    assert np.array_equal(sz, rs)
    assert (dst[:guard + 1] == 0xA5).all() and (dst[guard + 1 + n * stride:] == 0xA5).all()
    body = dst[guard + 1:guard + 1 + n * stride].reshape(n, stride)
    for i in range(n):
        assert body[i, :rs[i]].tobytes() == ref[i, :rs[i]].tobytes() and (body[i, rs[i]:] == 0xA5).all()


def test_python_layer_refusals():
    P = C.P()
    import torch
    x = C.frames("n3")
    with pytest.raises(TypeError):
        P.encode_depth_png(x.astype(np.int16))
    with pytest.raises(TypeError):
        P.encode_depth_png(x.astype(np.float32))
    with pytest.raises(ValueError):
        P.encode_depth_png(x[0])
    with pytest.raises(ValueError):
        P.encode_depth_png(np.zeros((1, 4097, 2), np.uint16))
    with pytest.raises(ValueError):
        P.encode_depth_png(x, out=(None, None))
    with pytest.raises(TypeError):
        P.encode_depth_png(torch.from_numpy(x.copy()))             # a host tensor: no quiet fallback
    with pytest.raises(TypeError):
        P.encode_depth_png(x.tolist())
    with pytest.raises(ValueError):
        P.depth_png_bound(0, 5)
    with pytest.raises(TypeError):
        P.depth_band_stats(x.astype(np.uint8))
    sl = x[:, ::2, ::3]                                            # a strided view is made contiguous
    assert P.png_files(*P.encode_depth_png(sl)) == P.png_files(*P.encode_depth_png(np.ascontiguousarray(sl)))


# ------------------------------------------------------------------------------------------ the rule alone
@pytest.fixture(scope="module")
def rule_program(tmp_path_factory):
    """tests/png16_rule_main.cpp with the address and undefined-behaviour sanitizers: a host program"""
    if not shutil.which("g++"):
        pytest.fail("g++ is needed to build the rule's host program")
    exe = str(tmp_path_factory.mktemp("rule16") / "png16_rule_main")
    p = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "png16_rule_main.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    return exe


def _fnv(b):
    h = 1469598103934665603
    for x in bytes(b):
        h = ((h ^ x) * 1099511628211) & (2 ** 64 - 1)
    return h


def test_sanitized_rule_writes_the_library_files(rule_program, tmp_path):
    lines, want = [], []
    for k, name in enumerate(C.NAMES):
        x = C.frames(name)
        path = str(tmp_path / f"{k}.u16")
        x.tofile(path)
        lines.append(f"{path} {x.shape[0]} {x.shape[1]} {x.shape[2]}")
        for i, f in enumerate(_files(name)):
            want.append((len(f), _fnv(f), _fnv(C.stats(name)[i].tobytes())))
    man = str(tmp_path / "manifest.txt")
    with open(man, "w") as f:
        f.write("\n".join(lines) + "\n")
    p = subprocess.run([rule_program, man], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and not p.stderr, p.stderr[-4000:]              # a sanitizer report ends the program
    got = [(int(a), int(b, 16), int(c, 16)) for a, b, c in (r.split() for r in p.stdout.splitlines())]
    assert got == want


# ------------------------------------------------------------------------------------------ the header
def _declared():
    return SO.exported_functions(C.PNG16_HEADER)


def test_header_compiles_as_c99():
    src = ('#include "monkeypose_png16.h"\nint main(void){ return MP_OK + MP_PNG16_STAT_INTS * 0 + '
           '(int)sizeof(&mp_png16_encode_dev) * 0; }\n')
    p = subprocess.run(["gcc", "-x", "c", "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-I",
                        os.path.dirname(C.PNG16_HEADER), "-"], input=src, text=True, capture_output=True)
    assert p.returncode == 0, p.stderr


def test_library_exports_what_the_header_declares():
    out = subprocess.run(["nm", "-D", "--defined-only", pkg()._lib.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = set(re.findall(r" T (mp_[a-z0-9_]+)", out))
    assert _declared() == ["mp_png16_band_count", "mp_png16_band_rows", "mp_png16_band_stats_host", "mp_png16_bound",
                           "mp_png16_encode_dev", "mp_png16_encode_host", "mp_png16_work_bytes"]
    assert not set(_declared()) - exported


def test_ctypes_tables_are_the_function_lists():
    P = C.P()
    assert sorted(P._PNG16_SIGS) == _declared()
    assert P._PNG16_SIGS["mp_png16_encode_dev"][1][-1] is ctypes.c_void_p
    assert sorted(P._PNG_SIGS) == SO.exported_functions(PC.PNG_HEADER)           # the RGB encoder's table is unchanged
    assert sorted(P._PNGDEC_SIGS) == SO.exported_functions(DC.PNGDEC_HEADER)     # and the decoder's
    with open(C.PNG16_HEADER) as f:
        assert int(re.search(r"#define MP_PNG16_STAT_INTS (\d+)", f.read()).group(1)) == P.STAT_INTS == 9


def test_stream_prototypes_are_the_ordered_cases():
    assert sorted(SO.stream_prototypes(C.PNG16_HEADER)) == sorted(C.PNG16_ORDERED) == ["mp_png16_encode_dev"]
    assert all(C.PNG16_ORDERED.values())
    assert not set(C.PNG16_ORDERED) & (set(SO.ORDERED) | set(SO.SYNCHRONOUS) | set(SO.DIAGNOSTIC) | set(PC.PNG_ORDERED)
                                       | set(DC.PNGDEC_ORDERED))
