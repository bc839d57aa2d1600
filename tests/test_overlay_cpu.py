"""CPU: the drawing rule of the joint overlays.  monkey-pose_amd/csrc/overlay_geom.hpp -- the one text
the kernel includes -- is evaluated by a small host program and compared with the numpy statement of
the rule (monkeydetector.render_overlays_np and its pieces); the numpy renderer is compared with a
brute-force loop that tests every primitive for every pixel; mp_overlay_dev is declared, exported and
validates its arguments before any GPU call (this test runs without a GPU); and the PNG writer of
tools/eval_real_data.py is parsed back."""
import ctypes
import importlib.util
import os
import re
import struct
import subprocess
import zlib

import numpy as np
import pytest

from helpers import ROOT, pkg

CSRC = os.path.join(ROOT, "monkey-pose_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "monkeypose.h")
MP_ERR_ARG, MP_ERR_SHAPE = -1, -5
F32, U16 = 0, 1

GEOM_MAIN = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "overlay_geom.hpp"

// usage: geom index LO HI      float32 values on stdin -> one int32 index each
//        geom center           float32 values on stdin -> per value: int32 eligible, int32 centre
//        geom disc CU CV R X0 Y0 N         -> N*N bytes, disc coverage of the window at (X0, Y0)
//        geom bone PX PY QX QY TH X0 Y0 N  -> N*N bytes, bone coverage (the int64 rule), then N*N
//                                             bytes of the prepared form (BonePlan)
//        geom bmeets PX PY QX QY TH X0 Y0 X1 Y1 -> one byte, the bone's tile test
//        geom box PX PY QX QY GROW X0 Y0 X1 Y1 -> one byte
static std::vector<float> read_floats() {
  std::vector<float> v;
  float b[4096];
  size_t k;
  while ((k = std::fread(b, 4, 4096, stdin)) > 0) v.insert(v.end(), b, b + k);
  return v;
}
int main(int argc, char** argv) {
  if (argc < 2) return 2;
  auto I = [&](int k) { return std::atoi(argv[k]); };
  if (!std::strcmp(argv[1], "index") && argc == 4) {
    const float lo = std::strtof(argv[2], nullptr), hi = std::strtof(argv[3], nullptr);
    std::vector<float> v = read_floats();
    std::vector<int32_t> o(v.size());
    for (size_t i = 0; i < v.size(); ++i) o[i] = mpovl::color_index(v[i], lo, hi);
    return std::fwrite(o.data(), 4, o.size(), stdout) == o.size() ? 0 : 3;
  }
  if (!std::strcmp(argv[1], "center") && argc == 2) {
    std::vector<float> v = read_floats();
    std::vector<int32_t> o(2 * v.size());
    for (size_t i = 0; i < v.size(); ++i) {
      int c = 0;
      o[2 * i] = mpovl::center(v[i], &c);
      o[2 * i + 1] = c;
    }
    return std::fwrite(o.data(), 4, o.size(), stdout) == o.size() ? 0 : 3;
  }
  if (!std::strcmp(argv[1], "disc") && argc == 8) {
    const int n = I(7);
    std::vector<unsigned char> o((size_t)n * n);
    for (int y = 0; y < n; ++y)
      for (int x = 0; x < n; ++x) o[(size_t)y * n + x] = mpovl::disc_covers(I(5) + x, I(6) + y, I(2), I(3), I(4));
    return std::fwrite(o.data(), 1, o.size(), stdout) == o.size() ? 0 : 3;
  }
  if (!std::strcmp(argv[1], "bone") && argc == 10) {
    const int n = I(9);
    std::vector<unsigned char> o((size_t)2 * n * n);
    const mpovl::BonePlan b = mpovl::bone_plan(I(2), I(3), I(4), I(5), I(6));
    for (int y = 0; y < n; ++y)
      for (int x = 0; x < n; ++x) {
        o[(size_t)y * n + x] = mpovl::bone_covers(I(7) + x, I(8) + y, I(2), I(3), I(4), I(5), I(6));
        o[(size_t)(n + y) * n + x] = mpovl::bone_covers(b, I(7) + x, I(8) + y);
      }
    return std::fwrite(o.data(), 1, o.size(), stdout) == o.size() ? 0 : 3;
  }
  if (!std::strcmp(argv[1], "bmeets") && argc == 11) {
    std::putchar(mpovl::bone_meets(mpovl::bone_plan(I(2), I(3), I(4), I(5), I(6)), I(6), I(7), I(8), I(9), I(10)));
    return 0;
  }
  if (!std::strcmp(argv[1], "box") && argc == 11) {
    std::putchar(mpovl::box_meets(I(2), I(3), I(4), I(5), I(6), I(7), I(8), I(9), I(10)));
    return 0;
  }
  return 2;
}
"""


def M():
    return pkg().monkeydetector


@pytest.fixture(scope="module")
def geom_exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("ovlgeom")
    src = d / "geom_main.cpp"
    src.write_text(GEOM_MAIN)
    exe = d / "geom"
    p = subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-I", CSRC, str(src),
                        "-o", str(exe)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    return str(exe)


def _run(exe, *args, stdin=b""):
    p = subprocess.run([exe] + [str(a) for a in args], input=stdin, capture_output=True)
    assert p.returncode == 0, (args, p.stderr)
    return p.stdout


def _f32_neighbours(v):
    v = np.float32(v)
    return [np.nextafter(v, np.float32(-np.inf)), v, np.nextafter(v, np.float32(np.inf))]


def test_header_colour_index_equals_numpy(geom_exe):
    every = np.arange(65536, dtype=np.uint16).astype(np.float32)
    for lo, hi in ((1000, 3000), (0, 65535), (0, 10000), (3000, 1000), (0.5, 10000.25), (-7.25, 123.5),
                   (0.1, 0.3), (65535, 0)):
        lo, hi = np.float32(lo), np.float32(hi)
        edge = []
        for v in (lo, hi, 0, (np.float64(lo) + hi) / 2):
            edge += _f32_neighbours(v)
        edge += [np.nan, np.inf, -np.inf, -0.0, 1e30, -1e30, 1e-45]
        # the values around every index step k / 255
        steps = (np.float64(lo) + (np.arange(256) + 0.5) / 255.0 * (np.float64(hi) - lo)).astype(np.float32)
        edge += [s for v in steps for s in _f32_neighbours(v)]
        vals = np.concatenate([every, np.asarray(edge, np.float32)])
        got = np.frombuffer(_run(geom_exe, "index", repr(float(lo)), repr(float(hi)), stdin=vals.tobytes()), np.int32)
        ref = M().overlay_color_index(vals, lo, hi)
        assert np.array_equal(got, ref), (lo, hi)
        assert got.min() == 0 and got.max() == 255
    # the statement itself, spelled out once more for the reference camera's gate
    lo, hi = np.float32(1000), np.float32(3000)
    x = (every - lo) / (hi - lo)
    k = np.where(x >= 1, 255, np.where(x >= 0, (x * np.float32(255) + np.float32(0.5)).astype(np.int64), 0))
    assert np.array_equal(k, M().overlay_color_index(every, lo, hi))
    assert k[999] == 0 and k[1000] == 0 and k[2000] == 128 and k[3000] == 255 and k[2999] == 255 and k[2996] == 254
    # lo > hi inverts the map
    assert np.array_equal(M().overlay_color_index(every[1000:3001], 3000, 1000)[::-1],
                          M().overlay_color_index(every[1000:3001], 1000, 3000))


def test_header_centres_equal_numpy(geom_exe):
    vals = []
    for v in (-4096.5, 8191.5, -4096, 8191, -4097, 8192, 0, -0.5, 0.5, 1.5, 2.5, -1.5, 255.5, 4095.5, 0.49999997):
        vals += _f32_neighbours(v)
    vals += [np.nan, np.inf, -np.inf, 1e30, -1e30, 3e9, -3e9]
    vals = np.asarray(vals, np.float32)
    got = np.frombuffer(_run(geom_exe, "center", stdin=vals.tobytes()), np.int32).reshape(-1, 2)
    ok, cen = M().overlay_centers(np.stack([vals, np.zeros_like(vals)], axis=1))
    assert np.array_equal(got[:, 0].astype(bool), ok)
    assert np.array_equal(got[ok, 1], cen[ok, 0])
    by = {float(v): (bool(o), int(c)) for v, o, c in zip(vals, got[:, 0], got[:, 1]) if np.isfinite(v)}
    assert by[-4096.5] == (True, -4096) and by[8191.5] == (False, 0) and by[8191.0] == (True, 8191)
    assert by[float(np.nextafter(np.float32(-4096.5), np.float32(-np.inf)))][0] is False
    assert by[float(np.nextafter(np.float32(8191.5), np.float32(-np.inf)))] == (True, 8191)
    assert by[0.5] == (True, 1) and by[1.5] == (True, 2) and by[-0.5] == (True, 0) and by[-1.5] == (True, -1)
    assert not ok[np.isnan(vals) | np.isinf(vals) | (np.abs(vals) > 1e9)].any()


def _window(x0, y0, n=40):
    Y, X = np.mgrid[y0:y0 + n, x0:x0 + n]
    return X, Y


def _bone(exe, P, Q, th, x0, y0, n):
    """the header's coverage of the window: the int64 rule, after checking that the prepared form
    (BonePlan: s, c and L2 as ints) gives the same"""
    both = np.frombuffer(_run(exe, "bone", *P, *Q, th, x0, y0, n), np.uint8).reshape(2, n, n).astype(bool)
    assert np.array_equal(both[0], both[1]), (P, Q, th)
    return both[0]


def test_header_disc_and_bone_coverage_equal_numpy(geom_exe):
    n = 40
    X, Y = _window(-3, -5, n)
    for r in range(16):
        for cu, cv in ((17, 14), (-3, -5), (36, 34), (-10, 12)):
            got = np.frombuffer(_run(geom_exe, "disc", cu, cv, r, -3, -5, n), np.uint8).reshape(n, n).astype(bool)
            assert np.array_equal(got, M().overlay_disc_mask(X, Y, cu, cv, r)), (r, cu, cv)
            if (cu, cv) == (17, 14):
                assert got[cv + 5, cu + 3] and got.sum() == sum(dx * dx + dy * dy <= r * r for dx in range(-r, r + 1)
                                                               for dy in range(-r, r + 1))
    # horizontal, vertical, 45 degrees, shallow, steep, reversed, zero length, and far ends outside
    segs = [((2, 10), (30, 10)), ((12, 1), (12, 33)), ((3, 3), (30, 30)), ((30, 3), (3, 30)), ((1, 8), (34, 13)),
            ((9, 0), (14, 35)), ((34, 13), (1, 8)), ((15, 15), (15, 15)), ((-200, -90), (300, 160)),
            ((5, 20), (4005, 25))]
    for th in range(1, 16):
        for P, Q in segs:
            got = _bone(geom_exe, P, Q, th, -3, -5, n)
            assert np.array_equal(got, M().overlay_bone_mask(X, Y, P, Q, th)), (th, P, Q)
            if P == Q:
                assert not got.any()
            elif th >= 2 and P == (2, 10):
                assert got[15, 5:34].all() and not got[15, :5].any()      # row y = 10, x from 2 to 30: no caps
    # the extreme eligible corners: the int64 bound (|c| < 2^29, 4 c^2 < 2^60), seen from windows at
    # both ends of the pixel range
    P, Q = (-4096, -4096), (8191, 8191)
    for x0, y0 in ((0, 0), (4056, 4056), (4056, 0), (0, 4056), (2000, 1990)):
        Xw, Yw = _window(x0, y0, n)
        for th in (1, 15):
            for A, B in ((P, Q), (Q, P), ((-4096, 8191), (8191, -4096))):
                got = _bone(geom_exe, A, B, th, x0, y0, n)
                ref = M().overlay_bone_mask(Xw, Yw, A, B, th)
                assert np.array_equal(got, ref), (x0, y0, th, A, B)
                # against Python's unbounded integers
                dx, dy = B[0] - A[0], B[1] - A[1]
                L2 = dx * dx + dy * dy
                big = np.array([[(lambda ex, ey: 0 <= ex * dx + ey * dy <= L2
                                  and 4 * (ex * dy - ey * dx) ** 2 <= th * th * L2)(int(x) - A[0], int(y) - A[1])
                                 for x in Xw[0]] for y in Yw[:, 0]])
                assert np.array_equal(got, big)
    assert 4 * (2 * 8192 * 12288) ** 2 < 2 ** 63
    # the culling tests are conservative: a primitive that misses a rectangle covers none of its pixels;
    # and the bone's test is tighter than its box
    rng = np.random.default_rng(0)
    tighter = 0
    for _ in range(150):
        P, Q = tuple(rng.integers(-20, 60, 2)), tuple(rng.integers(-20, 60, 2))
        th = int(rng.integers(1, 16))
        x0, y0 = (int(v) for v in rng.integers(0, 30, 2))
        x1, y1 = x0 + int(rng.integers(1, 12)), y0 + int(rng.integers(1, 12))
        meets = _run(geom_exe, "bmeets", *P, *Q, th, x0, y0, x1, y1)[0]
        box = _run(geom_exe, "box", *P, *Q, th, x0, y0, x1, y1)[0]
        assert box or not meets
        tighter += bool(box and not meets)
        Yr, Xr = np.mgrid[y0:y1, x0:x1]
        if not meets:
            assert not M().overlay_bone_mask(Xr, Yr, P, Q, th).any(), (P, Q, th, x0, y0, x1, y1)
        if not _run(geom_exe, "box", *P, *P, th, x0, y0, x1, y1)[0]:
            assert not M().overlay_disc_mask(Xr, Yr, P[0], P[1], th).any()
    assert tighter > 10
    # a long diagonal: its box holds the whole window, its line only the tiles along it
    assert _run(geom_exe, "box", 0, 0, 4000, 4000, 3, 3000, 100, 3128, 108)[0] == 1
    assert _run(geom_exe, "bmeets", 0, 0, 4000, 4000, 3, 3000, 100, 3128, 108)[0] == 0
    assert _run(geom_exe, "bmeets", 0, 0, 4000, 4000, 3, 3000, 3000, 3128, 3008)[0] == 1
    for x0 in range(0, 4096, 128):                       # exhaustive along one tile row against the rule
        Yr, Xr = np.mgrid[1000:1008, x0:x0 + 128]
        any_px = bool(M().overlay_bone_mask(Xr, Yr, (-4096, -4096), (8191, 8000), 15).any())
        meets = _run(geom_exe, "bmeets", -4096, -4096, 8191, 8000, 15, x0, 1000, x0 + 128, 1008)[0]
        assert meets or not any_px
        assert meets == any_px or abs(x0 - 1000) < 400     # tight away from the crossing


def _brute(frames, ju, bones, lo, hi, table, styles):
    """every primitive for every pixel, in drawing order"""
    Mo = M()
    n, h, w = frames.shape
    S, J = ju.shape[1], ju.shape[2]
    out = np.zeros((n, h, w, 3), np.uint8)
    for i in range(n):
        ok, cen = Mo.overlay_centers(ju[i, :, :, :2])
        for y in range(h):
            for x in range(w):
                rgb = table[int(Mo.overlay_color_index(np.float32(frames[i, y, x]), lo, hi))]
                for s in range(S):
                    m_rgb, b_rgb, r, th = styles[s]
                    for a, b in bones:
                        if ok[s, a] and ok[s, b]:
                            P, Q = [int(v) for v in cen[s, a]], [int(v) for v in cen[s, b]]
                            dx, dy = Q[0] - P[0], Q[1] - P[1]
                            L2 = dx * dx + dy * dy
                            ex, ey = x - P[0], y - P[1]
                            sdot, c = ex * dx + ey * dy, ex * dy - ey * dx
                            if L2 > 0 and 0 <= sdot <= L2 and 4 * c * c <= th * th * L2:
                                rgb = b_rgb
                    for j in range(J):
                        if ok[s, j] and (x - int(cen[s, j, 0])) ** 2 + (y - int(cen[s, j, 1])) ** 2 <= r * r:
                            rgb = m_rgb
                out[i, y, x] = rgb
    return out


def test_numpy_renderer_equals_brute_force():
    Mo = M()
    styles = (((0, 255, 0), (0, 160, 0), 3, 1), ((255, 0, 0), (200, 0, 200), 2, 3),
              ((0, 0, 255), (90, 90, 255), 0, 2), ((255, 255, 0), (200, 200, 0), 5, 4))
    for seed, (n, h, w, S, J) in enumerate([(2, 20, 24, 2, 6), (1, 1, 1, 1, 2), (1, 7, 5, 4, 3), (2, 24, 20, 3, 5)]):
        rng = np.random.default_rng(seed)
        ju = np.zeros((n, S, J, 3), np.float32)
        ju[..., 0] = rng.uniform(-5, w + 5, (n, S, J))
        ju[..., 1] = rng.uniform(-5, h + 5, (n, S, J))
        if J > 2:
            ju[0, S - 1, 1] = np.nan                                   # a padded joint: no marker, no bone
            ju[0, 0, 2, 0] = 9000                                      # past the eligible range
        bones = [(k, k + 1) for k in range(J - 1)] + [(J - 1, 0), (0, 0)]
        table = Mo.overlay_lut("jet")
        for dt, rng_d in ((np.uint16, (1000, 3000)), (np.float32, (0.1, 0.3))):
            mm = rng.integers(500, 3500, (n, h, w))
            fr = mm.astype(np.uint16) if dt == np.uint16 else (mm / np.float32(10000.)).astype(np.float32)
            got = Mo.render_overlays_np(fr, ju, bones=bones, depth_range=rng_d, lut="jet", styles=styles)
            ref = _brute(fr, ju, bones, np.float32(rng_d[0]), np.float32(rng_d[1]), table, styles)
            assert got.dtype == np.uint8 and np.array_equal(got, ref), (seed, dt)
        assert np.array_equal(Mo.render_overlays_np(fr[..., None], ju[:, 0], depth_range=rng_d, styles=styles),
                              _brute(fr, ju[:, :1], [], np.float32(rng_d[0]), np.float32(rng_d[1]),
                                     Mo.overlay_lut("gray"), styles))


def test_colour_tables():
    Mo = M()
    g, j = Mo.overlay_lut("gray"), Mo.overlay_lut("jet")
    assert g.shape == j.shape == (256, 3) and g.dtype == j.dtype == np.uint8
    assert np.array_equal(g[:, 0], np.arange(256)) and (g[:, 0] == g[:, 1]).all() and (g[:, 1] == g[:, 2]).all()
    assert tuple(j[0]) == (0, 0, 128) and tuple(j[255]) == (128, 0, 0) and j[64, 2] == 255 and j[192, 0] == 255
    assert len(np.unique(j, axis=0)) == 256
    with pytest.raises(ValueError):
        Mo.overlay_lut("viridis")


def _header_functions():
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return set(re.findall(r"\b(mp_[a-z0-9_]+)\s*\(", txt))


def test_header_table_and_library_list_the_overlay_calls():
    mp = pkg()
    out = subprocess.run(["nm", "-D", "--defined-only", mp._lib.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = set(re.findall(r" T (mp_[a-z0-9_]+)", out))
    for f in ("mp_overlay_dev", "mp_transform_joints_dev"):
        assert f in _header_functions(), f
        assert f in mp.monkeydetector._CROP_SIGS, f
        assert f in exported, f
    assert mp._lib.load().mp_version() == 3     # additive: the version is not bumped
    assert ctypes.sizeof(mp.monkeydetector.OverlayStyle) == 40
    assert "overlay_geom.hpp" in open(os.path.join(CSRC, "Makefile")).read()


def test_overlay_call_validates_before_any_gpu_call():
    """no GPU here: a call that reached the HIP runtime would return MP_ERR_HIP, not these codes"""
    Mo = M()
    lib = Mo._lib_crop()
    buf = np.zeros(8192, np.uint8)                      # host memory: only its address is looked at
    p = buf.ctypes.data
    assert p % 8 == 0
    P = ctypes.c_void_p
    style = Mo.OverlayStyle(struct_size=ctypes.sizeof(Mo.OverlayStyle))
    for s in range(4):
        style.sets[s].radius, style.sets[s].thickness = 3, 1
    bones = np.array([[0, 1], [1, 2]], np.int32)

    def call(frames=p, dt=U16, shape=(2, 8, 16), lo=1000.0, hi=3000.0, lut=p + 1024, joints=p + 2048, S=2, J=3,
             b=bones, nb=2, st=style, out=p + 4096 + 1):
        return lib.mp_overlay_dev(P(frames), dt, *shape, lo, hi, P(lut), P(joints), S, J,
                                  None if b is None else b.ctypes.data_as(P), nb,
                                  None if st is None else ctypes.byref(st), P(out), None)

    for S in (0, 5, -1):
        assert call(S=S) == MP_ERR_SHAPE
    for J in (-1, 129):
        assert call(J=J) == MP_ERR_SHAPE
    assert call(nb=257) == MP_ERR_SHAPE and call(nb=-1) == MP_ERR_SHAPE
    for bad in ([[0, 3], [1, 2]], [[0, 1], [-1, 2]]):
        assert call(b=np.array(bad, np.int32)) == MP_ERR_ARG
        assert b"bone index" in lib.mp_last_error()
    assert call(J=0) == MP_ERR_ARG                                   # bones need joints
    for shape in ((2, 4097, 16), (2, 8, 4097), (0, 8, 16), (2, 0, 16), (65536, 8, 16)):
        assert call(shape=shape) == MP_ERR_SHAPE
    assert call(lo=5.0, hi=5.0) == MP_ERR_ARG
    for lo, hi in ((float("nan"), 1.0), (0.0, float("inf")), (float("-inf"), 0.0)):
        assert call(lo=lo, hi=hi) == MP_ERR_ARG
    for dt in (2, 7, -1):
        assert call(dt=dt) == MP_ERR_ARG
    assert call(frames=p + 1, dt=U16) == MP_ERR_ARG                  # misaligned frames
    assert call(frames=p + 2, dt=F32) == MP_ERR_ARG
    assert call(joints=p + 2050) == MP_ERR_ARG
    for kw in (dict(frames=None), dict(lut=None), dict(joints=None), dict(b=None), dict(st=None), dict(out=None)):
        assert call(**kw) == MP_ERR_ARG, kw
    for size in (0, 32, 39, 48):                                     # a style struct of another size
        wrong = Mo.OverlayStyle(struct_size=size)
        assert call(st=wrong) == MP_ERR_ARG
        assert b"struct_size" in lib.mp_last_error()
    for r, th in ((16, 1), (3, 0), (3, 16)):
        bad = Mo.OverlayStyle(struct_size=ctypes.sizeof(Mo.OverlayStyle))
        for s in range(4):
            bad.sets[s].radius, bad.sets[s].thickness = 3, 1
        bad.sets[1].radius, bad.sets[1].thickness = r, th
        assert call(st=bad) == MP_ERR_ARG
    tj = lib.mp_transform_joints_dev
    assert tj(None, P(p), 2, 3, P(p + 64), None) == MP_ERR_ARG
    assert tj(P(p), P(p + 64), 0, 3, P(p + 128), None) == MP_ERR_SHAPE
    assert tj(P(p), P(p + 4), 2, 3, P(p + 128), None) == MP_ERR_ARG   # Ms off an 8-byte boundary


def test_facade_validates_before_gpu():
    import torch
    Mo = M()
    fr = torch.zeros((2, 8, 16), dtype=torch.uint16)
    ju = torch.zeros((2, 2, 5, 3), dtype=torch.float32)
    with pytest.raises(TypeError):                      # CPU tensors, once everything else is in order
        Mo.render_overlays(fr, ju, bones=[(0, 1)])
    with pytest.raises(TypeError):
        Mo.render_overlays(fr.numpy(), ju.numpy())
    for kw in (dict(bones=[(0, 5)]), dict(bones=[(0, 1, 2)]), dict(bones=np.zeros((257, 2), np.int64)),
               dict(depth_range=(5, 5)), dict(depth_range=(0, float("inf"))), dict(depth_range=5),
               dict(lut="viridis"), dict(lut=np.zeros((255, 3), np.uint8)), dict(styles=[((0, 0, 0), (0, 0, 0), 3, 1)]),
               dict(styles=[((0, 0, 0), (0, 0, 0), 16, 1)] * 2), dict(styles=[((0, 0, 0), (0, 0, 0), 3, 0)] * 2),
               dict(styles=[((0, 0, 256), (0, 0, 0), 3, 1)] * 2), dict(out=torch.zeros(5, dtype=torch.uint8))):
        with pytest.raises(ValueError):
            Mo.render_overlays(fr, ju, **kw)
        if "out" not in kw:
            with pytest.raises(ValueError):
                Mo.render_overlays_np(fr.numpy(), ju.numpy(), **kw)
    for f, j in ((torch.zeros((2, 8, 4097), dtype=torch.uint16), ju), (fr, torch.zeros((2, 5, 5, 3))),
                 (fr, torch.zeros((2, 2, 129, 3))), (fr, torch.zeros((3, 2, 5, 3))), (fr, torch.zeros((2, 2, 5, 2))),
                 (torch.zeros((2, 8, 16, 3), dtype=torch.uint16), ju)):
        with pytest.raises(ValueError):
            Mo.render_overlays(f, j)
    with pytest.raises(TypeError):
        Mo.render_overlays(fr.to(torch.int32), ju)
    with pytest.raises(TypeError):
        Mo.render_overlays(fr, ju.double())
    md = Mo.MonkeyDetector(365.456, 365.456, 256, 212, [800, 800, 1200], 200, 10000)
    with pytest.raises(TypeError):
        md.transform_joints_device(torch.zeros((2, 5, 3)), torch.zeros((2, 3, 3), dtype=torch.float64))
    with pytest.raises(ValueError):
        md.transform_joints_device(torch.zeros((2, 5, 3)), torch.zeros((3, 3, 3), dtype=torch.float64))


def _tool():
    spec = importlib.util.spec_from_file_location("eval_real_data_tool", os.path.join(ROOT, "tools", "eval_real_data.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _read_png(data):
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, chunks = 8, []
    while pos < len(data):
        (length,), kind = struct.unpack(">I", data[pos:pos + 4]), data[pos + 4:pos + 8]
        body = data[pos + 8:pos + 8 + length]
        (crc,) = struct.unpack(">I", data[pos + 8 + length:pos + 12 + length])
        assert crc == zlib.crc32(kind + body) & 0xffffffff, kind
        chunks.append((kind, body))
        pos += 12 + length
    assert pos == len(data)
    assert chunks[0][0] == b"IHDR" and chunks[-1] == (b"IEND", b"")
    w, h, depth, colour, comp, filt, lace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, colour, comp, filt, lace) == (8, 2, 0, 0, 0)          # 8-bit RGB, not interlaced
    raw = zlib.decompress(b"".join(b for k, b in chunks if k == b"IDAT"))
    rows = np.frombuffer(raw, np.uint8).reshape(h, 1 + 3 * w)
    assert (rows[:, 0] == 0).all()                                       # filter 0 on every row
    return rows[:, 1:].reshape(h, w, 3)


def test_png_writer_round_trip(tmp_path):
    tool = _tool()
    rng = np.random.default_rng(0)
    for h, w in ((1, 1), (7, 5), (33, 67)):
        rgb = rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
        path = tmp_path / f"o_{h}_{w}.png"
        tool.write_png(str(path), rgb)
        assert np.array_equal(_read_png(path.read_bytes()), rgb)
    with pytest.raises(ValueError):
        tool.write_png(str(tmp_path / "bad.png"), np.zeros((4, 4), np.uint8))
    assert tool.read_bones(None) is None
    bj = tmp_path / "bones.json"
    bj.write_text("[[0, 1], [1, 2], [2, 5]]")
    assert tool.read_bones(str(bj)) == [(0, 1), (1, 2), (2, 5)]
