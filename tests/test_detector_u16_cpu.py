"""CPU: the uint16 pixel rules of monkey-pose_amd/csrc/depth_u16.hpp -- the one text the host crop and
the device kernels include -- evaluated by a small host program for all 65,536 pixel values, equal
numpy's float64 comparisons and its store into a uint16 array; the header declares the detector's
*_dt entry points, the ctypes table lists them, the library exports them; they validate their
arguments before any GPU call (this test runs without a GPU), and so does the façade."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from helpers import ROOT, pkg

CSRC = os.path.join(ROOT, "monkey-pose_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "monkeypose.h")
NEW_FUNCS = ("mp_center_of_mass_dev_work_dt", "mp_center_of_mass_dev_dt", "mp_crop3d_dev_coms_dt")
CAM = (365.456, 365.456, 256, 212, [800, 800, 1200], 200, 10000)
MP_ERR_ARG, MP_ERR_SHAPE = -1, -5
F32, U16 = 0, 1

# (min_depth, max_depth) of calculateCoM's threshold: the reference camera's, fractional, negative,
# zero, the top of the pixel range and beyond it, min > max, and NaN (every comparison false)
COM_BOUNDS = [(200.0, 10000.0), (200.5, 9999.5), (-3.7, 10000.0), (0.0, 65535.0), (65535.0, 65535.5),
              (65535.5, 70000.0), (70000.0, 80000.0), (-3.7, -1.0), (10000.0, 200.0), (0.0, 0.0),
              (-0.0, 0.5), (0.5, 0.5), (1.0, 1.0), (float("nan"), 10000.0), (200.0, float("nan"))]
# (zstart, zend) of getCrop's rule, zstart in [-1e6, 65535] so that numpy's stored value is defined
CROP_BOUNDS = [(900.0, 2100.0), (900.7, 2100.7), (0.5, 1200.5), (0.0, 1200.0), (-3.7, 1196.3),
               (-1e6, -998800.0), (65535.0, 66735.0), (65534.99, 66734.99), (64999.5, 65535.5), (200.0, 200.0),
               (1.0, 65534.5)]

RULES_MAIN = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "depth_u16.hpp"

// usage: rules com MIN MAX      -> 65536 bytes com_out(v, MIN, MAX), then 65536 bytes com_out(v, com_bounds(MIN, MAX))
//        rules crop ZSTART ZEND -> 65536 uint16 crop_px(v, ZSTART, ZEND)
int main(int argc, char** argv) {
  if (argc != 4) return 2;
  const double a = std::strtod(argv[2], nullptr), b = std::strtod(argv[3], nullptr);
  if (!std::strcmp(argv[1], "com")) {
    std::vector<unsigned char> o(2 * 65536);
    const mpu16::ComBounds ib = mpu16::com_bounds(a, b);
    for (int v = 0; v < 65536; ++v) {
      o[v] = mpu16::com_out((uint16_t)v, a, b);
      o[65536 + v] = mpu16::com_out((uint16_t)v, ib);
    }
    return std::fwrite(o.data(), 1, o.size(), stdout) == o.size() ? 0 : 3;
  }
  if (!std::strcmp(argv[1], "crop")) {
    std::vector<uint16_t> o(65536);
    for (int v = 0; v < 65536; ++v) o[v] = mpu16::crop_px((uint16_t)v, a, b);
    return std::fwrite(o.data(), 2, o.size(), stdout) == o.size() ? 0 : 3;
  }
  return 2;
}
"""


@pytest.fixture(scope="module")
def rules_exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("u16rules")
    src = d / "rules_main.cpp"
    src.write_text(RULES_MAIN)
    exe = d / "rules"
    p = subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-I", CSRC, str(src),
                        "-o", str(exe)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    return str(exe)


def _run(exe, mode, a, b):
    p = subprocess.run([exe, mode, repr(a), repr(b)], capture_output=True)
    assert p.returncode == 0, p.stderr
    return p.stdout


def test_header_rules_equal_numpy_for_every_pixel_value(rules_exe):
    v = np.arange(65536, dtype=np.uint16)
    vd = v.astype(np.float64)
    for lo, hi in COM_BOUNDS:
        got = np.frombuffer(_run(rules_exe, "com", lo, hi), np.uint8).reshape(2, 65536).astype(bool)
        ref = (vd < lo) | (vd > hi)                        # dc[dc < minDepth] = 0; dc[dc > maxDepth] = 0
        assert np.array_equal(got[0], ref), (lo, hi)       # the float64 comparison (the host)
        assert np.array_equal(got[1], ref), (lo, hi)       # the integer bounds (the CoM kernel)
    assert ((vd < 10000.0) | (vd > 200.0)).all()           # min > max zeroes every pixel
    for zs, ze in CROP_BOUNDS:
        got = np.frombuffer(_run(rules_exe, "crop", zs, ze), np.uint16)
        ref = v.copy()                                     # getCrop (monkeydetector.py:208-212)
        m1 = (vd < zs) & (v != 0)
        m2 = (vd > ze) & (v != 0)
        if m1.any():
            assert 0.0 <= zs <= 65535.0
            ref[m1] = zs                                   # the store truncates
        ref[m2] = 0.
        assert np.array_equal(got, ref), (zs, ze)
    # the truncation is observable: a pixel below 900.7 is stored as 900, not 901
    assert np.frombuffer(_run(rules_exe, "crop", 900.7, 2100.7), np.uint16)[5] == 900


def _header_functions():
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return set(re.findall(r"\b(mp_[a-z0-9_]+)\s*\(", txt))


def test_header_table_and_library_list_the_dtype_calls():
    mp = pkg()
    fns = _header_functions()
    out = subprocess.run(["nm", "-D", "--defined-only", mp._lib.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = set(re.findall(r" T (mp_[a-z0-9_]+)", out))
    for f in NEW_FUNCS:
        assert f in fns, f
        assert f in mp.monkeydetector._CROP_SIGS, f
        assert f in exported, f
    assert mp._lib.load().mp_version() == 3     # additive: the version is not bumped


def test_dtype_calls_validate_before_any_gpu_call():
    """no GPU here: a call that reached the HIP runtime would return MP_ERR_HIP, not these codes"""
    mp = pkg()
    lib = mp.monkeydetector._lib_crop()
    cam = mp.monkeydetector.MonkeyDetector(*CAM)._cam()
    c = ctypes.byref(cam)
    buf = np.zeros(4096, np.uint8)                      # host memory: only its address is looked at
    p = buf.ctypes.data
    assert p % 8 == 0
    P = ctypes.c_void_p
    n, h, w = 2, 8, 16

    def com(frames, dt, scale, coms=p, work=p + 64, nbytes=2048, shape=(n, h, w)):
        return lib.mp_center_of_mass_dev_dt(c, P(frames), dt, *shape, scale, P(coms), P(work), nbytes, None)

    def crop(frames, dt, scale, coms=p + 64, coms_out=p + 128, flags=0, dsize=16, shape=(n, h, w)):
        return lib.mp_crop3d_dev_coms_dt(c, P(frames), dt, *shape, scale, P(coms), flags, dsize, P(p + 256),
                                         P(p + 512), P(coms_out), P(p + 1024), None)

    # the work-size query: float32 forwards, uint16 has its own size, anything else is 0
    assert lib.mp_center_of_mass_dev_work_dt(F32, n, h, w) == lib.mp_center_of_mass_dev_work(n, h, w) > 0
    assert lib.mp_center_of_mass_dev_work_dt(U16, n, h, w) > 0
    assert lib.mp_center_of_mass_dev_work_dt(U16, 1, 424, 512) <= lib.mp_center_of_mass_dev_work_dt(F32, 1, 424, 512)
    assert lib.mp_center_of_mass_dev_work_dt(7, n, h, w) == 0
    assert lib.mp_center_of_mass_dev_work_dt(U16, 0, h, w) == 0
    assert lib.mp_center_of_mass_dev_work_dt(U16, 1, 1 << 15, (1 << 15) + 1) == 0
    for dt in (F32, U16):
        assert com(None, dt, 1.0) == MP_ERR_ARG                      # null pointers
        assert com(p, dt, 1.0, coms=None) == MP_ERR_ARG
        assert com(p, dt, 1.0, work=None) == MP_ERR_ARG
        assert crop(None, dt, 1.0) == MP_ERR_ARG
        assert crop(p, dt, 1.0, coms=None) == MP_ERR_ARG
        assert crop(p, dt, 1.0, coms_out=None) == MP_ERR_ARG
        assert com(p, dt, 1.0, shape=(0, h, w)) == MP_ERR_SHAPE      # the existing shape limits
        assert com(p, dt, 1.0, shape=(65536, h, w)) == MP_ERR_SHAPE
        assert crop(p, dt, 1.0, shape=(n, 1 << 15, (1 << 15) + 1)) == MP_ERR_SHAPE
        assert crop(p, dt, 1.0, dsize=4097) == MP_ERR_SHAPE
        assert com(p, dt, 1.0, nbytes=8) == MP_ERR_ARG               # work buffer too small
        assert crop(p, dt, 1.0, flags=2) == MP_ERR_ARG
        assert crop(p, dt, 1.0, coms=p + 64, coms_out=p + 64) == MP_ERR_ARG
    for bad in (2, 7, -1):                                           # unknown dtype
        assert com(p, bad, 1.0) == MP_ERR_ARG
        assert crop(p, bad, 1.0) == MP_ERR_ARG
    assert com(p, U16, 2.0) == MP_ERR_ARG                            # uint16 frames are millimetres
    assert crop(p, U16, 2.0) == MP_ERR_ARG
    assert com(p, U16, 10000.0) == MP_ERR_ARG
    assert com(p + 1, U16, 1.0) == MP_ERR_ARG                        # an odd address
    assert crop(p + 1, U16, 1.0) == MP_ERR_ARG
    assert b"uint16" in lib.mp_last_error() or b"2-byte" in lib.mp_last_error()


def test_facade_validates_uint16_frames_before_gpu():
    import torch
    mp = pkg()
    md = mp.monkeydetector.MonkeyDetector(*CAM)
    fr = torch.zeros((2, 8, 16), dtype=torch.uint16)
    pipe = mp.train_cnn_networks_hgru.DetectorPosePipeline(object(), md, dsize=64)
    pipe_norm = mp.train_cnn_networks_hgru.DetectorPosePipeline(object(), md, dsize=64, frame_scale=10000.0)
    with pytest.raises(TypeError):                      # a CPU tensor
        md.calculateCoM_device(fr)
    with pytest.raises(TypeError):
        md.detect_crop_device(fr)
    with pytest.raises(TypeError):
        pipe.run(fr)
    with pytest.raises(ValueError):                     # uint16 frames have no normalised form
        md.calculateCoM_device(fr, frame_scale=10000)
    with pytest.raises(ValueError):
        md.detect_crop_device(fr, frame_scale=10000)
    with pytest.raises(ValueError):
        pipe_norm.run(fr)
    with pytest.raises(ValueError):                     # shapes first, as for float32 frames
        md.calculateCoM_device(torch.zeros((2, 8, 16, 3), dtype=torch.uint16))
    # the dtype code travels with the frames; float32 frames are untouched by the scale rule
    with pytest.raises(TypeError):
        md.calculateCoM_device(torch.zeros((2, 8, 16)), frame_scale=10000)
