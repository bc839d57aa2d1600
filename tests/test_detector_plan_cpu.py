"""CPU: the device calculateCoM's split plan (monkey-pose_amd/csrc/com_plan.hpp), evaluated by a
small host program that includes the very header the kernels include, equals numpy 1.x's float32
pairwise sum (oracle.crop_ref.np_pairwise_sum_f32) bit for bit; the header declares the detector's
device entry points, the ctypes tables list them, the library exports them, and the façade rejects
bad input before any GPU call."""
import os
import re
import subprocess

import numpy as np
import pytest

from helpers import ROOT, pkg
from oracle import crop_ref as CR

CSRC = os.path.join(ROOT, "monkey-pose_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "monkeypose.h")
NEW_FUNCS = ("mp_center_of_mass_dev_work", "mp_center_of_mass_dev", "mp_crop3d_dev_coms", "mp_abs_joints_dev")
SIZES = (1, 5, 8, 127, 128, 129, 136, 1961, 33300, 217088)
CAM = (365.456, 365.456, 256, 212, [800, 800, 1200], 200, 10000)

PLAN_MAIN = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "com_plan.hpp"

// usage: plan sum FILE n...   -> one line "n bits" per n: the plan's sum of the file's first n floats
//        plan check NMAX      -> walks the plan of every n <= NMAX and checks its size claims
static int check(int64_t n) {
  using namespace complan;
  const int D = depth_for(n, CHUNK_CAP);
  int64_t covered = 0;
  for (int64_t c = 0; c < ((int64_t)1 << D); ++c) {
    int64_t lo = 0, m = n;
    for (int b = D - 1; b >= 0; --b) {            // every node above a chunk is an internal node
      if (m <= LEAF) return 1;
      const int64_t n2 = left_len(m);
      if ((c >> b) & 1) { lo += n2; m -= n2; } else { m = n2; }
    }
    if (lo != covered || m < 1 || m > CHUNK_CAP || lo % 8) return 2;
    covered += m;
    const int E = depth_for(m, GROUP_CAP);
    if (((int64_t)1 << E) > MAX_GROUPS) return 3;
    int64_t gcov = 0;
    for (int64_t p = 0; p < ((int64_t)1 << E); ++p) {
      int64_t glo = 0, gm = m;
      for (int b = E - 1; b >= 0; --b) {
        if (gm <= LEAF) return 4;
        const int64_t n2 = left_len(gm);
        if ((p >> b) & 1) { glo += n2; gm -= n2; } else { gm = n2; }
      }
      if (glo != gcov || gm < 1 || gm > GROUP_CAP) return 5;
      int64_t llo[3], llen[3];
      const int nl = group_leaves(glo, gm, llo, llen);
      int64_t lcov = glo;
      for (int k = 0; k < nl; ++k) {
        if (llo[k] != lcov || llen[k] < 1 || llen[k] > LEAF || llo[k] % 8) return 6;
        if (llen[k] < 8 && n >= 8) return 7;
        lcov += llen[k];
      }
      if (lcov != glo + gm) return 8;
      if ((nl == 1) != (gm <= LEAF)) return 9;
      gcov += gm;
    }
    if (gcov != m) return 10;
  }
  return covered == n ? 0 : 11;
}

int main(int argc, char** argv) {
  if (argc >= 3 && !std::strcmp(argv[1], "check")) {
    const int64_t nmax = std::atoll(argv[2]);
    for (int64_t n = 1; n <= nmax; ++n) {
      const int rc = check(n);
      if (rc) { std::printf("n=%lld rule %d\n", (long long)n, rc); return 1; }
    }
    for (int64_t n = nmax; n <= ((int64_t)1 << 30); n = n * 3 / 2 + 5) {
      const int rc = check(n);
      if (rc) { std::printf("n=%lld rule %d\n", (long long)n, rc); return 1; }
    }
    std::printf("ok\n");
    return 0;
  }
  if (argc < 4 || std::strcmp(argv[1], "sum")) return 2;
  std::FILE* f = std::fopen(argv[2], "rb");
  if (!f) return 3;
  std::fseek(f, 0, SEEK_END);
  const long bytes = std::ftell(f);
  std::fseek(f, 0, SEEK_SET);
  std::vector<float> a((size_t)bytes / 4);
  if (std::fread(a.data(), 4, a.size(), f) != a.size()) return 4;
  std::fclose(f);
  for (int i = 3; i < argc; ++i) {
    const int64_t n = std::atoll(argv[i]);
    if (n < 1 || n > (int64_t)a.size()) return 5;
    std::vector<float> parts((size_t)1 << complan::depth_for(n, complan::CHUNK_CAP));
    const float s = complan::eval_host(a.data(), n, parts.data());
    uint32_t bits;
    std::memcpy(&bits, &s, 4);
    std::printf("%lld %08x\n", (long long)n, bits);
  }
  return 0;
}
"""


@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("plan")
    src = d / "plan_main.cpp"
    src.write_text(PLAN_MAIN)
    exe = d / "plan"
    p = subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-I", CSRC, str(src),
                        "-o", str(exe)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    return str(exe)


def _thresholded_frame():
    """dc of calculateCoM for a synthetic 424 x 512 frame in whole millimetres (217088 elements)"""
    fr = CR.synth_frame(5)
    dc = fr.copy()
    dc[dc < np.float32(200)] = 0
    dc[dc > np.float32(10000)] = 0
    return dc.reshape(-1)


@pytest.mark.parametrize("scale", [1.0, 0.37], ids=["integer_mm", "fractional"])
def test_plan_equals_numpy_pairwise_sum(plan_exe, tmp_path, scale):
    a = (_thresholded_frame() * np.float32(scale)).astype(np.float32)
    assert a.size == 217088
    path = tmp_path / "a.bin"
    a.tofile(path)
    p = subprocess.run([plan_exe, "sum", str(path)] + [str(n) for n in SIZES], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    got = {int(l.split()[0]): int(l.split()[1], 16) for l in p.stdout.splitlines()}
    for n in SIZES:
        ref = CR.np_pairwise_sum_f32(a[:n])
        assert got[n] == int(np.float32(ref).view(np.uint32)), (n, scale)
    # the order is observable on this data: the float64 sum of the full frame differs
    assert float(CR.np_pairwise_sum_f32(a)) != float(a.astype(np.float64).sum())


def test_plan_size_claims_hold(plan_exe):
    """every n up to 70000 and a geometric sweep up to 2^30: chunks tile the frame, fit the LDS tile,
    sit below internal nodes only, and every group is one to three leaves"""
    p = subprocess.run([plan_exe, "check", "70000"], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.strip() == "ok", p.stdout + p.stderr


def _header_functions():
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return set(re.findall(r"\b(mp_[a-z0-9_]+)\s*\(", txt))


def test_header_tables_and_library_list_the_detector_calls():
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


def test_detector_facade_validates_before_gpu():
    import torch
    mp = pkg()
    md = mp.monkeydetector.MonkeyDetector(*CAM)
    fr = torch.zeros((2, 8, 16))
    with pytest.raises(TypeError):
        md.calculateCoM_device(fr)
    with pytest.raises(TypeError):
        md.detect_crop_device(fr)
    with pytest.raises(TypeError):
        md.getAbsoluteCoordinates_device(torch.zeros((2, 69)), torch.zeros((2, 3), dtype=torch.float64))
    pipe = mp.train_cnn_networks_hgru.DetectorPosePipeline(object(), md, dsize=64)
    with pytest.raises(TypeError):
        pipe.run(fr)
    # shapes are checked first, so a bad shape is a ValueError whatever the device
    with pytest.raises(ValueError):
        md.calculateCoM_device(torch.zeros((2, 8, 16, 3)))
    with pytest.raises(ValueError):
        md.detect_crop_device(torch.zeros((8, 16)))
    with pytest.raises(ValueError):
        md.detect_crop_device(fr, coms=torch.zeros((3, 3), dtype=torch.float64))
    with pytest.raises(ValueError):
        md.getAbsoluteCoordinates_device(torch.zeros((2, 68)), torch.zeros((2, 3), dtype=torch.float64))
    with pytest.raises(ValueError):
        md.getAbsoluteCoordinates_device(torch.zeros((2, 69)), torch.zeros((3, 3), dtype=torch.float64))
    with pytest.raises(ValueError):
        pipe.run(torch.zeros((8, 16)))
