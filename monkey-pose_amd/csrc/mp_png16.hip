// PNG files from 16-bit depth frames (include/monkeypose_png16.h): the C entry points.  The host
// encoder is png16_host.hpp -- png16_rule.hpp on one thread -- which is what the kernels of
// k_png16.hip are compared with byte for byte.
#include <cstring>
#include <vector>

#include "../../include/monkeypose_png16.h"
#include "mp_kernels.hpp"
#include "mp_runtime.hpp"
#include "png16_host.hpp"

using namespace mpr;

static_assert(MP_PNG16_STAT_INTS == mppng16h::STAT_INTS, "the header's stats row is the host encoder's");

namespace {

bool shape_ok(int64_t h, int64_t w) { return h >= 1 && w >= 1 && h <= mppng16::MAX_HW && w <= mppng16::MAX_HW; }

void check_frames(const char* who, const void* frames, int64_t n, int64_t h, int64_t w) {
  if (!frames) fail(MP_ERR_ARG, std::string(who) + ": null pointer");
  if (n < 1 || n > mppng16::MAX_N || !shape_ok(h, w))
    fail(MP_ERR_SHAPE, std::string(who) + ": bad shape (1 <= n <= 65535, 1 <= h, w <= 4096)");
  if (reinterpret_cast<uintptr_t>(frames) & 1) fail(MP_ERR_ARG, std::string(who) + ": frames must be 2-byte aligned");
}

void check_call(const char* who, const void* frames, int64_t n, int64_t h, int64_t w, const void* out,
                int64_t out_stride, const void* sizes) {
  if (!out || !sizes) fail(MP_ERR_ARG, std::string(who) + ": null pointer");
  check_frames(who, frames, n, h, w);
  if (out_stride < mppng16::bound((int)h, (int)w))
    fail(MP_ERR_SHAPE, std::string(who) + ": out_stride is below mp_png16_bound(h, w)");
  if (reinterpret_cast<uintptr_t>(sizes) & 7) fail(MP_ERR_ARG, std::string(who) + ": sizes must be 8-byte aligned");
}

}  // namespace

extern "C" {

size_t mp_png16_bound(int64_t h, int64_t w) { return shape_ok(h, w) ? (size_t)mppng16::bound((int)h, (int)w) : 0; }

size_t mp_png16_work_bytes(int64_t n, int64_t h, int64_t w) {
  return (n >= 1 && n <= mppng16::MAX_N && shape_ok(h, w)) ? mp::png16_work_bytes(n, (int)h, (int)w) : 0;
}

int mp_png16_band_rows(int64_t w) { return (w >= 1 && w <= mppng16::MAX_HW) ? mppng16::band_rows((int)w) : 0; }

int mp_png16_band_count(int64_t h, int64_t w) { return shape_ok(h, w) ? mppng16::band_count((int)h, (int)w) : 0; }

int mp_png16_encode_host(const uint16_t* frames, int64_t n, int64_t h, int64_t w, uint8_t* out, int64_t out_stride,
                         int64_t* sizes) {
  return guard([&] {
    check_call("mp_png16_encode_host", frames, n, h, w, out, out_stride, sizes);
    std::vector<uint8_t> file((size_t)mppng16::bound((int)h, (int)w));
    for (int64_t i = 0; i < n; ++i) {
      const size_t sz = mppng16h::encode_image(frames + (size_t)i * h * w, (int)h, (int)w, file.data(), nullptr);
      std::memcpy(out + (size_t)i * out_stride, file.data(), sz);
      sizes[i] = (int64_t)sz;
    }
  });
}

int mp_png16_band_stats_host(const uint16_t* frames, int64_t n, int64_t h, int64_t w, int32_t* stats) {
  return guard([&] {
    if (!stats) fail(MP_ERR_ARG, "mp_png16_band_stats_host: null pointer");
    check_frames("mp_png16_band_stats_host", frames, n, h, w);
    if (reinterpret_cast<uintptr_t>(stats) & 3) fail(MP_ERR_ARG, "mp_png16_band_stats_host: stats must be 4-byte aligned");
    const int nb = mppng16::band_count((int)h, (int)w);
    std::vector<uint8_t> file((size_t)mppng16::bound((int)h, (int)w));
    std::vector<mppng16h::BandStats> st((size_t)nb);
    for (int64_t i = 0; i < n; ++i) {
      (void)mppng16h::encode_image(frames + (size_t)i * h * w, (int)h, (int)w, file.data(), st.data());
      std::memcpy(stats + (size_t)i * nb * MP_PNG16_STAT_INTS, st.data(), (size_t)nb * sizeof st[0]);
    }
  });
}

int mp_png16_encode_dev(const uint16_t* frames, int64_t n, int64_t h, int64_t w, uint8_t* out, int64_t out_stride,
                        int64_t* sizes, void* work, void* stream) {
  return guard([&] {
    check_call("mp_png16_encode_dev", frames, n, h, w, out, out_stride, sizes);
    if (!work) fail(MP_ERR_ARG, "mp_png16_encode_dev: null pointer");
    if (reinterpret_cast<uintptr_t>(work) & 15) fail(MP_ERR_ARG, "mp_png16_encode_dev: work must be 16-byte aligned");
    hip_check(mp::launch_png16_encode(frames, n, (int)h, (int)w, out, out_stride, sizes, work,
                                      static_cast<hipStream_t>(stream)),
              "png16_encode");
  });
}

}  // extern "C"
