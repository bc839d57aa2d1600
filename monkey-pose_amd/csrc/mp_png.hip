// PNG files from RGB pictures (include/monkeypose_png.h): the C entry points.  The host encoder is
// png_rgb_host.hpp -- png_rule.hpp on one thread -- which is what the kernels of k_png.hip are compared
// with byte for byte.
#include <cstring>
#include <vector>

#include "../../include/monkeypose_png.h"
#include "mp_kernels.hpp"
#include "mp_runtime.hpp"
#include "png_rgb_host.hpp"

using namespace mpr;

namespace {

bool shape_ok(int64_t h, int64_t w) { return h >= 1 && w >= 1 && h <= mppng::MAX_HW && w <= mppng::MAX_HW; }

void check_call(const char* who, const void* rgb, int64_t n, int64_t h, int64_t w, const void* out, int64_t out_stride,
                const void* sizes) {
  if (!rgb || !out || !sizes) fail(MP_ERR_ARG, std::string(who) + ": null pointer");
  if (n < 1 || n > mppng::MAX_N || !shape_ok(h, w))
    fail(MP_ERR_SHAPE, std::string(who) + ": bad shape (1 <= n <= 65535, 1 <= h, w <= 4096)");
  if (out_stride < mppng::bound((int)h, (int)w))
    fail(MP_ERR_SHAPE, std::string(who) + ": out_stride is below mp_png_bound(h, w)");
  if (reinterpret_cast<uintptr_t>(sizes) & 7) fail(MP_ERR_ARG, std::string(who) + ": sizes must be 8-byte aligned");
}

}  // namespace

extern "C" {

size_t mp_png_bound(int64_t h, int64_t w) { return shape_ok(h, w) ? (size_t)mppng::bound((int)h, (int)w) : 0; }

size_t mp_png_work_bytes(int64_t n, int64_t h, int64_t w) {
  return (n >= 1 && n <= mppng::MAX_N && shape_ok(h, w)) ? mp::png_work_bytes(n, (int)h, (int)w) : 0;
}

int mp_png_band_rows(int64_t w) { return (w >= 1 && w <= mppng::MAX_HW) ? mppng::band_rows((int)w) : 0; }

int mp_png_band_count(int64_t h, int64_t w) { return shape_ok(h, w) ? mppng::band_count((int)h, (int)w) : 0; }

int mp_png_encode_host(const uint8_t* rgb, int64_t n, int64_t h, int64_t w, uint8_t* out, int64_t out_stride,
                       int64_t* sizes) {
  return guard([&] {
    check_call("mp_png_encode_host", rgb, n, h, w, out, out_stride, sizes);
    std::vector<uint8_t> file((size_t)mppng::bound((int)h, (int)w));
    for (int64_t i = 0; i < n; ++i) {
      const size_t sz = mppngh::encode_rgb_image(rgb + (size_t)i * h * w * 3, (int)h, (int)w, file.data());
      std::memcpy(out + (size_t)i * out_stride, file.data(), sz);
      sizes[i] = (int64_t)sz;
    }
  });
}

int mp_png_encode_dev(const uint8_t* rgb, int64_t n, int64_t h, int64_t w, uint8_t* out, int64_t out_stride,
                      int64_t* sizes, void* work, void* stream) {
  return guard([&] {
    check_call("mp_png_encode_dev", rgb, n, h, w, out, out_stride, sizes);
    if (!work) fail(MP_ERR_ARG, "mp_png_encode_dev: null pointer");
    if (reinterpret_cast<uintptr_t>(work) & 15) fail(MP_ERR_ARG, "mp_png_encode_dev: work must be 16-byte aligned");
    hip_check(mp::launch_png_encode(rgb, n, (int)h, (int)w, out, out_stride, sizes, work,
                                    static_cast<hipStream_t>(stream)),
              "png_encode");
  });
}

}  // extern "C"
