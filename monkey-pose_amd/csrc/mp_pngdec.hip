// PNG files to pixels (include/monkeypose_pngdec.h): the C entry points, and the host decoder --
// pngdec_rule.hpp on one thread through its plain policies (bytes one after the other, the
// checksums byte by byte), which is what the kernels of k_pngdec.hip are compared with bit for bit.
#include <vector>

#include "../../include/monkeypose_pngdec.h"
#include "mp_kernels.hpp"
#include "mp_runtime.hpp"
#include "pngdec_rule.hpp"

using namespace mpr;

namespace {

bool shape_ok(int64_t n, int64_t h, int64_t w, int format, int64_t file_stride) {
  return n >= 1 && n <= mppd::MAX_N && h >= 1 && h <= mppd::MAX_HW && w >= 1 && w <= mppd::MAX_HW &&
         mppd::format_ok(format) && file_stride >= 1 && file_stride <= mppd::MAX_STRIDE;
}

void check_call(const char* who, const void* files, int64_t file_stride, const void* sizes, int64_t n, int64_t h,
                int64_t w, int format, const void* out, const void* status) {
  if (!files || !sizes || !out || !status) fail(MP_ERR_ARG, std::string(who) + ": null pointer");
  if (!shape_ok(n, h, w, format, file_stride))
    fail(MP_ERR_SHAPE, std::string(who) + ": bad shape (1 <= n <= 65535, 1 <= h, w <= 4096, format 0 .. 2, "
                                          "1 <= file_stride <= 2^30)");
  if (reinterpret_cast<uintptr_t>(sizes) & 7) fail(MP_ERR_ARG, std::string(who) + ": sizes must be 8-byte aligned");
  if (reinterpret_cast<uintptr_t>(status) & 3) fail(MP_ERR_ARG, std::string(who) + ": status must be 4-byte aligned");
  if (format == MP_PNG_GRAY16 && (reinterpret_cast<uintptr_t>(out) & 1))
    fail(MP_ERR_ARG, std::string(who) + ": out must be 2-byte aligned for MP_PNG_GRAY16");
}

}  // namespace

extern "C" {

size_t mp_png_decode_work_bytes(int64_t n, int64_t h, int64_t w, int format, int64_t file_stride) {
  return shape_ok(n, h, w, format, file_stride) ? mp::pngdec_work_bytes(n, (int)h, (int)w, format, file_stride) : 0;
}

int mp_png_decode_host(const uint8_t* files, int64_t file_stride, const int64_t* sizes, int64_t n, int64_t h, int64_t w,
                       int format, void* out, int32_t* status) {
  return guard([&] {
    check_call("mp_png_decode_host", files, file_stride, sizes, n, h, w, format, out, status);
    const size_t image = (size_t)h * mppd::row_bytes((int)w, format);
    std::vector<uint8_t> z((size_t)file_stride), raw((size_t)mppd::raw_bytes((int)h, (int)w, format));
    for (int64_t i = 0; i < n; ++i) {
      // a size the call does not allow is an empty file: nothing of it is read
      const int64_t size = (sizes[i] < 0 || sizes[i] > file_stride) ? 0 : sizes[i];
      status[i] = mppd::decode_file_host(files + (size_t)i * file_stride, size, (int)h, (int)w, format, z.data(),
                                         raw.data(), static_cast<uint8_t*>(out) + (size_t)i * image);
    }
  });
}

int mp_png_decode_dev(const uint8_t* files, int64_t file_stride, const int64_t* sizes, int64_t n, int64_t h, int64_t w,
                      int format, void* out, int32_t* status, void* work, void* stream) {
  return guard([&] {
    check_call("mp_png_decode_dev", files, file_stride, sizes, n, h, w, format, out, status);
    if (!work) fail(MP_ERR_ARG, "mp_png_decode_dev: null pointer");
    if (reinterpret_cast<uintptr_t>(work) & 15) fail(MP_ERR_ARG, "mp_png_decode_dev: work must be 16-byte aligned");
    hip_check(mp::launch_png_decode(files, file_stride, sizes, n, (int)h, (int)w, format, out, status, work,
                                    static_cast<hipStream_t>(stream)),
              "png_decode");
  });
}

}  // extern "C"
