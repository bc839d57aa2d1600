// PNG files from RGB pictures (include/monkeypose_png.h): the C entry points, and the host encoder --
// png_rule.hpp on one thread, written the plain way (a position's matches by comparing bytes, one
// token after the other, the checksums byte by byte), which is what the kernels of k_png.hip are
// compared with byte for byte.
#include <cstring>
#include <vector>

#include "../../include/monkeypose_png.h"
#include "mp_kernels.hpp"
#include "mp_runtime.hpp"
#include "png_rule.hpp"

using namespace mpr;

namespace {

struct CrcTable {
  uint32_t t[256];
  CrcTable() {
    for (uint32_t i = 0; i < 256; ++i) t[i] = mppng::crc_table_entry(i);
  }
};

uint32_t crc32_of(const uint8_t* p, size_t n) {
  static const CrcTable tab;
  uint32_t c = 0xffffffffu;
  for (size_t i = 0; i < n; ++i) c = tab.t[(c ^ p[i]) & 0xffu] ^ (c >> 8);
  return ~c;
}

void put_be32(uint8_t* p, uint32_t v) {
  p[0] = (uint8_t)(v >> 24);
  p[1] = (uint8_t)(v >> 16);
  p[2] = (uint8_t)(v >> 8);
  p[3] = (uint8_t)v;
}

// length || type || data || crc at p -> the bytes written
size_t put_chunk(uint8_t* p, const char* type, const uint8_t* data, size_t n) {
  put_be32(p, (uint32_t)n);
  std::memcpy(p + 4, type, 4);
  if (n) std::memcpy(p + 8, data, n);
  put_be32(p + 8 + n, crc32_of(p + 4, 4 + n));
  return n + mppng::CHUNK_BYTES;
}

struct BitWriter {
  std::vector<uint8_t>& v;
  uint64_t acc = 0;
  int nb = 0;
  void put(uint32_t val, int n) {
    acc |= (uint64_t)val << nb;
    nb += n;
    while (nb >= 8) {
      v.push_back((uint8_t)acc);
      acc >>= 8;
      nb -= 8;
    }
  }
  void align() {
    if (nb) put(0, 8 - nb);
  }
};

// the deflate bytes of one band a[0 .. len), its empty stored block included, appended to out
void encode_band(const uint8_t* a, int len, int w, bool last, std::vector<uint8_t>& out) {
  int cd[mppng::MAX_CANDS];
  const int nc = mppng::cands(w, cd);
  std::vector<uint8_t> fx;
  fx.reserve((size_t)len + 16);
  BitWriter bw{fx};
  bw.put(mppng::FIXED_HEAD, mppng::BLOCK_HEAD_BITS);
  int64_t token_bits = 0;
  const int stored = mppng::stored_band_bytes(len);
  for (int p = 0; p < len;) {
    int bl = 0, bd = 0;
    for (int c = 0; c < nc; ++c) {
      const int d = cd[c];
      if (d > p) continue;
      int L = 0;
      while (L < mppng::MAX_MATCH && p + L < len && a[p + L] == a[p + L - d]) ++L;
      if (L > bl || (L == bl && d < bd)) bl = L, bd = d;
    }
    int n;
    uint32_t v;
    if (bl >= mppng::MIN_MATCH) {
      v = mppng::match_code(bl, bd, &n);
      p += bl;
    } else {
      v = mppng::fixed_code(a[p], &n);
      p += 1;
    }
    token_bits += n;
    // a band the stored form already beats needs no more of its fixed form
    if (mppng::fixed_band_bytes(token_bits) > stored) break;
    bw.put(v, n);
  }
  if (mppng::fixed_band_bytes(token_bits) <= stored) {
    int n;
    const uint32_t eob = mppng::fixed_code(256, &n);
    bw.put(eob, n);
    bw.put(last ? 1u : 0u, mppng::BLOCK_HEAD_BITS);
    bw.align();
    out.insert(out.end(), fx.begin(), fx.end());
  } else {
    const uint8_t head[5] = {0, (uint8_t)len, (uint8_t)(len >> 8), (uint8_t)~len, (uint8_t)(~len >> 8)};
    out.insert(out.end(), head, head + 5);
    out.insert(out.end(), a, a + len);
    out.push_back(last ? 1 : 0);
  }
  const uint8_t empty[4] = {0, 0, 0xff, 0xff};
  out.insert(out.end(), empty, empty + 4);
}

size_t encode_image(const uint8_t* rgb, int h, int w, uint8_t* out) {
  static const uint8_t sig[8] = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1a, '\n'};
  uint8_t* p = out;
  std::memcpy(p, sig, 8);
  p += 8;
  uint8_t ihdr[13];
  put_be32(ihdr, (uint32_t)w);
  put_be32(ihdr + 4, (uint32_t)h);
  ihdr[8] = 8, ihdr[9] = 2, ihdr[10] = 0, ihdr[11] = 0, ihdr[12] = 0;
  p += put_chunk(p, "IHDR", ihdr, 13);

  const int rb = mppng::row_bytes(w), rows = mppng::band_rows(w), nb = mppng::band_count(h, w);
  std::vector<uint8_t> raw((size_t)rows * rb), data;
  uint32_t A = 1, B = 0;
  for (int k = 0; k < nb; ++k) {
    const int len = mppng::band_len(h, w, k);
    for (int r = 0; r < len / rb; ++r) {
      raw[(size_t)r * rb] = 0;
      std::memcpy(&raw[(size_t)r * rb + 1], rgb + ((size_t)k * rows + r) * 3 * w, (size_t)3 * w);
    }
    for (int i = 0; i < len; ++i) {
      A = (A + raw[i]) % mppng::ADLER_MOD;
      B = (B + A) % mppng::ADLER_MOD;
    }
    data.clear();
    if (k == 0) data.push_back(0x78), data.push_back(0x01);
    encode_band(raw.data(), len, w, k == nb - 1, data);
    p += put_chunk(p, "IDAT", data.data(), data.size());
  }
  uint8_t ad[4];
  put_be32(ad, (B << 16) | A);
  p += put_chunk(p, "IDAT", ad, 4);
  p += put_chunk(p, "IEND", nullptr, 0);
  return (size_t)(p - out);
}

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
      const size_t sz = encode_image(rgb + (size_t)i * h * w * 3, (int)h, (int)w, file.data());
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
