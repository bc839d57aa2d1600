// The host encoder of png_rule.hpp on png_host.hpp's frame: rows with the filter byte 0, and a band as
// one fixed-Huffman block or one stored block.  mp_png.hip wraps it for the library, and the kernels of
// k_png.hip are compared with it byte for byte.  Plain C++ (no HIP).
#pragma once
#include "png_host.hpp"

namespace mppngh {

// the RGB format, for the file's frame on the host and on the device
struct Rgb8 {
  static constexpr int BIT_DEPTH = 8, COLOUR_TYPE = 2;
  MP_PNG_HD static constexpr int row_bytes(int w) { return mppng::row_bytes(w); }
  static constexpr int band_rows(int w) { return mppng::band_rows(w); }
  static constexpr int band_count(int h, int w) { return mppng::band_count(h, w); }
  static constexpr int band_len(int h, int w, int k) { return mppng::band_len(h, w, k); }
};

// the deflate bytes of one band a[0 .. len), its empty stored block included, appended to out
inline void encode_rgb_band(const uint8_t* a, int len, int w, bool last, std::vector<uint8_t>& out) {
  int cd[mppng::MAX_CANDS];
  const int nc = mppng::cands(w, cd);
  std::vector<uint8_t> fx;
  fx.reserve((size_t)len + 16);
  BitWriter bw{fx};
  bw.put(mppng::FIXED_HEAD, mppng::BLOCK_HEAD_BITS);
  int64_t token_bits = 0;
  for (int p = 0; p < len;) {
    const Match m = best_match(a, len, p, cd, nc);
    const bool is_match = m.len >= mppng::MIN_MATCH;
    int n;
    const uint32_t v = is_match ? mppng::match_code(m.len, m.dist, &n) : mppng::fixed_code(a[p], &n);
    bw.put(v, n);
    token_bits += n;
    p += is_match ? m.len : 1;
  }
  if (mppng::fixed_band_bytes(token_bits) <= mppng::stored_band_bytes(len)) {
    int n;
    const uint32_t eob = mppng::fixed_code(256, &n);
    bw.put(eob, n);
    bw.put(last ? 1u : 0u, mppng::BLOCK_HEAD_BITS);
    bw.align();
    out.insert(out.end(), fx.begin(), fx.end());
  } else {
    put_stored_block(out, a, len, last);
  }
  put_empty_block(out);
}

// one picture [h][w][3] -> its file at out (mppng::bound(h, w) bytes are enough)
inline size_t encode_rgb_image(const uint8_t* rgb, int h, int w, uint8_t* out) {
  const int rb = mppng::row_bytes(w);
  return encode_file<Rgb8>(
      h, w, out,
      [&](int, int r0, int nr, uint8_t* raw) {
        for (int r = 0; r < nr; ++r) {
          raw[(size_t)r * rb] = 0;
          std::memcpy(&raw[(size_t)r * rb + 1], rgb + (size_t)(r0 + r) * 3 * w, (size_t)3 * w);
        }
      },
      [&](int, const uint8_t* a, int len, bool last, std::vector<uint8_t>& data) { encode_rgb_band(a, len, w, last, data); });
}

}  // namespace mppngh
