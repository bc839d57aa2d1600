// What the host PNG encoders share (png_rgb_host.hpp, png16_host.hpp): chunks and checksums, the bit
// writer, the greedy match search of png_rule.hpp, the stored and the empty block, and the file's
// frame -- signature, IHDR, one IDAT per band with the running Adler-32, the Adler-32's IDAT, IEND.
// One thread, written the plain way: a position's matches by comparing bytes, the checksums byte by
// byte.  Plain C++ (no HIP), so that a host program builds it with the sanitizers.
#pragma once
#include <cstring>
#include <vector>

#include "png_rule.hpp"

namespace mppngh {

struct CrcTable {
  uint32_t t[256];
  CrcTable() {
    for (uint32_t i = 0; i < 256; ++i) t[i] = mppng::crc_table_entry(i);
  }
};

inline uint32_t crc32_of(const uint8_t* p, size_t n) {
  static const CrcTable tab;
  uint32_t c = 0xffffffffu;
  for (size_t i = 0; i < n; ++i) c = tab.t[(c ^ p[i]) & 0xffu] ^ (c >> 8);
  return ~c;
}

inline void put_be32(uint8_t* p, uint32_t v) {
  p[0] = (uint8_t)(v >> 24);
  p[1] = (uint8_t)(v >> 16);
  p[2] = (uint8_t)(v >> 8);
  p[3] = (uint8_t)v;
}

// length || type || data || crc at p -> the bytes written
inline size_t put_chunk(uint8_t* p, const char* type, const uint8_t* data, size_t n) {
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
  void put(uint32_t val, int n) {     // n <= 32
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

struct Match {
  int len, dist;
};
// the rule's match at position p of the band a[0 .. len): the longest among the nc distances cd, ties to
// the smallest distance; len below MIN_MATCH means the literal a[p]
inline Match best_match(const uint8_t* a, int len, int p, const int* cd, int nc) {
  Match m{0, 0};
  for (int c = 0; c < nc; ++c) {
    const int d = cd[c];
    if (d > p) continue;
    int L = 0;
    while (L < mppng::MAX_MATCH && p + L < len && a[p + L] == a[p + L - d]) ++L;
    if (L > m.len || (L == m.len && d < m.dist)) m = {L, d};
  }
  return m;
}

// the band as one stored block
inline void put_stored_block(std::vector<uint8_t>& out, const uint8_t* a, int len, bool last) {
  const uint8_t head[5] = {0, (uint8_t)len, (uint8_t)(len >> 8), (uint8_t)~len, (uint8_t)(~len >> 8)};
  out.insert(out.end(), head, head + 5);
  out.insert(out.end(), a, a + len);
  out.push_back(last ? 1 : 0);
}

// the separator after a band's block: LEN 0000, NLEN ffff of the empty stored block whose header came before
inline void put_empty_block(std::vector<uint8_t>& out) {
  const uint8_t empty[4] = {0, 0, 0xff, 0xff};
  out.insert(out.end(), empty, empty + 4);
}

// One h x w file at out (the format's bound(h, w) bytes are enough) -> its size.  F states the format:
// the IHDR's BIT_DEPTH and COLOUR_TYPE and the rule's row_bytes, band_rows, band_count and band_len.
// fill(k, r0, nr, raw) writes band k's raw rows [r0, r0 + nr), filter bytes included;
// encode(k, raw, len, last, data) appends the band's deflate bytes, its empty block included.
template <class F, class Fill, class Encode>
size_t encode_file(int h, int w, uint8_t* out, Fill fill, Encode encode) {
  static const uint8_t sig[8] = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1a, '\n'};
  uint8_t* p = out;
  std::memcpy(p, sig, 8);
  p += 8;
  uint8_t ihdr[13];
  put_be32(ihdr, (uint32_t)w);
  put_be32(ihdr + 4, (uint32_t)h);
  ihdr[8] = F::BIT_DEPTH, ihdr[9] = F::COLOUR_TYPE, ihdr[10] = 0, ihdr[11] = 0, ihdr[12] = 0;
  p += put_chunk(p, "IHDR", ihdr, 13);

  const int rb = F::row_bytes(w), rows = F::band_rows(w), nb = F::band_count(h, w);
  std::vector<uint8_t> raw((size_t)rows * rb), data;
  uint32_t A = 1, B = 0;
  for (int k = 0; k < nb; ++k) {
    const int len = F::band_len(h, w, k);
    fill(k, k * rows, len / rb, raw.data());
    for (int i = 0; i < len; ++i) {
      A = (A + raw[i]) % mppng::ADLER_MOD;
      B = (B + A) % mppng::ADLER_MOD;
    }
    data.clear();
    if (k == 0) data.push_back(0x78), data.push_back(0x01);
    encode(k, raw.data(), len, k == nb - 1, data);
    p += put_chunk(p, "IDAT", data.data(), data.size());
  }
  uint8_t ad[4];
  put_be32(ad, (B << 16) | A);
  p += put_chunk(p, "IDAT", ad, 4);
  p += put_chunk(p, "IEND", nullptr, 0);
  return (size_t)(p - out);
}

}  // namespace mppngh
