// The byte rule of a PNG file written by mp_png_encode_host / mp_png_encode_dev, stated once for the
// host encoder (mp_png.hip), the kernels (k_png.hip) and the size bound.  It fixes every byte of the
// file, so the device's bytes are compared with the host's, not merely decoded.
//
// File        signature, IHDR (8-bit RGB, no interlace), one IDAT per band, one IDAT holding the
//             Adler-32, IEND.  Band 0's IDAT starts with the zlib header 78 01.
// Rows        filter byte 0, then 3 * w bytes (write_png's rows); the raw stream is h such rows.
// Bands       band_rows(w) = max(1, BAND_BYTES / (1 + 3 w)) whole rows each, the last one what is
//             left.  A band is compressed from that band alone: no match crosses a band.
// A band      one fixed-Huffman block (BTYPE 01, RFC 1951 3.2.6) or one stored block (BTYPE 00),
//             whichever is shorter, ties to fixed; then an empty stored block, which brings the stream
//             to a byte boundary (pigz's separator); the last band's empty block carries BFINAL.
// Tokens      greedy, left to right.  At position p, for every distance d of cands(w) with d <= p,
//             L_d = the longest L <= 258 with a[p + j] == a[p + j - d] for j < L and p + L <= band
//             length.  The longest wins, ties to the smallest d.  L >= 3: the match (L, d), advance L;
//             else the literal a[p], advance 1.
// Adler-32    of the whole raw stream, from per-band sums: a band of n bytes with s1 = sum a[i] and
//             s2 = sum (n - i) a[i] takes (A, B) to (A + s1, B + n A + s2) mod 65521.
// CRC-32      every chunk's own, over its type and data.
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MP_PNG_HD __host__ __device__
#else
#define MP_PNG_HD
#endif

#include <cstdint>

namespace mppng {

constexpr int MAX_HW = 4096;         // h, w (the overlay's limits)
constexpr int MAX_N = 65535;
constexpr int BAND_BYTES = 8192;     // part of the format: a band and its per-position state fit in LDS
constexpr int MIN_MATCH = 3, MAX_MATCH = 258;
constexpr int MAX_CANDS = 6;
constexpr uint32_t ADLER_MOD = 65521u;
constexpr uint32_t CRC_POLY = 0xedb88320u;   // reflected

MP_PNG_HD constexpr int row_bytes(int w) { return 1 + 3 * w; }
MP_PNG_HD constexpr int band_rows(int w) { return BAND_BYTES / row_bytes(w) > 1 ? BAND_BYTES / row_bytes(w) : 1; }
MP_PNG_HD constexpr int band_count(int h, int w) { return (h + band_rows(w) - 1) / band_rows(w); }
// raw bytes of band k
MP_PNG_HD constexpr int band_len(int h, int w, int k) {
  return (h - k * band_rows(w) < band_rows(w) ? h - k * band_rows(w) : band_rows(w)) * row_bytes(w);
}
// the longest band of any shape: several rows stay within BAND_BYTES, one row is at most 1 + 3 * 4096
constexpr int MAX_BAND = row_bytes(MAX_HW) > BAND_BYTES ? row_bytes(MAX_HW) : BAND_BYTES;
static_assert(MAX_BAND <= 65535, "a band is one stored block");

// the candidate distances: a run, the two previous pixels, the pixel above and its two neighbours.
// Not sorted, and 1 + 3 w - 3 repeats 1 at w = 1: a tie goes to the smallest distance by value, so
// neither matters.  All are at most 1 + 3 * 4096 + 3, inside the 32 KiB window.
MP_PNG_HD inline int cands(int w, int d[MAX_CANDS]) {
  d[0] = 1;
  d[1] = 3;
  d[2] = 6;
  d[3] = row_bytes(w) - 3;
  d[4] = row_bytes(w);
  d[5] = row_bytes(w) + 3;
  return MAX_CANDS;
}

// ---- the bit stream (LSB first; Huffman codes enter reversed) ----------------------------------
MP_PNG_HD inline uint32_t rev_bits(uint32_t v, int n) {   // n <= 16
  v = ((v & 0x5555u) << 1) | ((v >> 1) & 0x5555u);
  v = ((v & 0x3333u) << 2) | ((v >> 2) & 0x3333u);
  v = ((v & 0x0f0fu) << 4) | ((v >> 4) & 0x0f0fu);
  v = ((v & 0x00ffu) << 8) | ((v >> 8) & 0x00ffu);
  return v >> (16 - n);
}
MP_PNG_HD inline int floor_log2(uint32_t x) { return 31 - __builtin_clz(x); }   // x > 0

// a literal / length symbol 0..287 in the fixed code -> reversed code, *n its length
MP_PNG_HD inline uint32_t fixed_code(int sym, int* n) {
  if (sym < 144) { *n = 8; return rev_bits(0x30u + sym, 8); }
  if (sym < 256) { *n = 9; return rev_bits(0x190u + (sym - 144), 9); }
  if (sym < 280) { *n = 7; return rev_bits((uint32_t)(sym - 256), 7); }
  *n = 8;
  return rev_bits(0xc0u + (sym - 280), 8);
}
MP_PNG_HD inline int literal_bits(int v) { return v < 144 ? 8 : 9; }

// the bits of a match (L in 3..258, d in 1..32768) -> value, *n its length (at most 31)
MP_PNG_HD inline uint32_t match_code(int L, int d, int* n) {
  int sym, le = 0;
  uint32_t lx = 0;
  const uint32_t x = (uint32_t)(L - 3);
  if (x < 8) sym = 257 + (int)x;
  else if (L == MAX_MATCH) sym = 285;
  else {
    le = floor_log2(x) - 2;
    sym = 261 + 4 * le + (int)((x >> le) & 3u);
    lx = x & ((1u << le) - 1u);
  }
  int nb;
  uint32_t v = fixed_code(sym, &nb);
  v |= lx << nb;
  nb += le;
  const uint32_t dd = (uint32_t)(d - 1);
  int dc, de = 0;
  uint32_t dx = 0;
  if (dd < 4) dc = (int)dd;
  else {
    de = floor_log2(dd) - 1;
    dc = 2 * de + 2 + (int)((dd >> de) & 1u);
    dx = dd & ((1u << de) - 1u);
  }
  v |= rev_bits((uint32_t)dc, 5) << nb;
  nb += 5;
  v |= dx << nb;
  nb += de;
  *n = nb;
  return v;
}
MP_PNG_HD inline int match_bits(int L, int d) {
  int n;
  (void)match_code(L, d, &n);
  return n;
}

// ---- a band's two forms -------------------------------------------------------------------------
constexpr int BLOCK_HEAD_BITS = 3;   // BFINAL, BTYPE
constexpr int EOB_BITS = 7;          // symbol 256
constexpr uint32_t FIXED_HEAD = 2u;  // BFINAL 0, BTYPE 01, LSB first
// bytes of a band whose tokens take token_bits, in the fixed form: the block, then the empty stored
// block's header padded to a byte, LEN 0000 and NLEN ffff
MP_PNG_HD constexpr int fixed_band_bytes(int64_t token_bits) {
  return (int)((BLOCK_HEAD_BITS + token_bits + EOB_BITS + BLOCK_HEAD_BITS + 7) / 8) + 4;
}
// in the stored form: 00, LEN, NLEN, the bytes; then 00 / 01, 0000, ffff
MP_PNG_HD constexpr int stored_band_bytes(int len) { return 5 + len + 5; }

// ---- the file -----------------------------------------------------------------------------------
constexpr int SIG_BYTES = 8, CHUNK_BYTES = 12;               // a chunk's length, type and CRC
constexpr int HEAD_BYTES = SIG_BYTES + CHUNK_BYTES + 13;     // signature and IHDR
constexpr int TAIL_BYTES = CHUNK_BYTES + 4 + CHUNK_BYTES;    // the Adler-32's IDAT and IEND
constexpr int ZLIB_HEAD_BYTES = 2;                           // 78 01, in band 0's chunk
// the longest chunk of a band of len raw bytes (band 0's has the zlib header)
MP_PNG_HD constexpr int band_chunk_max(int len, bool first) {
  return CHUNK_BYTES + (first ? ZLIB_HEAD_BYTES : 0) + stored_band_bytes(len);
}
// the exact worst case of a file: every band stored
MP_PNG_HD constexpr int64_t bound(int h, int w) {
  return (int64_t)HEAD_BYTES + ZLIB_HEAD_BYTES + TAIL_BYTES + (int64_t)band_count(h, w) * (CHUNK_BYTES + 10) +
         (int64_t)h * row_bytes(w);
}

// ---- checksums ----------------------------------------------------------------------------------
MP_PNG_HD inline uint32_t crc_table_entry(uint32_t i) {
  for (int k = 0; k < 8; ++k) i = (i & 1u) ? (i >> 1) ^ CRC_POLY : i >> 1;
  return i;
}
// a * b mod P in the reflected representation (bit 31 is x^0)
MP_PNG_HD inline uint32_t crc_mul(uint32_t a, uint32_t b) {
  uint32_t p = 0;
  for (uint32_t m = 1u << 31; m && a; m >>= 1) {
    if (a & m) { p ^= b; a &= ~m; }
    b = (b & 1u) ? (b >> 1) ^ CRC_POLY : b >> 1;
  }
  return p;
}
// x^(8 n) mod P: the factor that moves a CRC past n following bytes,
// crc(A || B) = crc_mul(crc_shift(len B), crc(A)) ^ crc(B)
MP_PNG_HD inline uint32_t crc_shift(uint32_t n) {
  uint32_t r = 1u << 31, q = 1u << 23;   // x^0; x^8
  for (; n; n >>= 1) {
    if (n & 1u) r = crc_mul(r, q);
    q = crc_mul(q, q);
  }
  return r;
}

// a band's contribution to the file's Adler-32: with s1, s2 as above (mod 65521) and `after` raw
// bytes following the band, A = 1 + sum s1 and B = N + sum (s2 + s1 * after) over the bands, N the
// stream's length -- the combine formula unrolled from A0 = 1, B0 = 0
MP_PNG_HD inline uint32_t adler_b_term(uint32_t s1, uint32_t s2, int64_t after) {
  return (uint32_t)((s2 + (uint64_t)s1 * (uint64_t)(after % ADLER_MOD)) % ADLER_MOD);
}

}  // namespace mppng
