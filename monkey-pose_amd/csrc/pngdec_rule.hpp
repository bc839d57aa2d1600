// The rule of mp_png_decode_host / mp_png_decode_dev (include/monkeypose_pngdec.h), stated once for
// the host decoder (mp_pngdec.hip), the kernels (k_pngdec.hip) and a stand-alone sanitizer build.
// Plain C++: no zlib, no library call.  A file goes through four stages, and its status is the
// first failure in this order, so host and device always agree:
//
// parse     the signature; chunks of length, type, data, CRC-32.  IHDR first, 13 bytes; IEND last,
//           empty, nothing after it; at least one IDAT and the IDATs consecutive (a zero-length one
//           is legal); PLTE accepted before the IDATs and ignored; ancillary chunks (lower-case
//           first letter) skipped wherever they stand; any other critical chunk refused.  The whole
//           file is walked first (status 1), then every chunk's CRC counts (2), then the IHDR:
//           interlace, compression and filter method 0 and one of gray 16, gray 8, RGB 8 (3; a zero
//           width or height too), and h, w and the format are the call's (4).  The IDAT payloads are
//           gathered into one contiguous zlib stream on the way.
// inflate   RFC 1950 / 1951 in full: header CM 8, CINFO <= 7, FCHECK, no FDICT; stored, fixed and
//           dynamic blocks; code sets by zlib's verdicts (over-subscribed refused, incomplete refused
//           unless its longest code is 1 bit, no code-length code incomplete, symbol 256 present, at
//           most 286 / 30 symbols); symbols 286 / 287 and distances 30 / 31 refused; a distance
//           before the first byte, BTYPE 3, LEN != ~NLEN, input ending early, output other than
//           h (1 + row bytes), anything but 4 bytes after the last block: all status 5.  Then the
//           Adler-32 (6).
// unfilter  filter bytes 0..4 (7 otherwise), byte-wise at distance bpp, missing neighbours zero,
//           Paeth's ties in the order a, b, c.
//
// Safety: every read is bounded by the file's size or the stream's length (bits past the end read
// as zero and are counted, and the count is checked once a symbol), every write by the expected
// output length, and every loop iteration consumes at least one input bit, one chunk or ends.
//
// inflate() is a template over an IO policy: the host's (HostInflate, below) reads and writes plain
// memory on one thread; the device's (k_pngdec.hip) is one wave whose lanes all run the same symbol
// loop and share the table builds, the match copies and the flushes.
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MP_PD_HD __host__ __device__
#else
#define MP_PD_HD
#endif

#include <cstdint>

namespace mppd {

constexpr int MAX_HW = 4096;
constexpr int MAX_N = 65535;
constexpr int64_t MAX_STRIDE = (int64_t)1 << 30;
enum { GRAY16 = 0, GRAY8 = 1, RGB8 = 2 };
enum { ST_OK = 0, ST_CONTAINER = 1, ST_CRC = 2, ST_UNSUPPORTED = 3, ST_MISMATCH = 4, ST_STREAM = 5, ST_ADLER = 6,
       ST_FILTER = 7 };
constexpr uint32_t ADLER_MOD = 65521u;
constexpr uint32_t CRC_POLY = 0xedb88320u;

MP_PD_HD constexpr bool format_ok(int f) { return f >= 0 && f <= 2; }
MP_PD_HD constexpr int bpp(int format) { return format == GRAY16 ? 2 : format == GRAY8 ? 1 : 3; }
MP_PD_HD constexpr int row_bytes(int w, int format) { return w * bpp(format); }
// the raw stream: h rows of a filter byte and the row
MP_PD_HD constexpr int64_t raw_bytes(int h, int w, int format) { return (int64_t)h * (1 + row_bytes(w, format)); }
MP_PD_HD constexpr int64_t round16(int64_t v) { return (v + 15) & ~(int64_t)15; }

// ---- a file's slot in the work area: a 16-byte head, the zlib stream, the raw stream ------------
constexpr int SLOT_HEAD = 16;        // int32 status so far, int32 zlib length
MP_PD_HD constexpr int64_t slot_bytes(int h, int w, int format, int64_t file_stride) {
  return SLOT_HEAD + round16(file_stride) + round16(raw_bytes(h, w, format));
}

MP_PD_HD inline uint32_t be32(const uint8_t* p) {
  return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | (uint32_t)p[3];
}
MP_PD_HD inline uint32_t crc_table_entry(uint32_t i) {
  for (int k = 0; k < 8; ++k) i = (i & 1u) ? (i >> 1) ^ CRC_POLY : i >> 1;
  return i;
}
MP_PD_HD inline bool is_type(const uint8_t* t, char a, char b, char c, char d) {
  return t[0] == (uint8_t)a && t[1] == (uint8_t)b && t[2] == (uint8_t)c && t[3] == (uint8_t)d;
}
MP_PD_HD inline bool is_letter(uint8_t c) { return (c >= 'A' && c <= 'Z') || (c >= 'a' && c <= 'z'); }

// ---- parse ---------------------------------------------------------------------------------------
// IO: uint32_t crc(const uint8_t* p, int64_t n) -- the CRC-32 of n bytes;
//     void copy(uint8_t* dst, const uint8_t* src, int64_t n).
// z takes the IDAT payloads (at most `size` bytes), *zlen their total.  Every iteration moves p
// forward by at least 12 bytes.
template <class IO>
MP_PD_HD inline int parse_file(const uint8_t* f, int64_t size, int h, int w, int format, uint8_t* z, int64_t* zlen,
                               IO& io) {
  *zlen = 0;
  if (size < 8) return ST_CONTAINER;
  const uint8_t sig[8] = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1a, '\n'};
  for (int i = 0; i < 8; ++i)
    if (f[i] != sig[i]) return ST_CONTAINER;
  int64_t p = 8, zl = 0;
  bool first = true, iend = false, crc_bad = false;
  int idat = 0;                        // 0 none yet, 1 inside the run, 2 after it
  uint8_t ihdr[13] = {0};
  while (p < size) {
    if (iend || size - p < 12) return ST_CONTAINER;
    const uint32_t len = be32(f + p);
    if (len > 0x7fffffffu || (int64_t)len > size - p - 12) return ST_CONTAINER;
    const uint8_t* t = f + p + 4;
    for (int i = 0; i < 4; ++i)
      if (!is_letter(t[i])) return ST_CONTAINER;
    const bool is_ihdr = is_type(t, 'I', 'H', 'D', 'R');
    if (first != is_ihdr) return ST_CONTAINER;
    if (is_ihdr) {
      if (len != 13) return ST_CONTAINER;
      for (int i = 0; i < 13; ++i) ihdr[i] = f[p + 8 + i];
    } else if (is_type(t, 'I', 'D', 'A', 'T')) {
      if (idat == 2) return ST_CONTAINER;
      idat = 1;
      io.copy(z + zl, f + p + 8, (int64_t)len);
      zl += len;
    } else {
      if (idat == 1) idat = 2;
      if (is_type(t, 'I', 'E', 'N', 'D')) {
        if (len != 0 || idat == 0) return ST_CONTAINER;
        iend = true;
      } else if (is_type(t, 'P', 'L', 'T', 'E')) {
        if (idat != 0) return ST_CONTAINER;
      } else if (!(t[0] & 0x20)) {
        return ST_CONTAINER;
      }
    }
    if (io.crc(t, (int64_t)len + 4) != be32(f + p + 8 + len)) crc_bad = true;
    first = false;
    p += 12 + (int64_t)len;
  }
  if (!iend) return ST_CONTAINER;
  if (crc_bad) return ST_CRC;
  const uint32_t fw = be32(ihdr), fh = be32(ihdr + 4);
  const int depth = ihdr[8], ctype = ihdr[9];
  if (fw == 0 || fh == 0 || fw > 0x7fffffffu || fh > 0x7fffffffu) return ST_UNSUPPORTED;
  if (ihdr[10] != 0 || ihdr[11] != 0 || ihdr[12] != 0) return ST_UNSUPPORTED;
  int ff;
  if (ctype == 0 && depth == 16) ff = GRAY16;
  else if (ctype == 0 && depth == 8) ff = GRAY8;
  else if (ctype == 2 && depth == 8) ff = RGB8;
  else return ST_UNSUPPORTED;
  if (ff != format || fw != (uint32_t)w || fh != (uint32_t)h) return ST_MISMATCH;
  *zlen = zl;
  return ST_OK;
}

// ---- inflate -------------------------------------------------------------------------------------
constexpr int MAX_BITS = 15, MAX_LCODES = 286, MAX_DCODES = 30, FIXED_LCODES = 288, FIXED_DCODES = 32;
constexpr int FAST_BITS = 11, FAST_SIZE = 1 << FAST_BITS;

// a canonical Huffman code: puff's count / symbol pair for any length, and a direct table over the
// next FAST_BITS bits for the codes that fit: (symbol << 4) | length, 0 where no short code matches
struct Huff {
  uint16_t count[MAX_BITS + 1];
  uint16_t symbol[FIXED_LCODES];
  uint16_t fast[FAST_SIZE];
};
struct Tables {
  Huff ll, dd;
  uint16_t code[FIXED_LCODES];         // a build's scratch: each symbol's code, and the two running rows
  uint16_t offs[MAX_BITS + 1], next[MAX_BITS + 1];
  int left, maxlen;                    // a build's verdict, published by the lead lane
  uint8_t lens[FIXED_LCODES + FIXED_DCODES];
};

MP_PD_HD inline uint32_t rev_bits(uint32_t v, int n) {   // 1 <= n <= 16
  v = ((v & 0x5555u) << 1) | ((v >> 1) & 0x5555u);
  v = ((v & 0x3333u) << 2) | ((v >> 2) & 0x3333u);
  v = ((v & 0x0f0fu) << 4) | ((v >> 4) & 0x0f0fu);
  v = ((v & 0x00ffu) << 8) | ((v >> 8) & 0x00ffu);
  return v >> (16 - n);
}

// The serial half of a build, on the lead lane: counts, the sorted symbols, every symbol's code.
// Returns < 0 over-subscribed, 0 complete (or no code at all), > 0 incomplete; T.maxlen the longest.
MP_PD_HD inline int huff_count(Huff& hf, Tables& T, const uint8_t* lens, int n) {
  for (int l = 0; l <= MAX_BITS; ++l) hf.count[l] = 0;
  for (int s = 0; s < n; ++s) hf.count[lens[s]]++;
  T.maxlen = 0;
  for (int l = 1; l <= MAX_BITS; ++l)
    if (hf.count[l]) T.maxlen = l;
  if (hf.count[0] == n) return 0;
  int left = 1;
  for (int l = 1; l <= MAX_BITS; ++l) {
    left <<= 1;
    left -= hf.count[l];
    if (left < 0) return left;
  }
  T.offs[1] = 0;
  T.next[1] = 0;
  for (int l = 1; l < MAX_BITS; ++l) {
    T.offs[l + 1] = (uint16_t)(T.offs[l] + hf.count[l]);
    T.next[l + 1] = (uint16_t)((T.next[l] + hf.count[l]) << 1);
  }
  for (int s = 0; s < n; ++s)
    if (lens[s]) {
      hf.symbol[T.offs[lens[s]]++] = (uint16_t)s;
      T.code[s] = T.next[lens[s]]++;
    }
  return left;
}

// IO (inflate): lane() / lanes() / lead() / sync() for the shared builds; Tables& tables();
//   uint32_t word(int64_t i)   input bytes i .. i + 3 (i a multiple of 4), little-endian, zero past
//                              the stream's end
//   lit(b), match(dist, len)   append to the output; the caller has checked both bounds
//   finish()                   the output is complete;  adler() its Adler-32 afterwards
//   uni(v)                     v, which every lane holds alike (the device keeps it in a scalar register)
// Every length is at most MAX_BITS (a 4-bit field or a code-length symbol 0 .. 15).
template <class IO>
MP_PD_HD inline int huff_build(IO& io, Huff& hf, const uint8_t* lens, int n, int* maxlen) {
  Tables& T = io.tables();
  if (io.lead()) T.left = huff_count(hf, T, lens, n);
  for (int k = io.lane(); k < FAST_SIZE; k += io.lanes()) hf.fast[k] = 0;
  io.sync();
  const int left = T.left;
  *maxlen = T.maxlen;
  if (left < 0) return left;
  for (int s = io.lane(); s < n; s += io.lanes()) {
    const int l = lens[s];
    if (l >= 1 && l <= FAST_BITS) {
      const uint16_t e = (uint16_t)((s << 4) | l);
      for (uint32_t k = rev_bits(T.code[s], l); k < (uint32_t)FAST_SIZE; k += 1u << l) hf.fast[k] = e;
    }
  }
  io.sync();
  return left;
}

struct Bits {
  uint64_t acc = 0;
  int nb = 0;
  int64_t ip = 0;      // the next input byte to load, a multiple of 4
  int64_t used = 0;    // bits taken so far
};
template <class IO>
MP_PD_HD inline void fill(Bits& b, IO& io) {   // at least 32 bits afterwards
  if (b.nb <= 32) {
    b.acc |= (uint64_t)io.word(b.ip) << b.nb;
    b.ip += 4;
    b.nb += 32;
  }
}
MP_PD_HD inline uint32_t take(Bits& b, int n) {   // n <= 32 <= b.nb
  const uint32_t v = (uint32_t)(b.acc & (((uint64_t)1 << n) - 1));
  b.acc >>= n;
  b.nb -= n;
  b.used += n;
  return v;
}
template <class IO>
MP_PD_HD inline uint32_t get(Bits& b, IO& io, int n) {
  fill(b, io);
  return take(b, n);
}
// the next symbol of hf, or -1 when the bits are no code of it
template <class IO>
MP_PD_HD inline int decode(Bits& b, IO& io, const Huff& hf) {
  fill(b, io);
  const uint32_t e = io.uni(hf.fast[(uint32_t)b.acc & (FAST_SIZE - 1)]);
  if (e) {
    (void)take(b, (int)(e & 15u));
    return (int)(e >> 4);
  }
  uint32_t bits = (uint32_t)b.acc;
  int code = 0, first = 0, index = 0;
  for (int len = 1; len <= MAX_BITS; ++len) {
    code |= (int)(bits & 1u);
    bits >>= 1;
    const int count = (int)io.uni(hf.count[len]);
    if (code - count < first) {
      (void)take(b, len);
      return (int)io.uni(hf.symbol[index + (code - first)]);
    }
    index += count;
    first += count;
    first <<= 1;
    code <<= 1;
  }
  (void)take(b, MAX_BITS);
  return -1;
}

MP_PD_HD inline int length_base(int s, int* extra) {   // s = symbol - 257, 0 .. 28
  if (s < 8) { *extra = 0; return 3 + s; }
  if (s == 28) { *extra = 0; return 258; }
  const int e = (s - 4) >> 2;
  *extra = e;
  return 3 + ((4 + ((s - 4) & 3)) << e);
}
MP_PD_HD inline int dist_base(int s, int* extra) {     // s = 0 .. 29
  if (s < 4) { *extra = 0; return 1 + s; }
  const int e = (s - 2) >> 1;
  *extra = e;
  return 1 + ((2 + (s & 1)) << e);
}

// the zlib stream of zlen bytes -> exactly `expect` output bytes: ST_OK, ST_STREAM or ST_ADLER
template <class IO>
MP_PD_HD inline int inflate(IO& io, int64_t zlen, int64_t expect) {
  Tables& T = io.tables();
  Bits b;
  const int64_t total = zlen * 8;
  int64_t produced = 0;
  if (zlen < 2) return ST_STREAM;
  {
    const uint32_t cmf = get(b, io, 8), flg = get(b, io, 8);
    if ((cmf & 15u) != 8u || (cmf >> 4) > 7u || ((cmf << 8) | flg) % 31u != 0u || (flg & 0x20u)) return ST_STREAM;
  }
  for (bool last = false; !last;) {
    if (b.used + 3 > total) return ST_STREAM;
    last = get(b, io, 1) != 0;
    const uint32_t type = get(b, io, 2);
    if (type == 3) return ST_STREAM;
    if (type == 0) {
      (void)take(b, b.nb & 7);                                  // nb and used are congruent mod 8
      if (b.used + 32 > total) return ST_STREAM;
      const uint32_t len = get(b, io, 16), nlen = get(b, io, 16);
      if ((len ^ nlen) != 0xffffu) return ST_STREAM;
      if (b.used + (int64_t)len * 8 > total || produced + (int64_t)len > expect) return ST_STREAM;
      for (uint32_t i = 0; i < len; ++i) io.lit((uint8_t)get(b, io, 8));
      produced += len;
      continue;
    }
    int nl, nd;
    io.sync();                                                   // the last block's tables are done with
    if (type == 1) {
      nl = FIXED_LCODES, nd = FIXED_DCODES;
      for (int s = io.lane(); s < nl + nd; s += io.lanes())
        T.lens[s] = (uint8_t)(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : s < 288 ? 8 : 5);
      io.sync();
    } else {
      if (b.used + 14 > total) return ST_STREAM;
      nl = (int)get(b, io, 5) + 257;
      nd = (int)get(b, io, 5) + 1;
      const int nc = (int)get(b, io, 4) + 4;
      if (nl > MAX_LCODES || nd > MAX_DCODES) return ST_STREAM;
      const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
      uint8_t cl[19];
      for (int i = 0; i < 19; ++i) cl[i] = 0;
      for (int i = 0; i < nc; ++i) cl[order[i]] = (uint8_t)get(b, io, 3);
      if (b.used > total) return ST_STREAM;
      if (io.lead())
        for (int i = 0; i < 19; ++i) T.lens[i] = cl[i];
      io.sync();
      int mx;
      if (huff_build(io, T.dd, T.lens, 19, &mx) != 0 || mx == 0) return ST_STREAM;   // complete, as zlib asks
      int i = 0, prev = 0;
      bool has256 = false;
      while (i < nl + nd) {
        const int sym = decode(b, io, T.dd);
        if (sym < 0 || b.used > total) return ST_STREAM;
        int rep = 1, val = sym;
        if (sym == 16) {
          if (i == 0) return ST_STREAM;
          val = prev;
          rep = 3 + (int)get(b, io, 2);
        } else if (sym == 17) {
          val = 0;
          rep = 3 + (int)get(b, io, 3);
        } else if (sym == 18) {
          val = 0;
          rep = 11 + (int)get(b, io, 7);
        }
        if (i + rep > nl + nd) return ST_STREAM;
        if (val && i <= 256 && 256 < i + rep) has256 = true;
        // the distance lengths follow the literal / length ones at FIXED_LCODES, as in the fixed case
        if (io.lead())
          for (int k = i; k < i + rep; ++k) T.lens[k < nl ? k : FIXED_LCODES + (k - nl)] = (uint8_t)val;
        i += rep;
        prev = val;
      }
      if (b.used > total || !has256) return ST_STREAM;
      io.sync();
    }
    {
      int mx;
      int left = huff_build(io, T.ll, T.lens, nl, &mx);
      if (left < 0 || (left > 0 && mx != 1)) return ST_STREAM;
      left = huff_build(io, T.dd, T.lens + FIXED_LCODES, nd, &mx);
      if (left < 0 || (left > 0 && mx != 1)) return ST_STREAM;
    }
    for (;;) {
      const int sym = decode(b, io, T.ll);
      if (sym < 0 || b.used > total) return ST_STREAM;
      if (sym < 256) {
        if (produced >= expect) return ST_STREAM;
        io.lit((uint8_t)sym);
        produced += 1;
        continue;
      }
      if (sym == 256) break;
      if (sym >= 257 + 29) return ST_STREAM;
      int le, de;
      int len = length_base(sym - 257, &le);
      len += (int)get(b, io, le);
      const int ds = decode(b, io, T.dd);
      if (ds < 0 || ds >= MAX_DCODES) return ST_STREAM;
      int dist = dist_base(ds, &de);
      dist += (int)get(b, io, de);
      if (b.used > total || (int64_t)dist > produced || produced + len > expect) return ST_STREAM;
      io.match(dist, len);
      produced += len;
    }
  }
  (void)take(b, b.nb & 7);
  if (total - b.used != 32 || produced != expect) return ST_STREAM;
  io.finish();
  uint32_t want = 0;
  for (int i = 0; i < 4; ++i) want = (want << 8) | get(b, io, 8);
  return want == io.adler() ? ST_OK : ST_ADLER;
}

// ---- unfilter ------------------------------------------------------------------------------------
MP_PD_HD inline uint8_t paeth(int a, int b, int c) {
  const int p = a + b - c;
  const int pa = p > a ? p - a : a - p, pb = p > b ? p - b : b - p, pc = p > c ? p - c : c - p;
  return (uint8_t)((pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c));
}
MP_PD_HD inline uint8_t unfilter_byte(int ft, uint8_t x, uint8_t a, uint8_t b, uint8_t c) {
  switch (ft) {
    case 0: return x;
    case 1: return (uint8_t)(x + a);
    case 2: return (uint8_t)(x + b);
    case 3: return (uint8_t)(x + (((int)a + (int)b) >> 1));
    default: return (uint8_t)(x + paeth(a, b, c));
  }
}

// ---- the host's policies and one file on the host ------------------------------------------------
struct HostParse {
  uint32_t crc(const uint8_t* p, int64_t n) {
    uint32_t c = 0xffffffffu;
    for (int64_t i = 0; i < n; ++i) c = crc_table_entry((c ^ p[i]) & 0xffu) ^ (c >> 8);
    return ~c;
  }
  void copy(uint8_t* dst, const uint8_t* src, int64_t n) {
    for (int64_t i = 0; i < n; ++i) dst[i] = src[i];
  }
};

struct HostInflate {
  const uint8_t* z;
  int64_t zlen;
  uint8_t* raw;
  int64_t pos = 0;
  Tables T;
  HostInflate(const uint8_t* z_, int64_t zlen_, uint8_t* raw_) : z(z_), zlen(zlen_), raw(raw_) {}
  int lane() const { return 0; }
  int lanes() const { return 1; }
  bool lead() const { return true; }
  void sync() {}
  uint32_t uni(uint32_t v) const { return v; }
  Tables& tables() { return T; }
  uint32_t word(int64_t i) const {
    uint32_t v = 0;
    for (int k = 0; k < 4; ++k)
      if (i + k < zlen) v |= (uint32_t)z[i + k] << (8 * k);
    return v;
  }
  void lit(uint8_t v) { raw[pos++] = v; }
  void match(int dist, int len) {
    for (int j = 0; j < len; ++j, ++pos) raw[pos] = raw[pos - dist];
  }
  void finish() {}
  uint32_t adler() const {
    uint32_t A = 1, B = 0;
    for (int64_t i = 0; i < pos; ++i) {
      A = (A + raw[i]) % ADLER_MOD;
      B = (B + A) % ADLER_MOD;
    }
    return (B << 16) | A;
  }
};

// One file on the calling thread.  z: `size` bytes of scratch, raw: raw_bytes(h, w, format) bytes,
// out: the image (h w elements; uint16 for GRAY16), written in full -- zeros unless the status is 0.
inline int decode_file_host(const uint8_t* f, int64_t size, int h, int w, int format, uint8_t* z, uint8_t* raw,
                            void* out) {
  const int rb = row_bytes(w, format), bp = bpp(format);
  const int64_t out_bytes = (int64_t)h * rb;
  uint8_t* o8 = static_cast<uint8_t*>(out);
  for (int64_t i = 0; i < out_bytes; ++i) o8[i] = 0;
  int64_t zlen = 0;
  HostParse pio;
  int st = parse_file(f, size, h, w, format, z, &zlen, pio);
  if (st) return st;
  HostInflate iio(z, zlen, raw);
  st = inflate(iio, zlen, raw_bytes(h, w, format));
  if (st) return st;
  for (int r = 0; r < h; ++r)
    if (raw[(int64_t)r * (1 + rb)] > 4) return ST_FILTER;
  for (int r = 0; r < h; ++r) {
    uint8_t* row = raw + (int64_t)r * (1 + rb) + 1;
    const uint8_t* up = r ? row - (1 + rb) : nullptr;
    const int ft = row[-1];
    for (int i = 0; i < rb; ++i) {
      const uint8_t a = i >= bp ? row[i - bp] : 0, b = up ? up[i] : 0, c = (up && i >= bp) ? up[i - bp] : 0;
      row[i] = unfilter_byte(ft, row[i], a, b, c);
    }
    if (format == GRAY16) {
      uint16_t* o = static_cast<uint16_t*>(out) + (int64_t)r * w;
      for (int x = 0; x < w; ++x) o[x] = (uint16_t)((row[2 * x] << 8) | row[2 * x + 1]);
    } else {
      for (int i = 0; i < rb; ++i) o8[(int64_t)r * rb + i] = row[i];
    }
  }
  return ST_OK;
}

}  // namespace mppd
