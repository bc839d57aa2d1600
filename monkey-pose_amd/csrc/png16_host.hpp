// The host encoder of png16_rule.hpp: the rule on one thread, written the plain way -- a row's five
// filters one after the other, a position's matches by comparing bytes, one token after the other,
// the checksums byte by byte.  Plain C++ (no HIP), so that tests/png16_rule_main.cpp builds it with the
// host sanitizers; mp_png16.hip wraps it for the library, and the kernels of k_png16.hip are compared
// with it byte for byte.
#pragma once
#include <cstring>
#include <stdexcept>
#include <vector>

#include "png16_rule.hpp"

namespace mppng16h {

// what mp_png16_band_stats_host reports of a band (include/monkeypose_png16.h)
constexpr int STAT_INTS = 9;
struct BandStats {
  int32_t form, filters[mppng16::NFILT], matches, dist_symbols, depth;
};
static_assert(sizeof(BandStats) == STAT_INTS * 4, "nine int32 a band");

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

// rows [r0, r0 + nr) of the frame, filtered, to raw (nr * row_bytes(w)); filters[f] += rows that took f
inline void filter_rows(const uint16_t* frame, int w, int r0, int nr, uint8_t* raw, int32_t* filters) {
  const int rb = mppng16::row_bytes(w);
  const std::vector<uint16_t> zeros((size_t)w, 0);
  for (int r = 0; r < nr; ++r) {
    const uint16_t* cur = frame + (size_t)(r0 + r) * w;
    const uint16_t* up = r0 + r > 0 ? cur - w : zeros.data();
    uint32_t cost[mppng16::NFILT] = {0, 0, 0, 0, 0};
    for (int f = 0; f < mppng16::NFILT; ++f)
      for (int j = 0; j < 2 * w; ++j)
        cost[f] += (uint32_t)mppng16::filter_cost(mppng16::filter_byte(
            f, mppng16::pixel_byte(cur, j), mppng16::pixel_byte(cur, j - 2), mppng16::pixel_byte(up, j),
            mppng16::pixel_byte(up, j - 2)));
    const int f = mppng16::best_filter(cost);
    uint8_t* o = raw + (size_t)r * rb;
    o[0] = (uint8_t)f;
    for (int j = 0; j < 2 * w; ++j)
      o[1 + j] = mppng16::filter_byte(f, mppng16::pixel_byte(cur, j), mppng16::pixel_byte(cur, j - 2),
                                      mppng16::pixel_byte(up, j), mppng16::pixel_byte(up, j - 2));
    if (filters) filters[f] += 1;
  }
}

struct Token {
  uint16_t len, dist;   // len 0: the literal `dist`
};

// the deflate bytes of one band a[0 .. len), its empty stored block included, appended to out
inline void encode_band(const uint8_t* a, int len, int w, bool last, std::vector<uint8_t>& out, BandStats* st) {
  namespace R = mppng16;
  int cd[R::MAX_CANDS];
  const int nc = R::cands(w, cd);
  std::vector<Token> toks;
  toks.reserve((size_t)len);
  R::DynTables T;
  std::memset(&T, 0, sizeof T);
  int64_t fixed_bits = 0, extra_bits = 0;
  int matches = 0;
  for (int p = 0; p < len;) {
    int bl = 0, bd = 0;
    for (int c = 0; c < nc; ++c) {
      const int d = cd[c];
      if (d > p) continue;
      int L = 0;
      while (L < R::MAX_MATCH && p + L < len && a[p + L] == a[p + L - d]) ++L;
      if (L > bl || (L == bl && d < bd)) bl = L, bd = d;
    }
    if (bl >= R::MIN_MATCH) {
      int eb, db;
      uint32_t ev;
      T.llf[R::length_sym(bl, &eb, &ev)] += 1;
      T.df[R::dist_sym(bd, &db, &ev)] += 1;
      extra_bits += eb + db;
      fixed_bits += mppng::match_bits(bl, bd);
      toks.push_back({(uint16_t)bl, (uint16_t)bd});
      ++matches;
      p += bl;
    } else {
      T.llf[a[p]] += 1;
      fixed_bits += mppng::literal_bits(a[p]);
      toks.push_back({0, a[p]});
      p += 1;
    }
  }
  T.llf[256] = 1;
  const int mll = R::order_symbols(T.llf, R::NLL, T.llorder), md = R::order_symbols(T.df, R::NDIST, T.dorder);
  int depth;
  const R::DynPlan P = R::plan_codes(T, mll, md, &depth);
  for (int s = 0; s < R::NLL; ++s) T.llcode[s] = T.lllen[s] ? (uint16_t)R::canon_code(T.lllen, R::NLL, s) : 0;
  for (int s = 0; s < R::NDIST; ++s) T.dcode[s] = T.dlen[s] ? (uint16_t)R::canon_code(T.dlen, R::NDIST, s) : 0;
  for (int s = 0; s < R::NCL; ++s) T.clcode[s] = T.cllen[s] ? (uint16_t)R::canon_code(T.cllen, R::NCL, s) : 0;
  int64_t dyn_bits = extra_bits;
  for (int s = 0; s < R::NLL; ++s) dyn_bits += (int64_t)T.llf[s] * T.lllen[s];
  for (int s = 0; s < R::NDIST; ++s) dyn_bits += (int64_t)T.df[s] * T.dlen[s];
  dyn_bits -= T.lllen[256];           // symbol 256 is counted apart
  const int stored_b = mppng::stored_band_bytes(len), fixed_b = mppng::fixed_band_bytes(fixed_bits);
  const int dynamic_b = R::dynamic_band_bytes(P.header_bits, dyn_bits, T.lllen[256]);
  const int form = R::choose_form(stored_b, fixed_b, dynamic_b);
  if (st) {
    st->form = form;
    st->matches = matches;
    st->dist_symbols = md;
    st->depth = depth;
  }
  const size_t at = out.size();
  BitWriter bw{out};
  if (form == R::FORM_STORED) {
    const uint8_t head[5] = {0, (uint8_t)len, (uint8_t)(len >> 8), (uint8_t)~len, (uint8_t)(~len >> 8)};
    out.insert(out.end(), head, head + 5);
    out.insert(out.end(), a, a + len);
    out.push_back(last ? 1 : 0);
  } else {
    if (form == R::FORM_FIXED) {
      bw.put(mppng::FIXED_HEAD, mppng::BLOCK_HEAD_BITS);
      for (const Token& t : toks) {
        int n;
        const uint32_t v = t.len ? mppng::match_code(t.len, t.dist, &n) : mppng::fixed_code(t.dist, &n);
        bw.put(v, n);
      }
      int n;
      const uint32_t eob = mppng::fixed_code(256, &n);
      bw.put(eob, n);
    } else {
      bw.put(R::DYNAMIC_HEAD, mppng::BLOCK_HEAD_BITS);
      bw.put((uint32_t)(P.hlit - 257), 5);
      bw.put((uint32_t)(P.hdist - 1), 5);
      bw.put((uint32_t)(P.hclen - 4), 4);
      for (int i = 0; i < P.hclen; ++i) bw.put(T.cllen[R::cl_order(i)], 3);
      for (int i = 0; i < P.nseq; ++i) {
        const int s = T.seq_sym[i];
        bw.put(T.clcode[s], T.cllen[s]);
        bw.put(T.seq_ext[i], R::cl_extra_bits(s));
      }
      for (const Token& t : toks) {
        if (!t.len) {
          bw.put(T.llcode[t.dist], T.lllen[t.dist]);
          continue;
        }
        int eb;
        uint32_t ev;
        const int ls = R::length_sym(t.len, &eb, &ev);
        bw.put(T.llcode[ls], T.lllen[ls]);
        bw.put(ev, eb);
        const int ds = R::dist_sym(t.dist, &eb, &ev);
        bw.put(T.dcode[ds], T.dlen[ds]);
        bw.put(ev, eb);
      }
      bw.put(T.llcode[256], T.lllen[256]);
    }
    bw.put(last ? 1u : 0u, mppng::BLOCK_HEAD_BITS);
    bw.align();
  }
  const uint8_t empty[4] = {0, 0, 0xff, 0xff};
  out.insert(out.end(), empty, empty + 4);
  // the size the rule's formulas gave is the size written
  const int want = form == R::FORM_STORED ? stored_b : form == R::FORM_FIXED ? fixed_b : dynamic_b;
  if ((int)(out.size() - at) != want) throw std::logic_error("png16: a band's bytes are not its formula's");
}

// one frame [h][w] -> its file at out (bound(h, w) bytes are enough); stats: band_count entries or null
inline size_t encode_image(const uint16_t* frame, int h, int w, uint8_t* out, BandStats* stats) {
  namespace R = mppng16;
  static const uint8_t sig[8] = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1a, '\n'};
  uint8_t* p = out;
  std::memcpy(p, sig, 8);
  p += 8;
  uint8_t ihdr[13];
  put_be32(ihdr, (uint32_t)w);
  put_be32(ihdr + 4, (uint32_t)h);
  ihdr[8] = 16, ihdr[9] = 0, ihdr[10] = 0, ihdr[11] = 0, ihdr[12] = 0;
  p += put_chunk(p, "IHDR", ihdr, 13);

  const int rb = R::row_bytes(w), rows = R::band_rows(w), nb = R::band_count(h, w);
  std::vector<uint8_t> raw((size_t)rows * rb), data;
  uint32_t A = 1, B = 0;
  for (int k = 0; k < nb; ++k) {
    const int len = R::band_len(h, w, k);
    BandStats* st = stats ? stats + k : nullptr;
    if (st) std::memset(st, 0, sizeof *st);
    filter_rows(frame, w, k * rows, len / rb, raw.data(), st ? st->filters : nullptr);
    for (int i = 0; i < len; ++i) {
      A = (A + raw[i]) % mppng::ADLER_MOD;
      B = (B + A) % mppng::ADLER_MOD;
    }
    data.clear();
    if (k == 0) data.push_back(0x78), data.push_back(0x01);
    encode_band(raw.data(), len, w, k == nb - 1, data, st);
    p += put_chunk(p, "IDAT", data.data(), data.size());
  }
  uint8_t ad[4];
  put_be32(ad, (B << 16) | A);
  p += put_chunk(p, "IDAT", ad, 4);
  p += put_chunk(p, "IEND", nullptr, 0);
  return (size_t)(p - out);
}

}  // namespace mppng16h
