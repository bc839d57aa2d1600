// The host encoder of png16_rule.hpp on png_host.hpp's frame: the rule on one thread, written the plain
// way -- a row's five filters one after the other, one token after the other, the three forms' sizes
// and the dynamic block's header.  Plain C++ (no HIP), so that tests/png16_rule_main.cpp builds it with
// the host sanitizers; mp_png16.hip wraps it for the library, and the kernels of k_png16.hip are
// compared with it byte for byte.
#pragma once
#include <stdexcept>

#include "png16_rule.hpp"
#include "png_host.hpp"

namespace mppng16h {

using mppngh::BitWriter;

// what mp_png16_band_stats_host reports of a band (include/monkeypose_png16.h)
constexpr int STAT_INTS = 9;
struct BandStats {
  int32_t form, filters[mppng16::NFILT], matches, dist_symbols, depth;
};
static_assert(sizeof(BandStats) == STAT_INTS * 4, "nine int32 a band");

// the 16-bit grayscale format, for the file's frame on the host and on the device
struct Gray16 {
  static constexpr int BIT_DEPTH = 16, COLOUR_TYPE = 0;
  MP_PNG_HD static constexpr int row_bytes(int w) { return mppng16::row_bytes(w); }
  static constexpr int band_rows(int w) { return mppng16::band_rows(w); }
  static constexpr int band_count(int h, int w) { return mppng16::band_count(h, w); }
  static constexpr int band_len(int h, int w, int k) { return mppng16::band_len(h, w, k); }
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
    const mppngh::Match m = mppngh::best_match(a, len, p, cd, nc);
    const int bl = m.len, bd = m.dist;
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
    mppngh::put_stored_block(out, a, len, last);
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
  mppngh::put_empty_block(out);
  // the size the rule's formulas gave is the size written
  const int want = form == R::FORM_STORED ? stored_b : form == R::FORM_FIXED ? fixed_b : dynamic_b;
  if ((int)(out.size() - at) != want) throw std::logic_error("png16: a band's bytes are not its formula's");
}

// one frame [h][w] -> its file at out (bound(h, w) bytes are enough); stats: band_count entries or null
inline size_t encode_image(const uint16_t* frame, int h, int w, uint8_t* out, BandStats* stats) {
  if (stats) std::memset(stats, 0, (size_t)mppng16::band_count(h, w) * sizeof *stats);
  return mppngh::encode_file<Gray16>(
      h, w, out,
      [&](int k, int r0, int nr, uint8_t* raw) { filter_rows(frame, w, r0, nr, raw, stats ? stats[k].filters : nullptr); },
      [&](int k, const uint8_t* a, int len, bool last, std::vector<uint8_t>& data) {
        encode_band(a, len, w, last, data, stats ? stats + k : nullptr);
      });
}

}  // namespace mppng16h
