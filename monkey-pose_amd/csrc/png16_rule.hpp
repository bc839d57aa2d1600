// The byte rule of a 16-bit grayscale PNG file written by mp_png16_encode_host / mp_png16_encode_dev,
// stated once for the host encoder (png16_host.hpp), the kernels (k_png16.hip) and the size bound.
// It fixes every byte of the file, so the device's bytes are compared with the host's.  What it
// shares with the RGB rule -- the Adler-32 and CRC-32 arithmetic, the band separator, the fixed
// code -- is png_rule.hpp's.
//
// File        signature, IHDR (bit depth 16, colour type 0, no interlace), one IDAT per band, one IDAT
//             holding the Adler-32, IEND.  Band 0's IDAT starts with the zlib header 78 01.
// Rows        a filter byte, then 2 w bytes: every pixel's high byte, then its low byte.  The filter is
//             chosen per row among None (0), Sub (1), Up (2), Average (3) and Paeth (4) with bpp = 2
//             (PNG 1.2, 6.2 - 6.6): the one with the smallest sum of |residual byte taken as int8|,
//             ties to the smallest number.  The row above row 0 is zeros.  A row is filtered against
//             the frame's row above, whichever band that one lies in.
// Bands       band_rows(w) = max(1, BAND_BYTES / (1 + 2 w)) whole rows each, the last one what is
//             left.  A band is compressed from that band's filtered bytes alone: no match crosses it.
// Tokens      png_rule.hpp's greedy parse with the distances of cands(w).
// A band      one stored block, one fixed-Huffman block or one dynamic-Huffman block (RFC 1951 3.2.7),
//             whichever gives the fewest bytes; a tie goes to fixed, then to stored.  Then the empty
//             stored block of the RGB rule; the last band's carries BFINAL.
// Codes       the dynamic block's literal/length code covers the band's tokens and one symbol 256, its
//             distance code the tokens' distance symbols.  A code's lengths from its counts f[]:
//               order    the symbols with f > 0 by (f, symbol), ascending (sym_rank);
//               tree     Huffman's, by two queues: the leaves in that order and the merged nodes in the
//                        order they were made; each step takes twice the lighter front, the leaf when
//                        the weights are equal, and appends their sum.  A leaf's depth is its length
//                        in the unlimited code;
//               limit    count[l] = leaves of depth l, depths above the limit counted at the limit;
//                        while sum count[l] 2^(limit - l) exceeds 2^limit: count[limit] -= 1, the
//                        largest l < limit with count[l] > 0 gives one leaf to l + 1, which gains two
//                        (count[l] -= 1, count[l + 1] += 2), and the sum falls by one;
//               assign   the lengths limit, limit - 1, .. 1, count[l] times each, to the symbols in
//                        the order above (the rarest get the longest).
//             One symbol: length 1.  The limit is 15, and 7 for the code-length code.  Codes are the
//             canonical ones of RFC 1951 3.2.2 (canon_code).
// Header      HLIT = max(257, last literal/length symbol used + 1), HDIST = max(1, last distance
//             symbol used + 1); the HLIT + HDIST lengths as one sequence, left to right: at a length
//             v that starts r equal ones -- v = 0 and r >= 3: symbol 18 for min(r, 138) if r >= 11,
//             else 17 for r; v != 0, the length before it also v, r >= 3: 16 for min(r, 6); else v
//             itself.  HCLEN = max(4, last code-length symbol used in RFC order + 1).
// Edge cases  a band without a match has HDIST = 1 and that one distance length is 0 (no distance
//             code at all, RFC 1951 3.2.7); a band whose matches use one distance symbol gives it a
//             1-bit code (the code 0; an incomplete set, which the RFC allows for exactly this).  The
//             literal/length code always has two symbols or more (a band has a byte, and 256), and so
//             has the code-length code: the first nonzero length of the sequence stands for itself,
//             and 257 lengths or more are not all that one symbol (equal ones fold into 16s, zeros
//             are 0, 17 or 18).
#pragma once
#include "png_rule.hpp"

namespace mppng16 {

using mppng::BAND_BYTES;
using mppng::MAX_HW;
using mppng::MAX_N;
using mppng::MAX_MATCH;
using mppng::MIN_MATCH;
constexpr int MAX_CANDS = 6;
constexpr int NFILT = 5;
constexpr int NLL = 286, NDIST = 30, NCL = 19;      // symbols of the three codes
constexpr int LIMIT = 15, CL_LIMIT = 7;
constexpr int MAX_SEQ = NLL + NDIST;                 // entries of the header's length sequence
enum { FORM_STORED = 0, FORM_FIXED = 1, FORM_DYNAMIC = 2 };

MP_PNG_HD constexpr int row_bytes(int w) { return 1 + 2 * w; }
MP_PNG_HD constexpr int band_rows(int w) { return BAND_BYTES / row_bytes(w) > 1 ? BAND_BYTES / row_bytes(w) : 1; }
MP_PNG_HD constexpr int band_count(int h, int w) { return (h + band_rows(w) - 1) / band_rows(w); }
MP_PNG_HD constexpr int band_len(int h, int w, int k) {
  return (h - k * band_rows(w) < band_rows(w) ? h - k * band_rows(w) : band_rows(w)) * row_bytes(w);
}
// the longest band of any shape: one row of 4096 pixels
constexpr int MAX_BAND = row_bytes(MAX_HW) > BAND_BYTES ? row_bytes(MAX_HW) : BAND_BYTES;
static_assert(MAX_BAND == 8193, "the kernels' LDS plan is made for this");
static_assert(MAX_BAND + 1 <= 65535, "a band's counts and a Huffman node's weight fit 16 bits");

// the exact worst case of a file: every band stored
MP_PNG_HD constexpr int64_t bound(int h, int w) {
  return (int64_t)mppng::HEAD_BYTES + mppng::ZLIB_HEAD_BYTES + mppng::TAIL_BYTES +
         (int64_t)band_count(h, w) * (mppng::CHUNK_BYTES + 10) + (int64_t)h * row_bytes(w);
}

// the candidate distances: a run, the pixel before and the one before that, the pixel above and its
// two neighbours.  At w = 1 the fourth equals the first: a tie goes to the smallest distance by value.
MP_PNG_HD inline int cands(int w, int d[MAX_CANDS]) {
  d[0] = 1;
  d[1] = 2;
  d[2] = 4;
  d[3] = row_bytes(w) - 2;
  d[4] = row_bytes(w);
  d[5] = row_bytes(w) + 2;
  return MAX_CANDS;
}

// ---- filters --------------------------------------------------------------------------------------
// the filtered byte of x with a = the byte bpp before it, b = the byte above, c = the byte above a
MP_PNG_HD inline uint8_t filter_byte(int f, int x, int a, int b, int c) {
  int p = 0;
  if (f == 1) p = a;
  else if (f == 2) p = b;
  else if (f == 3) p = (a + b) >> 1;
  else if (f == 4) {
    const int q = a + b - c;
    const int pa = q > a ? q - a : a - q, pb = q > b ? q - b : b - q, pc = q > c ? q - c : c - q;
    p = (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
  }
  return (uint8_t)(x - p);
}
MP_PNG_HD inline int filter_cost(uint8_t r) { return r < 128 ? r : 256 - r; }
// byte j (0 .. 2 w) of a raw row from its pixels: the high byte first; out of the row: 0
MP_PNG_HD inline int pixel_byte(const uint16_t* row, int j) { return j < 0 ? 0 : ((j & 1) ? row[j >> 1] & 0xff : row[j >> 1] >> 8); }
MP_PNG_HD inline int best_filter(const uint32_t cost[NFILT]) {
  int f = 0;
  for (int g = 1; g < NFILT; ++g)
    if (cost[g] < cost[f]) f = g;
  return f;
}

// ---- symbols --------------------------------------------------------------------------------------
// a match length 3 .. 258 -> its symbol, *eb extra bits holding *ev
MP_PNG_HD inline int length_sym(int L, int* eb, uint32_t* ev) {
  const uint32_t x = (uint32_t)(L - 3);
  *eb = 0, *ev = 0;
  if (x < 8) return 257 + (int)x;
  if (L == MAX_MATCH) return 285;
  const int le = mppng::floor_log2(x) - 2;
  *eb = le, *ev = x & ((1u << le) - 1u);
  return 261 + 4 * le + (int)((x >> le) & 3u);
}
// a distance 1 .. 32768 -> its symbol
MP_PNG_HD inline int dist_sym(int d, int* eb, uint32_t* ev) {
  const uint32_t dd = (uint32_t)(d - 1);
  *eb = 0, *ev = 0;
  if (dd < 4) return (int)dd;
  const int de = mppng::floor_log2(dd) - 1;
  *eb = de, *ev = dd & ((1u << de) - 1u);
  return 2 * de + 2 + (int)((dd >> de) & 1u);
}

// ---- code construction ----------------------------------------------------------------------------
// the place of symbol s (f[s] > 0) in the order by (f, symbol) of the n symbols' used ones
MP_PNG_HD inline int sym_rank(const uint16_t* f, int n, int s) {
  int r = 0;
  const uint32_t fs = f[s];
  for (int u = 0; u < n; ++u) r += (f[u] && (f[u] < fs || (f[u] == fs && u < s))) ? 1 : 0;
  return r;
}

// scratch of code_lengths for a code of up to NLL symbols
struct TreeScratch {
  uint16_t weight[2 * NLL], parent[2 * NLL];
  uint8_t depth[2 * NLL];               // an unlimited tree of a band is at most 2 log_phi 8194 deep
};

// order[0 .. m): the used symbols by (f, symbol), m >= 1 -> len[order[i]]; len of the other symbols
// is not written.  Returns the depth of the unlimited tree.
MP_PNG_HD inline int code_lengths(const uint16_t* f, const uint16_t* order, int m, int limit, uint8_t* len,
                                  TreeScratch& S) {
  if (m == 1) {
    len[order[0]] = 1;
    return 1;
  }
  for (int i = 0; i < m; ++i) S.weight[i] = f[order[i]];
  int leaf = 0, node = m, made = m;     // the two queues' fronts; nodes made so far
  while (made < 2 * m - 1) {
    uint32_t sum = 0;
    for (int k = 0; k < 2; ++k) {
      int pick;
      if (leaf < m && (node >= made || S.weight[leaf] <= S.weight[node])) pick = leaf++;
      else pick = node++;
      sum += S.weight[pick];
      S.parent[pick] = (uint16_t)made;
    }
    S.weight[made++] = (uint16_t)sum;
  }
  uint16_t count[LIMIT + 2];
  for (int l = 0; l < LIMIT + 2; ++l) count[l] = 0;
  S.depth[made - 1] = 0;
  int deepest = 0;
  for (int i = made - 2; i >= 0; --i) {
    const int d = S.depth[S.parent[i]] + 1;
    S.depth[i] = (uint8_t)d;
    if (i < m) {
      count[d < limit ? d : limit] += 1;
      if (d > deepest) deepest = d;
    }
  }
  uint32_t total = 0;
  for (int l = 1; l <= limit; ++l) total += (uint32_t)count[l] << (limit - l);
  while (total > (1u << limit)) {
    count[limit] -= 1;
    for (int l = limit - 1; l >= 1; --l)
      if (count[l]) {
        count[l] -= 1;
        count[l + 1] += 2;
        break;
      }
    total -= 1;
  }
  int i = 0;
  for (int l = limit; l >= 1; --l)
    for (int c = 0; c < count[l]; ++c) len[order[i++]] = (uint8_t)l;
  return deepest;
}

// symbol s (len[s] > 0) of the canonical code of len[0 .. n), bit-reversed for the LSB-first stream
MP_PNG_HD inline uint32_t canon_code(const uint8_t* len, int n, int s) {
  const int L = len[s];
  uint32_t c = 0;
  for (int u = 0; u < n; ++u) {
    const int l = len[u];
    if (l && l < L) c += 1u << (L - l);
    else if (l == L && u < s) c += 1u;
  }
  return mppng::rev_bits(c, L);
}

// ---- the dynamic block's header ---------------------------------------------------------------------
constexpr int DYN_HEAD_BITS = 5 + 5 + 4;
MP_PNG_HD inline int cl_order(int i) {
  const uint8_t o[NCL] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
  return o[i];
}
MP_PNG_HD inline int cl_extra_bits(int sym) { return sym == 16 ? 2 : sym == 17 ? 3 : sym == 18 ? 7 : 0; }

// what a band's codes are, beside the lengths and codes themselves
struct DynPlan {
  int hlit, hdist, hclen, nseq;
  uint32_t header_bits;                 // HLIT .. the last length of the sequence
};

// one past the last symbol with a count, at least `least`
MP_PNG_HD inline int used_symbols(const uint16_t* f, int n, int least) {
  int k = n;
  while (k > least && !f[k - 1]) --k;
  return k;
}

// the length sequence lens[0 .. n) by the header rule -> seq_sym / seq_ext (n entries at most) and the
// code-length symbols' counts clf[NCL]; returns the entries
MP_PNG_HD inline int length_sequence(const uint8_t* lens, int n, uint8_t* seq_sym, uint8_t* seq_ext, uint16_t* clf) {
  for (int i = 0; i < NCL; ++i) clf[i] = 0;
  int k = 0;
  for (int i = 0; i < n;) {
    const int v = lens[i];
    int r = 1;
    while (i + r < n && lens[i + r] == v) ++r;
    int sym = v, ext = 0, adv = 1;
    if (v == 0 && r >= 11) sym = 18, adv = r < 138 ? r : 138, ext = adv - 11;
    else if (v == 0 && r >= 3) sym = 17, adv = r, ext = adv - 3;
    else if (v != 0 && i > 0 && lens[i - 1] == v && r >= 3) sym = 16, adv = r < 6 ? r : 6, ext = adv - 3;
    seq_sym[k] = (uint8_t)sym, seq_ext[k] = (uint8_t)ext;
    clf[sym] += 1;
    ++k;
    i += adv;
  }
  return k;
}

// everything a band's dynamic block is made from.  The counts come in; plan_codes and the two loops
// around it (order_symbols before, canon_code after) fill the rest.
struct DynTables {
  uint16_t llf[NLL], df[NDIST], clf[NCL];            // counts
  uint16_t llorder[NLL], dorder[NDIST], clorder[NCL];
  uint16_t llcode[NLL], dcode[NDIST], clcode[NCL];   // bit-reversed codes
  uint8_t lllen[NLL], dlen[NDIST], cllen[NCL];
  uint8_t lens[MAX_SEQ], seq_sym[MAX_SEQ], seq_ext[MAX_SEQ];
  TreeScratch tree;
};

// order[0 .. m) of the used symbols; returns m.  (The kernels call sym_rank from many lanes instead.)
MP_PNG_HD inline int order_symbols(const uint16_t* f, int n, uint16_t* order) {
  int m = 0;
  for (int s = 0; s < n; ++s)
    if (f[s]) {
      order[sym_rank(f, n, s)] = (uint16_t)s;
      ++m;
    }
  return m;
}

// llf, df, llorder (mll used symbols) and dorder (md) are set: the three codes' lengths, the header's
// sequence and its cost.  One thread's work: at most 286 + 30 + 19 symbols.  *depth: the deepest
// unlimited tree of the literal/length and the distance code.
MP_PNG_HD inline DynPlan plan_codes(DynTables& T, int mll, int md, int* depth) {
  DynPlan P;
  for (int s = 0; s < NLL; ++s) T.lllen[s] = 0;
  for (int s = 0; s < NDIST; ++s) T.dlen[s] = 0;
  for (int s = 0; s < NCL; ++s) T.cllen[s] = 0;
  int deep = code_lengths(T.llf, T.llorder, mll, LIMIT, T.lllen, T.tree);
  if (md) {
    const int dd = code_lengths(T.df, T.dorder, md, LIMIT, T.dlen, T.tree);
    if (dd > deep) deep = dd;
  }
  *depth = deep;
  P.hlit = used_symbols(T.llf, NLL, 257);
  P.hdist = used_symbols(T.df, NDIST, 1);
  for (int i = 0; i < P.hlit; ++i) T.lens[i] = T.lllen[i];
  for (int i = 0; i < P.hdist; ++i) T.lens[P.hlit + i] = T.dlen[i];
  P.nseq = length_sequence(T.lens, P.hlit + P.hdist, T.seq_sym, T.seq_ext, T.clf);
  const int mcl = order_symbols(T.clf, NCL, T.clorder);
  (void)code_lengths(T.clf, T.clorder, mcl, CL_LIMIT, T.cllen, T.tree);
  P.hclen = NCL;
  while (P.hclen > 4 && !T.cllen[cl_order(P.hclen - 1)]) --P.hclen;
  P.header_bits = DYN_HEAD_BITS + 3 * P.hclen;
  for (int s = 0; s < NCL; ++s) P.header_bits += (uint32_t)T.clf[s] * (uint32_t)(T.cllen[s] + cl_extra_bits(s));
  return P;
}

// ---- a band's three forms ---------------------------------------------------------------------------
constexpr uint32_t DYNAMIC_HEAD = 4u;   // BFINAL 0, BTYPE 10, LSB first
// bytes of a band in the dynamic form: header_bits, the tokens' bits, symbol 256's eob_bits
MP_PNG_HD constexpr int dynamic_band_bytes(int64_t header_bits, int64_t token_bits, int eob_bits) {
  return (int)((mppng::BLOCK_HEAD_BITS + header_bits + token_bits + eob_bits + mppng::BLOCK_HEAD_BITS + 7) / 8) + 4;
}
MP_PNG_HD inline int choose_form(int stored_b, int fixed_b, int dynamic_b) {
  if (fixed_b <= stored_b && fixed_b <= dynamic_b) return FORM_FIXED;
  return stored_b <= dynamic_b ? FORM_STORED : FORM_DYNAMIC;
}

}  // namespace mppng16
