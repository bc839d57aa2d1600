// PNG files from 16-bit depth frames on the device (mp_png16_encode_dev).  The bytes are
// png16_rule.hpp's, the same the host encoder of png16_host.hpp writes; this file is how a workgroup
// arrives at them.  The shape is k_png.hip's -- one workgroup of 256 threads per (band, image), the band
// in LDS, then a second kernel that packs the bands' chunks into the file -- and the match, chain, crc
// and out stages are that file's algorithm restated here with this rule's distances, so that the RGB
// kernels keep their code and their bytes.
//
//   png16_band_kernel
//     stage    the band's source rows and the frame's row above them (zeros above row 0) are
//              contiguous in `frames`: aligned words in, bytes out to LDS (the jump region, which is
//              free until the match stage).
//     filter   one wave per row, rows dealt round robin.  A lane takes the bytes lane, lane + 64, ..
//              of its row and sums the five filters' costs; a butterfly of shuffles gives every lane the
//              row's five totals, best_filter picks, and the lanes write the filter byte and the
//              filtered bytes to the band.  Integer sums: the lanes' order does not show.
//     match, chain     k_png.hip's: per-chunk backward walk with the carry from the chunks' heads, then
//              pointer jumping from position 0 marks the positions the greedy parse visits.
//     count    the visited tokens' symbols into the two histograms with integer LDS atomics; the fixed
//              form's bits, the extra bits and the Adler-32 sums on the way.
//     codes    sym_rank from 256 lanes puts the used symbols in order; lane 0 runs plan_codes (the
//              trees, the limit, the header's sequence and the code-length code: at most 286 + 30 + 19
//              symbols); canon_code from 256 lanes again.  The dynamic form's bits are sum count x
//              length + extra bits, so the three forms' bytes are known before a token is written.
//     bits     a chunk's token bits in the chosen form, an exclusive scan over the 256 chunks.
//     emit     the whole IDAT chunk is built in LDS over the jump array.  Tokens enter with atomicOr
//              (distinct bits of a zeroed image); a dynamic token is at most 15 + 5 + 15 + 13 = 48 bits,
//              three words.  Lane 0 writes the dynamic header.  The stored form is byte stores.
//     crc, out k_png.hip's.
//   png16_file_kernel   k_png.hip's png_file_kernel with this format's IHDR and row length.
//
// Nothing is written outside out[i][0 .. sizes[i]), sizes and work.  Integer adds, ORs and XORs only:
// no result depends on the order in which atomics arrive.  All stores are vector stores.
#include "mp_kernels.hpp"
#include "png16_rule.hpp"

namespace mp {

namespace {

namespace R = mppng16;

constexpr int PT = 256;                                        // threads of a workgroup
constexpr int WAVE = 64, NWAVE = PT / WAVE;
constexpr int PQ = (R::MAX_BAND + PT - 1) / PT;                // positions a thread at most (33)
constexpr int NC = R::MAX_CANDS;
constexpr int SLOT_HEAD = 16;                                  // chunk bytes, Adler s1, Adler B term, 0

struct BandLds {
  int raw, tok, jump, mark, total;   // word offsets
};
// the source bytes of a band's filter stage: its rows and the one above, with up to 2 bytes in front
// of an address that is not a multiple of 4
__host__ __device__ constexpr int src_words(int rows, int w) { return ((rows + 1) * 2 * w + 2 + 3) / 4 + 1; }
// the LDS plan of a band of `rows` rows.  The jump region also holds, at other times, the source rows,
// the chunks' heads (NC * 256 uint16), the scan (256 words) and the chunk's image (two spare words:
// a token's third word).
__host__ __device__ constexpr BandLds band_lds(int rows, int w) {
  const int len = rows * R::row_bytes(w);
  BandLds L{};
  L.raw = 0;
  L.tok = L.raw + (len + 3) / 4 + 1;
  L.jump = L.tok + (len + 1) / 2;
  int jw = (len + 1 + 1) / 2;
  const int img = (mppng::band_chunk_max(len, true) + 3) / 4 + 2;
  if (jw < img) jw = img;
  if (jw < NC * PT / 2) jw = NC * PT / 2;
  if (jw < src_words(rows, w)) jw = src_words(rows, w);
  L.mark = L.jump + jw;
  L.total = L.mark + (len + 31) / 32;
  return L;
}
static_assert(NC * PT / 2 >= PT, "the scan fits where the heads do");

// what the kernel keeps in static LDS beside the band
struct BandStatic {
  R::DynTables T;
  uint32_t hist[R::NLL + R::NDIST];
  uint32_t crc[256];
  uint32_t acc[8];                   // fixed bits, CRC, Adler s1, s2, extra bits, dynamic bits, used ll, used dist
  R::DynPlan plan;
};
// the longest bands: one row of 4096 pixels, and 8192 bytes of several rows (w = 2047: two rows of 4095)
static_assert((size_t)band_lds(1, R::MAX_HW).total * 4 + sizeof(BandStatic) <= 64 * 1024 &&
                  (size_t)band_lds(R::band_rows(2047), 2047).total * 4 + sizeof(BandStatic) <= 64 * 1024,
              "a band, its per-position state and its code tables fit a workgroup's 64 KiB of LDS");

size_t slot_bytes(int h, int w) {
  return SLOT_HEAD + (size_t)((mppng::band_chunk_max(R::band_len(h, w, 0), true) + 15) / 16) * 16;
}

__device__ __forceinline__ void or_bits(uint32_t* img, uint32_t bit, uint32_t v, int n) {
  const uint32_t wd = bit >> 5, sh = bit & 31u;
  atomicOr(&img[wd], v << sh);
  if (sh + n > 32) atomicOr(&img[wd + 1], v >> (32 - sh));
}
// n <= 48: up to three words
__device__ __forceinline__ void or_bits64(uint32_t* img, uint32_t bit, uint64_t v, int n) {
  const uint32_t wd = bit >> 5, sh = bit & 31u;
  atomicOr(&img[wd], (uint32_t)(v << sh));
  if (sh + n > 32) atomicOr(&img[wd + 1], (uint32_t)(v >> (32 - sh)));
  if (sh + n > 64) atomicOr(&img[wd + 2], (uint32_t)(v >> (64 - sh)));
}

__device__ __forceinline__ void store_be32(uint8_t* p, uint32_t v) {
  p[0] = (uint8_t)(v >> 24);
  p[1] = (uint8_t)(v >> 16);
  p[2] = (uint8_t)(v >> 8);
  p[3] = (uint8_t)v;
}

__device__ inline uint32_t crc_small(const uint8_t* p, int n) {
  uint32_t c = 0xffffffffu;
  for (int i = 0; i < n; ++i) c = mppng::crc_table_entry((c ^ p[i]) & 0xffu) ^ (c >> 8);
  return ~c;
}

// a token of the dynamic form -> its bits, *n their number
__device__ __forceinline__ uint64_t dynamic_token(const R::DynTables& T, uint32_t tk, int d, uint8_t lit, int* n) {
  if (!tk) {
    *n = T.lllen[lit];
    return T.llcode[lit];
  }
  int eb, nb;
  uint32_t ev;
  const int ls = R::length_sym((int)(tk & 0x1ffu), &eb, &ev);
  uint64_t v = T.llcode[ls];
  nb = T.lllen[ls];
  v |= (uint64_t)ev << nb;
  nb += eb;
  const int ds = R::dist_sym(d, &eb, &ev);
  v |= (uint64_t)T.dcode[ds] << nb;
  nb += T.dlen[ds];
  v |= (uint64_t)ev << nb;
  nb += eb;
  *n = nb;
  return v;
}

__global__ __launch_bounds__(PT) void png16_band_kernel(const uint16_t* __restrict__ frames, int h, int w,
                                                        uint8_t* __restrict__ work, size_t slot) {
  extern __shared__ uint32_t smem[];
  __shared__ BandStatic S;

  const int t = threadIdx.x, k = blockIdx.x, nb = gridDim.x;
  const size_t img = blockIdx.y;
  const int rb = R::row_bytes(w), rows = R::band_rows(w);
  const int r0 = k * rows, nr = (h - r0 < rows) ? h - r0 : rows, len = nr * rb;
  const BandLds P = band_lds(nr, w);
  uint8_t* a = reinterpret_cast<uint8_t*>(smem + P.raw);
  uint16_t* tok = reinterpret_cast<uint16_t*>(smem + P.tok);
  uint16_t* jump = reinterpret_cast<uint16_t*>(smem + P.jump);
  uint8_t* srcb = reinterpret_cast<uint8_t*>(smem + P.jump);   // [nr + 1][2 w], before the heads are written
  uint16_t* head = jump;             // [NC][PT], before jump is written
  uint32_t* scan = smem + P.jump;    // [PT], after the chain
  uint32_t* image = smem + P.jump;   // the chunk, after the scan
  uint32_t* mark = smem + P.mark;
  R::DynTables& T = S.T;

  int cd[NC];
  R::cands(w, cd);

  // ---- stage
  S.crc[t] = mppng::crc_table_entry((uint32_t)t);
  if (t < 8) S.acc[t] = 0;
  for (int s = t; s < R::NLL + R::NDIST; s += PT) S.hist[s] = 0;
  const int w2 = 2 * w;
  {
    const int have = r0 > 0 ? 1 : 0;                            // the row above is the frame's
    const int nsrc = (nr + have) * w2, off = have ? 0 : w2;
    const uint8_t* src = reinterpret_cast<const uint8_t*>(frames + (img * h + (size_t)(r0 - have)) * w);
    const int mis = (int)(reinterpret_cast<uintptr_t>(src) & 3);
    const uint32_t* srcw = reinterpret_cast<const uint32_t*>(src - mis);
    const int nw = (mis + nsrc + 3) / 4;
    for (int i = t; i < nw; i += PT) {
      const uint32_t v = srcw[i];
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const int j = 4 * i + b - mis;
        if (j >= 0 && j < nsrc) srcb[off + j] = (uint8_t)(v >> (8 * b));
      }
    }
    if (!have)
      for (int i = t; i < w2; i += PT) srcb[i] = 0;
    for (int i = t; i < (len + 31) / 32; i += PT) mark[i] = (i == 0) ? 1u : 0u;
  }
  __syncthreads();

  // ---- filter: raw byte j of a row is byte j ^ 1 of its little-endian pixels
  {
    const int lane = t & (WAVE - 1), wv = t / WAVE;
    for (int r = wv; r < nr; r += NWAVE) {
      const uint8_t* up = srcb + (size_t)r * w2;
      const uint8_t* cur = up + w2;
      uint32_t cost[R::NFILT] = {0, 0, 0, 0, 0};
      for (int j = lane; j < w2; j += WAVE) {
        const int x = cur[j ^ 1], b = up[j ^ 1];
        const int av = j >= 2 ? cur[(j - 2) ^ 1] : 0, c = j >= 2 ? up[(j - 2) ^ 1] : 0;
#pragma unroll
        for (int f = 0; f < R::NFILT; ++f) cost[f] += (uint32_t)R::filter_cost(R::filter_byte(f, x, av, b, c));
      }
#pragma unroll
      for (int f = 0; f < R::NFILT; ++f)
        for (int o = WAVE / 2; o; o >>= 1) cost[f] += __shfl_xor(cost[f], o, WAVE);
      const int f = R::best_filter(cost);
      uint8_t* dst = a + (size_t)r * rb;
      if (lane == 0) dst[0] = (uint8_t)f;
      for (int j = lane; j < w2; j += WAVE) {
        const int x = cur[j ^ 1], b = up[j ^ 1];
        const int av = j >= 2 ? cur[(j - 2) ^ 1] : 0, c = j >= 2 ? up[(j - 2) ^ 1] : 0;
        dst[1 + j] = R::filter_byte(f, x, av, b, c);
      }
    }
  }
  __syncthreads();                   // the source rows are read: the heads may be written

  // ---- match
  const int C = (len + PT - 1) / PT;
  const int cs = t * C < len ? t * C : len, ce = (t + 1) * C < len ? (t + 1) * C : len;
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const int d = cd[c];
    int i = cs;
    while (i < ce && i >= d && a[i] == a[i - d]) ++i;
    head[c * PT + t] = (uint16_t)((i - cs) | ((ce > cs && i == ce) ? 0x8000 : 0));
  }
  __syncthreads();
  int run[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    int cr = 0;
    for (int u = t + 1; u < PT && cr < R::MAX_MATCH; ++u) {
      const uint32_t hv = head[c * PT + u];
      cr += (int)(hv & 0x7fffu);
      if (!(hv >> 15)) break;
    }
    run[c] = cr < R::MAX_MATCH ? cr : R::MAX_MATCH;
  }
  __syncthreads();                   // the heads are read: jump may be written
  for (int i = ce - 1; i >= cs; --i) {
    const uint8_t v = a[i];
    int bl = 0, bd = 0, bc = 0;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const int d = cd[c];
      const bool eq = i >= d && v == a[i - d];
      run[c] = eq ? (run[c] + 1 < R::MAX_MATCH ? run[c] + 1 : R::MAX_MATCH) : 0;
      if (run[c] > bl || (run[c] == bl && d < bd)) bl = run[c], bd = d, bc = c;
    }
    const bool m = bl >= R::MIN_MATCH;
    tok[i] = m ? (uint16_t)(bl | (bc << 9)) : (uint16_t)0;
    jump[i] = (uint16_t)(i + (m ? bl : 1));
  }
  if (t == 0) jump[len] = (uint16_t)len;
  __syncthreads();

  // ---- chain
  for (int step = 1; step < len; step <<= 1) {
    uint16_t nj[PQ];
    int added = 0;
#pragma unroll
    for (int q = 0; q < PQ; ++q) {
      const int i = t + PT * q;
      if (i < len) {
        const int j = jump[i];
        if (j < len && ((mark[i >> 5] >> (i & 31)) & 1u))
          added |= !((atomicOr(&mark[j >> 5], 1u << (j & 31)) >> (j & 31)) & 1u);
        nj[q] = jump[j];
      }
    }
    if (!__syncthreads_or(added)) break;
#pragma unroll
    for (int q = 0; q < PQ; ++q) {
      const int i = t + PT * q;
      if (i < len) jump[i] = nj[q];
    }
    __syncthreads();
  }

  // ---- count: the histograms, the fixed form's bits, the extra bits and the Adler-32 sums
  {
    uint32_t fbits = 0, xbits = 0, s1 = 0, s2 = 0;
    for (int i = cs; i < ce; ++i) {
      const uint32_t v = a[i];
      s1 += v;
      s2 += (uint32_t)(len - i) * v;
      if ((mark[i >> 5] >> (i & 31)) & 1u) {
        const uint32_t tk = tok[i];
        if (tk) {
          const int L = (int)(tk & 0x1ffu), d = cd[tk >> 9];
          int eb, db;
          uint32_t ev;
          atomicAdd(&S.hist[R::length_sym(L, &eb, &ev)], 1u);
          atomicAdd(&S.hist[R::NLL + R::dist_sym(d, &db, &ev)], 1u);
          xbits += (uint32_t)(eb + db);
          fbits += (uint32_t)mppng::match_bits(L, d);
        } else {
          atomicAdd(&S.hist[v], 1u);
          fbits += (uint32_t)mppng::literal_bits((int)v);
        }
      }
    }
    atomicAdd(&S.acc[0], fbits);
    atomicAdd(&S.acc[4], xbits);
    atomicAdd(&S.acc[2], s1 % mppng::ADLER_MOD);
    atomicAdd(&S.acc[3], s2 % mppng::ADLER_MOD);
  }
  __syncthreads();

  // ---- codes
  for (int s = t; s < R::NLL; s += PT) T.llf[s] = s == 256 ? (uint16_t)1 : (uint16_t)S.hist[s];
  if (t < R::NDIST) T.df[t] = (uint16_t)S.hist[R::NLL + t];
  __syncthreads();
  for (int s = t; s < R::NLL; s += PT)
    if (T.llf[s]) {
      T.llorder[R::sym_rank(T.llf, R::NLL, s)] = (uint16_t)s;
      atomicAdd(&S.acc[6], 1u);
    }
  if (t < R::NDIST && T.df[t]) {
    T.dorder[R::sym_rank(T.df, R::NDIST, t)] = (uint16_t)t;
    atomicAdd(&S.acc[7], 1u);
  }
  __syncthreads();
  if (t == 0) {
    int depth;
    S.plan = R::plan_codes(T, (int)S.acc[6], (int)S.acc[7], &depth);
  }
  __syncthreads();
  {
    uint32_t dbits = 0;
    for (int s = t; s < R::NLL; s += PT) {
      T.llcode[s] = T.lllen[s] ? (uint16_t)R::canon_code(T.lllen, R::NLL, s) : (uint16_t)0;
      if (s != 256) dbits += (uint32_t)T.llf[s] * T.lllen[s];
    }
    if (t < R::NDIST) {
      T.dcode[t] = T.dlen[t] ? (uint16_t)R::canon_code(T.dlen, R::NDIST, t) : (uint16_t)0;
      dbits += (uint32_t)T.df[t] * T.dlen[t];
    }
    if (t < R::NCL) T.clcode[t] = T.cllen[t] ? (uint16_t)R::canon_code(T.cllen, R::NCL, t) : (uint16_t)0;
    atomicAdd(&S.acc[5], dbits);
  }
  __syncthreads();
  const R::DynPlan plan = S.plan;
  const uint32_t dyn_bits = S.acc[5] + S.acc[4];
  const int eob_bits = T.lllen[256];
  const int fixed_b = mppng::fixed_band_bytes(S.acc[0]), stored_b = mppng::stored_band_bytes(len);
  const int dynamic_b = R::dynamic_band_bytes(plan.header_bits, dyn_bits, eob_bits);
  const int form = R::choose_form(stored_b, fixed_b, dynamic_b);

  // ---- bits
  uint32_t bits = 0;
  if (form != R::FORM_STORED)
    for (int i = cs; i < ce; ++i)
      if ((mark[i >> 5] >> (i & 31)) & 1u) {
        const uint32_t tk = tok[i];
        int n;
        if (form == R::FORM_FIXED) n = tk ? mppng::match_bits((int)(tk & 0x1ffu), cd[tk >> 9]) : mppng::literal_bits(a[i]);
        else (void)dynamic_token(T, tk, cd[tk >> 9], a[i], &n);
        bits += (uint32_t)n;
      }
  scan[t] = bits;                    // jump is dead from here
  __syncthreads();
  for (int o = 1; o < PT; o <<= 1) {
    const uint32_t add = t >= o ? scan[t - o] : 0u;
    __syncthreads();
    scan[t] += add;
    __syncthreads();
  }
  const uint32_t bit0 = scan[t] - bits, token_bits = scan[PT - 1];
  __syncthreads();                   // the scan is read: the image may be written

  // ---- emit
  const int zh = k == 0 ? mppng::ZLIB_HEAD_BYTES : 0;
  const int dlen = zh + (form == R::FORM_FIXED ? fixed_b : form == R::FORM_STORED ? stored_b : dynamic_b);
  const int csz = mppng::CHUNK_BYTES + dlen;
  const int imgw = (csz + 3) / 4;
  const uint32_t last = k == nb - 1 ? 1u : 0u;
  for (int i = t; i < imgw; i += PT) image[i] = 0;
  __syncthreads();
  uint8_t* ib = reinterpret_cast<uint8_t*>(image);
  const int d0 = 8 + zh;                                       // the deflate bytes' place
  if (form == R::FORM_STORED) {
    for (int i = t; i < len; i += PT) ib[d0 + 5 + i] = a[i];
    if (t == 0) {
      ib[d0] = 0;
      ib[d0 + 1] = (uint8_t)len;
      ib[d0 + 2] = (uint8_t)(len >> 8);
      ib[d0 + 3] = (uint8_t)~len;
      ib[d0 + 4] = (uint8_t)(~len >> 8);
      ib[d0 + 5 + len] = (uint8_t)last;
      ib[8 + dlen - 2] = 0xff;
      ib[8 + dlen - 1] = 0xff;
    }
  } else {
    const uint32_t head_bits = form == R::FORM_FIXED ? 0u : plan.header_bits;
    const uint32_t base = 8u * d0 + mppng::BLOCK_HEAD_BITS + head_bits;
    uint32_t bit = base + bit0;
    for (int i = cs; i < ce; ++i) {
      if ((mark[i >> 5] >> (i & 31)) & 1u) {
        const uint32_t tk = tok[i];
        int n;
        if (form == R::FORM_FIXED) {
          const uint32_t v = tk ? mppng::match_code((int)(tk & 0x1ffu), cd[tk >> 9], &n) : mppng::fixed_code(a[i], &n);
          or_bits(image, bit, v, n);
        } else {
          const uint64_t v = dynamic_token(T, tk, cd[tk >> 9], a[i], &n);
          or_bits64(image, bit, v, n);
        }
        bit += n;
      }
    }
    if (t == 0) {
      uint32_t p = 8u * d0;
      if (form == R::FORM_FIXED) {
        or_bits(image, p, mppng::FIXED_HEAD, mppng::BLOCK_HEAD_BITS);
        or_bits(image, base + token_bits + mppng::EOB_BITS, last, mppng::BLOCK_HEAD_BITS);
      } else {
        or_bits(image, p, R::DYNAMIC_HEAD, mppng::BLOCK_HEAD_BITS);
        p += mppng::BLOCK_HEAD_BITS;
        or_bits(image, p, (uint32_t)(plan.hlit - 257) | (uint32_t)(plan.hdist - 1) << 5 | (uint32_t)(plan.hclen - 4) << 10,
                R::DYN_HEAD_BITS);
        p += R::DYN_HEAD_BITS;
        for (int i = 0; i < plan.hclen; ++i, p += 3) or_bits(image, p, T.cllen[R::cl_order(i)], 3);
        for (int i = 0; i < plan.nseq; ++i) {
          const int s = T.seq_sym[i], n = T.cllen[s], xb = R::cl_extra_bits(s);
          or_bits(image, p, (uint32_t)T.clcode[s] | (uint32_t)T.seq_ext[i] << n, n + xb);
          p += n + xb;
        }
        or_bits(image, base + token_bits, T.llcode[256], eob_bits);
        or_bits(image, base + token_bits + eob_bits, last, mppng::BLOCK_HEAD_BITS);
      }
      or_bits(image, 8u * (uint32_t)(8 + dlen - 2), 0xffffu, 16);
    }
  }
  __syncthreads();                   // atomics and byte stores to one word are kept apart by this barrier
  if (t == 0) {
    store_be32(ib, (uint32_t)dlen);
    ib[4] = 'I', ib[5] = 'D', ib[6] = 'A', ib[7] = 'T';
    if (zh) ib[8] = 0x78, ib[9] = 0x01;
  }
  __syncthreads();

  // ---- crc over the type and the data: the bytes [4, 8 + dlen)
  {
    const int nbytes = 4 + dlen, E = 8 + dlen, pc = (nbytes + PT - 1) / PT;
    int b0 = E - (PT - t) * pc, b1 = b0 + pc;
    if (b0 < 4) b0 = 4;
    if (b1 > b0) {
      uint32_t c = 0xffffffffu;
      for (int i = b0; i < b1; ++i) c = S.crc[(c ^ ib[i]) & 0xffu] ^ (c >> 8);
      atomicXor(&S.acc[1], mppng::crc_mul(mppng::crc_shift((uint32_t)(E - b1)), ~c));
    }
  }
  __syncthreads();
  if (t == 0) store_be32(ib + 8 + dlen, S.acc[1]);
  __syncthreads();

  // ---- out
  uint32_t* dst = reinterpret_cast<uint32_t*>(work + (img * nb + k) * slot);
  if (t == 0) {
    const int64_t after = (int64_t)(h - (r0 + nr)) * rb;
    const uint32_t m1 = S.acc[2] % mppng::ADLER_MOD, m2 = S.acc[3] % mppng::ADLER_MOD;
    dst[0] = (uint32_t)csz;
    dst[1] = m1;
    dst[2] = mppng::adler_b_term(m1, m2, after);
    dst[3] = 0;
  }
  for (int i = t; i < imgw; i += PT) dst[SLOT_HEAD / 4 + i] = image[i];
}

__global__ __launch_bounds__(PT) void png16_file_kernel(const uint8_t* __restrict__ work, size_t slot, int h, int w,
                                                        uint8_t* __restrict__ out, int64_t out_stride,
                                                        int64_t* __restrict__ sizes) {
  __shared__ uint32_t s_sum[3];
  const int t = threadIdx.x, k = blockIdx.x, nb = gridDim.x;
  const size_t img = blockIdx.y;
  const uint8_t* base = work + img * nb * slot;
  const bool is_last = k == nb - 1;
  if (t < 3) s_sum[t] = 0;
  __syncthreads();
  uint32_t before = 0, s1 = 0, bt = 0;
  for (int j = t; j < (is_last ? nb : k); j += PT) {
    const uint32_t* hd = reinterpret_cast<const uint32_t*>(base + (size_t)j * slot);
    if (j < k) before += hd[0];
    s1 += hd[1];                     // the last band only: at most 4096 terms below 65521 each
    bt += hd[2];
  }
  atomicAdd(&s_sum[0], before);      // a file is below 2^26 bytes
  if (is_last) {
    atomicAdd(&s_sum[1], s1 % mppng::ADLER_MOD);
    atomicAdd(&s_sum[2], bt % mppng::ADLER_MOD);
  }
  __syncthreads();
  const uint8_t* src = base + (size_t)k * slot;
  const int csz = (int)reinterpret_cast<const uint32_t*>(src)[0];
  uint8_t* file = out + img * (size_t)out_stride;
  uint8_t* dst = file + mppng::HEAD_BYTES + s_sum[0];
  for (int i = t; i < csz; i += PT) dst[i] = src[SLOT_HEAD + i];
  if (k == 0 && t == 0) {
    uint8_t b[mppng::HEAD_BYTES] = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1a, '\n', 0, 0, 0, 13, 'I', 'H', 'D', 'R'};
    store_be32(b + 16, (uint32_t)w);
    store_be32(b + 20, (uint32_t)h);
    b[24] = 16, b[25] = 0, b[26] = 0, b[27] = 0, b[28] = 0;
    store_be32(b + 29, crc_small(b + 12, 17));
    for (int i = 0; i < mppng::HEAD_BYTES; ++i) file[i] = b[i];
  }
  if (is_last && t == 0) {
    const uint64_t N = (uint64_t)h * R::row_bytes(w);
    const uint32_t A = (1u + s_sum[1]) % mppng::ADLER_MOD;
    const uint32_t B = (uint32_t)((N + s_sum[2]) % mppng::ADLER_MOD);
    uint8_t b[mppng::TAIL_BYTES] = {0, 0, 0, 4, 'I', 'D', 'A', 'T', 0, 0, 0, 0, 0, 0, 0, 0,
                                    0, 0, 0, 0, 'I', 'E', 'N', 'D', 0xae, 0x42, 0x60, 0x82};
    store_be32(b + 8, (B << 16) | A);
    store_be32(b + 12, crc_small(b + 4, 8));
    uint8_t* tail = dst + csz;
    for (int i = 0; i < mppng::TAIL_BYTES; ++i) tail[i] = b[i];
    sizes[img] = (int64_t)mppng::HEAD_BYTES + s_sum[0] + csz + mppng::TAIL_BYTES;
  }
}

}  // namespace

size_t png16_work_bytes(int64_t n, int h, int w) { return (size_t)n * R::band_count(h, w) * slot_bytes(h, w); }

hipError_t launch_png16_encode(const uint16_t* frames, int64_t n, int h, int w, uint8_t* out, int64_t out_stride,
                               int64_t* sizes, void* work, hipStream_t st) {
  const int nb = R::band_count(h, w);
  const size_t slot = slot_bytes(h, w);
  const int rows = R::band_rows(w);
  const size_t lds = (size_t)band_lds(h < rows ? h : rows, w).total * 4;
  const dim3 grid((unsigned)nb, (unsigned)n);
  hipLaunchKernelGGL(png16_band_kernel, grid, dim3(PT), lds, st, frames, h, w, static_cast<uint8_t*>(work), slot);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(png16_file_kernel, grid, dim3(PT), 0, st, static_cast<const uint8_t*>(work), slot, h, w, out,
                     out_stride, sizes);
  return hipGetLastError();
}

}  // namespace mp
