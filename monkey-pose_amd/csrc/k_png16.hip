// PNG files from 16-bit depth frames on the device (mp_png16_encode_dev).  The bytes are
// png16_rule.hpp's, the same the host encoder of png16_host.hpp writes.  The band pipeline is
// png_band_dev.hpp's; what this file adds is the 16-bit rule's own:
//     stage    the band's source rows and the frame's row above them (zeros above row 0) are
//              contiguous in `frames`; they go to the jump region, which is free until the match stage.
//     filter   one wave per row, rows dealt round robin.  A lane takes the bytes lane, lane + 64, ..
//              of its row and sums the five filters' costs; a butterfly of shuffles gives every lane the
//              row's five totals, best_filter picks, and the lanes write the filter byte and the
//              filtered bytes to the band.  Integer sums: the lanes' order does not show.
//     count    the visited tokens' symbols into the two histograms with integer LDS atomics; the fixed
//              form's bits, the extra bits and the Adler-32 sums on the way.
//     codes    sym_rank from 256 lanes puts the used symbols in order; lane 0 runs plan_codes (the
//              trees, the limit, the header's sequence and the code-length code: at most 286 + 30 + 19
//              symbols); canon_code from 256 lanes again.  The dynamic form's bits are sum count x
//              length + extra bits, so the three forms' bytes are known before a token is written.
//     emit     a dynamic token is at most 15 + 5 + 15 + 13 = 48 bits, three words.  Lane 0 writes the
//              dynamic header.
#include "png16_host.hpp"
#include "png_band_dev.hpp"

namespace mp {

namespace {

namespace R = mppng16;

constexpr int WAVE = 64, NWAVE = PT / WAVE;
constexpr int PQ = (R::MAX_BAND + PT - 1) / PT;                // positions a thread at most (33)
constexpr int NC = R::MAX_CANDS;

// the source bytes of a band's filter stage: its rows and the one above, with up to 2 bytes in front
// of an address that is not a multiple of 4
__host__ __device__ constexpr int src_words(int rows, int w) { return ((rows + 1) * 2 * w + 2 + 3) / 4 + 1; }
// the LDS plan of a band of `rows` rows: two spare words behind the image (a token's third word), and
// the jump region holds the source rows first
__host__ __device__ constexpr BandLds lds_plan(int rows, int w) {
  return band_lds<NC>(rows * R::row_bytes(w), 2, src_words(rows, w));
}
static_assert(lds_plan(R::band_rows(512), 512).total == 9196 && lds_plan(1, R::MAX_HW).total == 10502 &&
                  lds_plan(R::band_rows(2047), 2047).total == 10496,
              "the plans of a 424 x 512 frame's bands and of the two longest bands");

// what the kernel keeps in static LDS beside the band
struct BandStatic {
  R::DynTables T;
  uint32_t hist[R::NLL + R::NDIST];
  uint32_t crc[256];
  uint32_t acc[8];                   // fixed bits, CRC, Adler s1, s2, extra bits, dynamic bits, used ll, used dist
  R::DynPlan plan;
};
// the longest bands: one row of 4096 pixels, and 8192 bytes of several rows (w = 2047: two rows of 4095)
static_assert((size_t)lds_plan(1, R::MAX_HW).total * 4 + sizeof(BandStatic) <= 64 * 1024 &&
                  (size_t)lds_plan(R::band_rows(2047), 2047).total * 4 + sizeof(BandStatic) <= 64 * 1024,
              "a band, its per-position state and its code tables fit a workgroup's 64 KiB of LDS");

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
  const BandLds P = lds_plan(nr, w);
  uint8_t* a = reinterpret_cast<uint8_t*>(smem + P.raw);
  uint16_t* tok = reinterpret_cast<uint16_t*>(smem + P.tok);
  uint16_t* jump = reinterpret_cast<uint16_t*>(smem + P.jump);
  uint8_t* srcb = reinterpret_cast<uint8_t*>(smem + P.jump);   // [nr + 1][2 w], before the heads are written
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
    stage_words(reinterpret_cast<const uint8_t*>(frames + (img * h + (size_t)(r0 - have)) * w), nsrc, srcb,
                [off](int j) { return off + j; });
    if (!have)
      for (int i = t; i < w2; i += PT) srcb[i] = 0;
    mark_start(mark, len);
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

  const int C = (len + PT - 1) / PT;
  const int cs = t * C < len ? t * C : len, ce = (t + 1) * C < len ? (t + 1) * C : len;
  match_stage<NC>(a, len, cd, cs, ce, tok, jump);
  chain_stage<PQ>(jump, mark, len);

  // ---- count: the histograms, the fixed form's bits, the extra bits and the Adler-32 sums
  {
    uint32_t fbits = 0, xbits = 0, s1 = 0, s2 = 0;
    for (int i = cs; i < ce; ++i) {
      const uint32_t v = a[i];
      s1 += v;
      s2 += (uint32_t)(len - i) * v;
      if (marked(mark, i)) {
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
    add_adler(S.acc, s1, s2);
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
      if (marked(mark, i)) {
        const uint32_t tk = tok[i];
        int n;
        if (form == R::FORM_FIXED) n = tk ? mppng::match_bits((int)(tk & 0x1ffu), cd[tk >> 9]) : mppng::literal_bits(a[i]);
        else (void)dynamic_token(T, tk, cd[tk >> 9], a[i], &n);
        bits += (uint32_t)n;
      }
  uint32_t token_bits;
  const uint32_t bit0 = block_scan(scan, bits, &token_bits);

  // ---- emit
  const int zh = k == 0 ? mppng::ZLIB_HEAD_BYTES : 0;
  const int dlen = zh + (form == R::FORM_FIXED ? fixed_b : form == R::FORM_STORED ? stored_b : dynamic_b);
  const uint32_t last = k == nb - 1 ? 1u : 0u;
  clear_image(image, dlen);
  uint8_t* ib = reinterpret_cast<uint8_t*>(image);
  const int d0 = 8 + zh;                                       // the deflate bytes' place
  if (form == R::FORM_STORED) {
    emit_stored(ib, d0, dlen, a, len, last);
  } else {
    const uint32_t head_bits = form == R::FORM_FIXED ? 0u : plan.header_bits;
    const uint32_t base = 8u * d0 + mppng::BLOCK_HEAD_BITS + head_bits;
    uint32_t bit = base + bit0;
    for (int i = cs; i < ce; ++i) {
      if (marked(mark, i)) {
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
  chunk_head(ib, dlen, zh);
  chunk_crc(ib, dlen, S.crc, S.acc);
  write_slot(work + (img * nb + k) * slot, image, dlen, S.acc, (int64_t)(h - (r0 + nr)) * rb);
}

}  // namespace

size_t png16_work_bytes(int64_t n, int h, int w) {
  return (size_t)n * R::band_count(h, w) * slot_bytes(R::band_len(h, w, 0));
}

hipError_t launch_png16_encode(const uint16_t* frames, int64_t n, int h, int w, uint8_t* out, int64_t out_stride,
                               int64_t* sizes, void* work, hipStream_t st) {
  const int rows = R::band_rows(w);
  return launch_band_and_file<mppng16h::Gray16>(png16_band_kernel, (size_t)lds_plan(h < rows ? h : rows, w).total * 4, frames,
                                                n, h, w, R::band_count(h, w), slot_bytes(R::band_len(h, w, 0)), out,
                                                out_stride, sizes, work, st);
}

}  // namespace mp
