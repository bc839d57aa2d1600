// PNG files from RGB pictures on the device (mp_png_encode_dev).  The bytes are png_rule.hpp's, the
// same the host encoder of png_rgb_host.hpp writes.  The band pipeline is png_band_dev.hpp's; what this
// file adds is the RGB rule's own:
//     stage    the filter byte 0 put in front of every row.
//     bits     the fixed form's token bits -> its bytes against the stored form's (png_rule.hpp), ties
//              to fixed.
//     emit     the fixed form: a token is at most 31 bits, two words.
#include "png_band_dev.hpp"
#include "png_rgb_host.hpp"

namespace mp {

namespace {

constexpr int PQ = (mppng::MAX_BAND + PT - 1) / PT;            // positions a thread at most (49)
constexpr int NC = mppng::MAX_CANDS;

// the LDS plan of a band of len bytes: one spare word behind the image (a token's second word)
__host__ __device__ constexpr BandLds lds_plan(int len) { return band_lds<NC>(len, 1, 0); }
static_assert(lds_plan(mppng::band_len(424, 512, 0)).total == 9850, "the plan of a 424 x 512 picture's bands");

__global__ __launch_bounds__(PT) void png_band_kernel(const uint8_t* __restrict__ rgb, int h, int w,
                                                      uint8_t* __restrict__ work, size_t slot) {
  extern __shared__ uint32_t smem[];
  __shared__ uint32_t s_crc[256];
  __shared__ uint32_t s_acc[4];      // token bits' total, CRC, Adler s1, s2

  const int t = threadIdx.x, k = blockIdx.x, nb = gridDim.x;
  const size_t img = blockIdx.y;
  const int rb = mppng::row_bytes(w), rows = mppng::band_rows(w);
  const int r0 = k * rows, nr = (h - r0 < rows) ? h - r0 : rows, len = nr * rb;
  const BandLds P = lds_plan(len);
  uint8_t* a = reinterpret_cast<uint8_t*>(smem + P.raw);
  uint16_t* tok = reinterpret_cast<uint16_t*>(smem + P.tok);
  uint16_t* jump = reinterpret_cast<uint16_t*>(smem + P.jump);
  uint32_t* scan = smem + P.jump;    // [PT], after the chain
  uint32_t* image = smem + P.jump;   // the chunk, after the scan
  uint32_t* mark = smem + P.mark;

  int cd[NC];
  mppng::cands(w, cd);

  // ---- stage
  s_crc[t] = mppng::crc_table_entry((uint32_t)t);
  if (t < 4) s_acc[t] = 0;
  {
    const int w3 = 3 * w;
    stage_words(rgb + (img * h + r0) * (size_t)w3, nr * w3, a, [w3](int j) { return j + j / w3 + 1; });
    for (int r = t; r < nr; r += PT) a[r * rb] = 0;
    mark_start(mark, len);
  }
  __syncthreads();

  const int C = (len + PT - 1) / PT;
  const int cs = t * C < len ? t * C : len, ce = (t + 1) * C < len ? (t + 1) * C : len;
  match_stage<NC>(a, len, cd, cs, ce, tok, jump);
  chain_stage<PQ>(jump, mark, len);

  // ---- bits; and the band's Adler-32 sums on the way
  uint32_t bits = 0, s1 = 0, s2 = 0;
  for (int i = cs; i < ce; ++i) {
    const uint32_t v = a[i];
    s1 += v;
    s2 += (uint32_t)(len - i) * v;
    if (marked(mark, i)) {
      const uint32_t tk = tok[i];
      bits += tk ? mppng::match_bits((int)(tk & 0x1ffu), cd[tk >> 9]) : mppng::literal_bits((int)v);
    }
  }
  add_adler(s_acc, s1, s2);
  uint32_t token_bits;
  const uint32_t bit0 = block_scan(scan, bits, &token_bits);

  // ---- emit
  const int zh = k == 0 ? mppng::ZLIB_HEAD_BYTES : 0;
  const int fixed_b = mppng::fixed_band_bytes(token_bits), stored_b = mppng::stored_band_bytes(len);
  const bool fixed = fixed_b <= stored_b;
  const int dlen = zh + (fixed ? fixed_b : stored_b);        // the chunk's data bytes
  const uint32_t last = k == nb - 1 ? 1u : 0u;
  clear_image(image, dlen);
  uint8_t* ib = reinterpret_cast<uint8_t*>(image);
  const int d0 = 8 + zh;                                       // the deflate bytes' place
  if (fixed) {
    const uint32_t base = 8u * d0 + mppng::BLOCK_HEAD_BITS;
    uint32_t bit = base + bit0;
    for (int i = cs; i < ce; ++i) {
      if (marked(mark, i)) {
        const uint32_t tk = tok[i];
        int n;
        const uint32_t v = tk ? mppng::match_code((int)(tk & 0x1ffu), cd[tk >> 9], &n) : mppng::fixed_code(a[i], &n);
        or_bits(image, bit, v, n);
        bit += n;
      }
    }
    if (t == 0) {
      or_bits(image, 8u * d0, mppng::FIXED_HEAD, mppng::BLOCK_HEAD_BITS);
      or_bits(image, base + token_bits + mppng::EOB_BITS, last, mppng::BLOCK_HEAD_BITS);
      or_bits(image, 8u * (uint32_t)(8 + dlen - 2), 0xffffu, 16);
    }
  } else {
    emit_stored(ib, d0, dlen, a, len, last);
  }
  chunk_head(ib, dlen, zh);
  chunk_crc(ib, dlen, s_crc, s_acc);
  write_slot(work + (img * nb + k) * slot, image, dlen, s_acc, (int64_t)(h - (r0 + nr)) * rb);
}

}  // namespace

size_t png_work_bytes(int64_t n, int h, int w) {
  return (size_t)n * mppng::band_count(h, w) * slot_bytes(mppng::band_len(h, w, 0));
}

hipError_t launch_png_encode(const uint8_t* rgb, int64_t n, int h, int w, uint8_t* out, int64_t out_stride,
                             int64_t* sizes, void* work, hipStream_t st) {
  const int len = mppng::band_len(h, w, 0);
  return launch_band_and_file<mppngh::Rgb8>(png_band_kernel, (size_t)lds_plan(len).total * 4, rgb, n, h, w,
                                            mppng::band_count(h, w), slot_bytes(len), out, out_stride, sizes, work, st);
}

}  // namespace mp
