// PNG files from RGB pictures on the device (mp_png_encode_dev).  The bytes are png_rule.hpp's, the
// same the host encoder of mp_png.hip writes; this file is how a workgroup arrives at them.
//
//   png_band_kernel   one workgroup of 256 threads per (band, image); the band lives in LDS.
//     stage    the band's source rows are contiguous in rgb: aligned words in, bytes out to LDS with
//              the filter byte 0 put in front of every row.
//     match    thread t owns the positions [t C, (t + 1) C), C = ceil(len / 256).  For a distance d
//              the match length at i is the run of e_d[j] = (j >= d && a[j] == a[j - d]) starting at
//              i, cut at 258: a backward walk of the chunk, r = e_d[i] ? min(r + 1, 258) : 0, started
//              from the run that enters the chunk from the right.  That carry comes from the chunks'
//              heads (the run at a chunk's first position, and whether it fills the chunk), which a
//              first walk leaves in LDS: a thread adds the heads to its right while they are full,
//              at most 258 / C + 1 of them.  The walk keeps every candidate's r in registers, picks
//              the longest (ties: the smallest d) and leaves tok[i] = L | candidate << 9 (0: a
//              literal) and next[i] = i + (L >= 3 ? L : 1).
//     chain    which positions the greedy parse visits: those reachable from 0 along next.  Pointer
//              jumping: after round k, jump[i] = next^(2^k)[i] and the marked set holds every position
//              fewer than 2^k hops from 0; a round marks jump[i] of every marked i and squares jump
//              (all reads, a barrier, all writes).  At most ceil(log2 len) rounds; a round that marks
//              nothing new ends the loop (a band of long matches has few hops).  A mark seen early,
//              in the round that sets it, marks a reachable position too, so the final set is the same.
//     bits     a chunk's token bits, an exclusive scan over the 256 chunks, the total -> the fixed
//              form's bytes against the stored form's (png_rule.hpp), ties to fixed.
//     emit     the whole IDAT chunk -- length, "IDAT", 78 01 in band 0, the block(s), the CRC -- is
//              built in LDS over the jump array, which is dead by then.  Tokens enter with atomicOr
//              (distinct bits of a zeroed image: no order shows); a token is at most 31 bits, two
//              words.  The stored form is byte stores.
//     crc      thread t takes the bytes [E - (256 - t) P, E - (255 - t) P) of type + data, P =
//              ceil(bytes / 256), E their end, with the CRC table in LDS; its CRC times x^(8 bytes
//              after it) mod P (crc_shift, crc_mul) is its share, and the chunk's CRC is the XOR of
//              the shares (crc32_combine, unrolled).
//     out      the chunk as words to the band's slot of `work`, behind its header: the chunk's bytes,
//              and the band's two Adler-32 terms.
//   png_file_kernel   one workgroup per (band, image) again: the sizes of the bands before it summed
//              give the chunk's place in the file; its bytes are copied there (any alignment, byte
//              stores: a file is a few percent of the raw picture).  Band 0 also writes the signature
//              and IHDR; the last band sums the Adler terms and writes the Adler-32's IDAT, IEND and
//              sizes[image].
//
// Nothing is written outside out[i][0 .. sizes[i]), sizes and work.  Integer adds, ORs and XORs only:
// no result depends on the order in which atomics arrive.
#include "mp_kernels.hpp"
#include "png_rule.hpp"

namespace mp {

namespace {

constexpr int PT = 256;                                        // threads of a workgroup
constexpr int PQ = (mppng::MAX_BAND + PT - 1) / PT;            // positions a thread at most (49)
constexpr int NC = mppng::MAX_CANDS;
constexpr int SLOT_HEAD = 16;                                  // chunk bytes, Adler s1, Adler B term, 0

struct BandLds {
  int raw, tok, jump, mark, total;   // word offsets
};
// the LDS plan of a band of len bytes.  The jump region also holds, at other times, the chunks' heads
// (NC * 256 uint16), the scan (256 words) and the chunk's image.
__host__ __device__ inline BandLds band_lds(int len) {
  BandLds L;
  L.raw = 0;
  L.tok = L.raw + (len + 3) / 4 + 1;
  L.jump = L.tok + (len + 1) / 2;
  int jw = (len + 1 + 1) / 2;
  const int img = (mppng::band_chunk_max(len, true) + 3) / 4 + 1;
  if (jw < img) jw = img;
  if (jw < NC * PT / 2) jw = NC * PT / 2;
  L.mark = L.jump + jw;
  L.total = L.mark + (len + 31) / 32;
  return L;
}
static_assert(NC * PT / 2 >= PT, "the scan fits where the heads do");

size_t slot_bytes(int h, int w) {
  return SLOT_HEAD + (size_t)((mppng::band_chunk_max(mppng::band_len(h, w, 0), true) + 15) / 16) * 16;
}

__device__ __forceinline__ void or_bits(uint32_t* img, uint32_t bit, uint32_t v, int n) {
  const uint32_t wd = bit >> 5, sh = bit & 31u;
  atomicOr(&img[wd], v << sh);
  if (sh + n > 32) atomicOr(&img[wd + 1], v >> (32 - sh));
}

__device__ __forceinline__ void store_be32(uint8_t* p, uint32_t v) {
  p[0] = (uint8_t)(v >> 24);
  p[1] = (uint8_t)(v >> 16);
  p[2] = (uint8_t)(v >> 8);
  p[3] = (uint8_t)v;
}

// the CRC-32 of a few bytes without a table
__device__ inline uint32_t crc_small(const uint8_t* p, int n) {
  uint32_t c = 0xffffffffu;
  for (int i = 0; i < n; ++i) c = mppng::crc_table_entry((c ^ p[i]) & 0xffu) ^ (c >> 8);
  return ~c;
}

__global__ __launch_bounds__(PT) void png_band_kernel(const uint8_t* __restrict__ rgb, int h, int w,
                                                      uint8_t* __restrict__ work, size_t slot) {
  extern __shared__ uint32_t smem[];
  __shared__ uint32_t s_crc[256];
  __shared__ uint32_t s_acc[4];      // token bits' total, CRC, Adler s1, s2

  const int t = threadIdx.x, k = blockIdx.x, nb = gridDim.x;
  const size_t img = blockIdx.y;
  const int rb = mppng::row_bytes(w), rows = mppng::band_rows(w);
  const int r0 = k * rows, nr = (h - r0 < rows) ? h - r0 : rows, len = nr * rb;
  const BandLds P = band_lds(len);
  uint8_t* a = reinterpret_cast<uint8_t*>(smem + P.raw);
  uint16_t* tok = reinterpret_cast<uint16_t*>(smem + P.tok);
  uint16_t* jump = reinterpret_cast<uint16_t*>(smem + P.jump);
  uint16_t* head = jump;             // [NC][PT], before jump is written
  uint32_t* scan = smem + P.jump;    // [PT], after the chain
  uint32_t* image = smem + P.jump;   // the chunk, after the scan
  uint32_t* mark = smem + P.mark;

  int cd[NC];
  mppng::cands(w, cd);

  // ---- stage
  s_crc[t] = mppng::crc_table_entry((uint32_t)t);
  if (t < 4) s_acc[t] = 0;
  {
    const int w3 = 3 * w, nsrc = nr * w3;
    const uint8_t* src = rgb + (img * h + r0) * (size_t)w3;
    const int mis = (int)(reinterpret_cast<uintptr_t>(src) & 3);
    const uint32_t* srcw = reinterpret_cast<const uint32_t*>(src - mis);
    const int nw = (mis + nsrc + 3) / 4;
    for (int i = t; i < nw; i += PT) {
      const uint32_t v = srcw[i];
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const int j = 4 * i + b - mis;
        if (j >= 0 && j < nsrc) a[j + j / w3 + 1] = (uint8_t)(v >> (8 * b));
      }
    }
    for (int r = t; r < nr; r += PT) a[r * rb] = 0;
    for (int i = t; i < (len + 31) / 32; i += PT) mark[i] = (i == 0) ? 1u : 0u;
  }
  __syncthreads();

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
    for (int u = t + 1; u < PT && cr < mppng::MAX_MATCH; ++u) {
      const uint32_t hv = head[c * PT + u];
      cr += (int)(hv & 0x7fffu);
      if (!(hv >> 15)) break;
    }
    run[c] = cr < mppng::MAX_MATCH ? cr : mppng::MAX_MATCH;
  }
  __syncthreads();                   // the heads are read: jump may be written
  for (int i = ce - 1; i >= cs; --i) {
    const uint8_t v = a[i];
    int bl = 0, bd = 0, bc = 0;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const int d = cd[c];
      const bool eq = i >= d && v == a[i - d];
      run[c] = eq ? (run[c] + 1 < mppng::MAX_MATCH ? run[c] + 1 : mppng::MAX_MATCH) : 0;
      if (run[c] > bl || (run[c] == bl && d < bd)) bl = run[c], bd = d, bc = c;
    }
    const bool m = bl >= mppng::MIN_MATCH;
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
    // a round that marks nothing new found the marked set closed under jump, and it holds every
    // position fewer than `step` hops from 0: it is the whole chain
    if (!__syncthreads_or(added)) break;
#pragma unroll
    for (int q = 0; q < PQ; ++q) {
      const int i = t + PT * q;
      if (i < len) jump[i] = nj[q];
    }
    __syncthreads();
  }

  // ---- bits; and the band's Adler-32 sums on the way
  uint32_t bits = 0, s1 = 0, s2 = 0;
  for (int i = cs; i < ce; ++i) {
    const uint32_t v = a[i];
    s1 += v;
    s2 += (uint32_t)(len - i) * v;
    if ((mark[i >> 5] >> (i & 31)) & 1u) {
      const uint32_t tk = tok[i];
      bits += tk ? mppng::match_bits((int)(tk & 0x1ffu), cd[tk >> 9]) : mppng::literal_bits((int)v);
    }
  }
  scan[t] = bits;                    // jump is dead from here
  atomicAdd(&s_acc[2], s1 % mppng::ADLER_MOD);
  atomicAdd(&s_acc[3], s2 % mppng::ADLER_MOD);
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
  const int fixed_b = mppng::fixed_band_bytes(token_bits), stored_b = mppng::stored_band_bytes(len);
  const bool fixed = fixed_b <= stored_b;
  const int dlen = zh + (fixed ? fixed_b : stored_b);        // the chunk's data bytes
  const int csz = mppng::CHUNK_BYTES + dlen;
  const int imgw = (csz + 3) / 4;
  const uint32_t last = k == nb - 1 ? 1u : 0u;
  for (int i = t; i < imgw; i += PT) image[i] = 0;
  __syncthreads();
  uint8_t* ib = reinterpret_cast<uint8_t*>(image);
  const int d0 = 8 + zh;                                       // the deflate bytes' place
  if (fixed) {
    const uint32_t base = 8u * d0 + mppng::BLOCK_HEAD_BITS;
    uint32_t bit = base + bit0;
    for (int i = cs; i < ce; ++i) {
      if ((mark[i >> 5] >> (i & 31)) & 1u) {
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
      for (int i = b0; i < b1; ++i) c = s_crc[(c ^ ib[i]) & 0xffu] ^ (c >> 8);
      atomicXor(&s_acc[1], mppng::crc_mul(mppng::crc_shift((uint32_t)(E - b1)), ~c));
    }
  }
  __syncthreads();
  if (t == 0) store_be32(ib + 8 + dlen, s_acc[1]);
  __syncthreads();

  // ---- out
  uint32_t* dst = reinterpret_cast<uint32_t*>(work + (img * nb + k) * slot);
  if (t == 0) {
    const int64_t after = (int64_t)(h - (r0 + nr)) * rb;
    const uint32_t m1 = s_acc[2] % mppng::ADLER_MOD, m2 = s_acc[3] % mppng::ADLER_MOD;
    dst[0] = (uint32_t)csz;
    dst[1] = m1;
    dst[2] = mppng::adler_b_term(m1, m2, after);
    dst[3] = 0;
  }
  for (int i = t; i < imgw; i += PT) dst[SLOT_HEAD / 4 + i] = image[i];
}

__global__ __launch_bounds__(PT) void png_file_kernel(const uint8_t* __restrict__ work, size_t slot, int h, int w,
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
    b[24] = 8, b[25] = 2, b[26] = 0, b[27] = 0, b[28] = 0;
    store_be32(b + 29, crc_small(b + 12, 17));
    for (int i = 0; i < mppng::HEAD_BYTES; ++i) file[i] = b[i];
  }
  if (is_last && t == 0) {
    const uint64_t N = (uint64_t)h * mppng::row_bytes(w);
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

size_t png_work_bytes(int64_t n, int h, int w) { return (size_t)n * mppng::band_count(h, w) * slot_bytes(h, w); }

hipError_t launch_png_encode(const uint8_t* rgb, int64_t n, int h, int w, uint8_t* out, int64_t out_stride,
                             int64_t* sizes, void* work, hipStream_t st) {
  const int nb = mppng::band_count(h, w);
  const size_t slot = slot_bytes(h, w);
  const size_t lds = (size_t)band_lds(mppng::band_len(h, w, 0)).total * 4;
  const dim3 grid((unsigned)nb, (unsigned)n);
  hipLaunchKernelGGL(png_band_kernel, grid, dim3(PT), lds, st, rgb, h, w, static_cast<uint8_t*>(work), slot);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(png_file_kernel, grid, dim3(PT), 0, st, static_cast<const uint8_t*>(work), slot, h, w, out,
                     out_stride, sizes);
  return hipGetLastError();
}

}  // namespace mp
