// The band pipeline of the PNG encoders on the device, stated once for the RGB kernels (k_png.hip) and the
// 16-bit ones (k_png16.hip).  The bytes are the rule's (png_rule.hpp, png16_rule.hpp), the same the host
// encoders write; this file is how a workgroup arrives at them.  A band kernel is a sequence of the
// stages below with its format's own stages -- how the raw rows come to be, which forms a band may
// take, the Huffman-coded forms' bits -- in between.
//
//   band kernel       one workgroup of 256 threads per (band, image); the band lives in LDS.
//     stage    the band's source rows are contiguous in memory: aligned words in, bytes out to LDS
//              through the format's map of source byte to LDS byte (stage_words).
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
//     bits     a chunk's token bits in the form the kernel chose, an exclusive scan over the 256
//              chunks, the total (block_scan).
//     emit     the whole IDAT chunk -- length, "IDAT", 78 01 in band 0, the block(s), the CRC -- is
//              built in LDS over the jump array, which is dead by then.  Tokens enter with atomicOr
//              (distinct bits of a zeroed image: no order shows; or_bits, or_bits64).  The stored form
//              is byte stores (emit_stored).
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
// no result depends on the order in which atomics arrive.  All stores are vector stores.
//
// Everything here is in an unnamed namespace: each of the two files has its own copy, as its kernels are
// its own.
#pragma once
#include "mp_kernels.hpp"
#include "png_rule.hpp"

namespace mp {

namespace {

constexpr int PT = 256;                                        // threads of a workgroup
constexpr int SLOT_HEAD = 16;                                  // chunk bytes, Adler s1, Adler B term, 0
// a band kernel's accumulators in static LDS: acc[0] is the kernel's own, then these
constexpr int ACC_CRC = 1, ACC_S1 = 2, ACC_S2 = 3;

struct BandLds {
  int raw, tok, jump, mark, total;   // word offsets
};
// the LDS plan of a band of len bytes and NC candidate distances.  The jump region also holds, at other
// times, the chunks' heads (NC * 256 uint16), the scan (256 words), the chunk's image with `spare`
// words behind it (a token's last word) and whatever else the format keeps there (`least` words).
template <int NC>
__host__ __device__ constexpr BandLds band_lds(int len, int spare, int least) {
  static_assert(NC * PT / 2 >= PT, "the scan fits where the heads do");
  BandLds L{};
  L.raw = 0;
  L.tok = L.raw + (len + 3) / 4 + 1;
  L.jump = L.tok + (len + 1) / 2;
  int jw = (len + 1 + 1) / 2;
  const int img = (mppng::band_chunk_max(len, true) + 3) / 4 + spare;
  if (jw < img) jw = img;
  if (jw < NC * PT / 2) jw = NC * PT / 2;
  if (jw < least) jw = least;
  L.mark = L.jump + jw;
  L.total = L.mark + (len + 31) / 32;
  return L;
}

// a band's slot of `work`: its header and the longest chunk, in whole 16 bytes
constexpr size_t slot_bytes(int band_len_max) {
  return SLOT_HEAD + (size_t)((mppng::band_chunk_max(band_len_max, true) + 15) / 16) * 16;
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

// the CRC-32 of a few bytes without a table
__device__ inline uint32_t crc_small(const uint8_t* p, int n) {
  uint32_t c = 0xffffffffu;
  for (int i = 0; i < n; ++i) c = mppng::crc_table_entry((c ^ p[i]) & 0xffu) ^ (c >> 8);
  return ~c;
}

__device__ __forceinline__ bool marked(const uint32_t* mark, int i) { return (mark[i >> 5] >> (i & 31)) & 1u; }

// ---- stage: nsrc bytes at src (any alignment) as aligned words; byte j goes to dst[map(j)].  No barrier.
template <class Map>
__device__ __forceinline__ void stage_words(const uint8_t* __restrict__ src, int nsrc, uint8_t* dst, Map map) {
  const int mis = (int)(reinterpret_cast<uintptr_t>(src) & 3);
  const uint32_t* srcw = reinterpret_cast<const uint32_t*>(src - mis);
  const int nw = (mis + nsrc + 3) / 4;
  for (int i = threadIdx.x; i < nw; i += PT) {
    const uint32_t v = srcw[i];
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int j = 4 * i + b - mis;
      if (j >= 0 && j < nsrc) dst[map(j)] = (uint8_t)(v >> (8 * b));
    }
  }
}

// the chain starts from position 0: its mark alone is set.  No barrier.
__device__ __forceinline__ void mark_start(uint32_t* mark, int len) {
  for (int i = threadIdx.x; i < (len + 31) / 32; i += PT) mark[i] = (i == 0) ? 1u : 0u;
}

// ---- match: tok and jump of the band a[0 .. len) from this thread's chunk [cs, ce); head is jump's memory
template <int NC>
__device__ __forceinline__ void match_stage(const uint8_t* a, int len, const int (&cd)[NC], int cs, int ce,
                                            uint16_t* tok, uint16_t* jump) {
  const int t = threadIdx.x;
  uint16_t* head = jump;             // [NC][PT], before jump is written
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
}

// ---- chain: marks the positions the greedy parse visits; PQ = positions a thread at most
template <int PQ>
__device__ __forceinline__ void chain_stage(uint16_t* jump, uint32_t* mark, int len) {
  const int t = threadIdx.x;
  for (int step = 1; step < len; step <<= 1) {
    uint16_t nj[PQ];
    int added = 0;
#pragma unroll
    for (int q = 0; q < PQ; ++q) {
      const int i = t + PT * q;
      if (i < len) {
        const int j = jump[i];
        if (j < len && marked(mark, i))
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
}

// a chunk's share of the band's Adler-32 sums into the accumulators.  No barrier.
__device__ __forceinline__ void add_adler(uint32_t* acc, uint32_t s1, uint32_t s2) {
  atomicAdd(&acc[ACC_S1], s1 % mppng::ADLER_MOD);
  atomicAdd(&acc[ACC_S2], s2 % mppng::ADLER_MOD);
}

// ---- bits: the exclusive scan of the chunks' bits over the workgroup -> this chunk's first bit, *total
__device__ __forceinline__ uint32_t block_scan(uint32_t* scan, uint32_t bits, uint32_t* total) {
  const int t = threadIdx.x;
  scan[t] = bits;                    // jump is dead from here
  __syncthreads();
  for (int o = 1; o < PT; o <<= 1) {
    const uint32_t add = t >= o ? scan[t - o] : 0u;
    __syncthreads();
    scan[t] += add;
    __syncthreads();
  }
  const uint32_t bit0 = scan[t] - bits;
  *total = scan[PT - 1];
  __syncthreads();                   // the scan is read: the image may be written
  return bit0;
}

// ---- emit: a chunk of dlen data bytes starts as zeros
__device__ __forceinline__ void clear_image(uint32_t* image, int dlen) {
  for (int i = threadIdx.x; i < (mppng::CHUNK_BYTES + dlen + 3) / 4; i += PT) image[i] = 0;
  __syncthreads();
}

// the band as one stored block at ib + d0, and the empty block that ends the chunk's data.  No barrier.
__device__ __forceinline__ void emit_stored(uint8_t* ib, int d0, int dlen, const uint8_t* a, int len, uint32_t last) {
  for (int i = threadIdx.x; i < len; i += PT) ib[d0 + 5 + i] = a[i];
  if (threadIdx.x == 0) {
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

// the chunk's length and type, and the zlib header in band 0's, once the block is in place
__device__ __forceinline__ void chunk_head(uint8_t* ib, int dlen, int zh) {
  __syncthreads();                   // atomics and byte stores to one word are kept apart by this barrier
  if (threadIdx.x == 0) {
    store_be32(ib, (uint32_t)dlen);
    ib[4] = 'I', ib[5] = 'D', ib[6] = 'A', ib[7] = 'T';
    if (zh) ib[8] = 0x78, ib[9] = 0x01;
  }
  __syncthreads();
}

// ---- crc over the type and the data, the bytes [4, 8 + dlen), written behind them; table: 256 entries in LDS
__device__ __forceinline__ void chunk_crc(uint8_t* ib, int dlen, const uint32_t* table, uint32_t* acc) {
  const int t = threadIdx.x;
  {
    const int nbytes = 4 + dlen, E = 8 + dlen, pc = (nbytes + PT - 1) / PT;
    int b0 = E - (PT - t) * pc, b1 = b0 + pc;
    if (b0 < 4) b0 = 4;
    if (b1 > b0) {
      uint32_t c = 0xffffffffu;
      for (int i = b0; i < b1; ++i) c = table[(c ^ ib[i]) & 0xffu] ^ (c >> 8);
      atomicXor(&acc[ACC_CRC], mppng::crc_mul(mppng::crc_shift((uint32_t)(E - b1)), ~c));
    }
  }
  __syncthreads();
  if (t == 0) store_be32(ib + 8 + dlen, acc[ACC_CRC]);
  __syncthreads();
}

// ---- out: the chunk of dlen data bytes and the band's Adler terms to its slot; `after` raw bytes follow the band
__device__ __forceinline__ void write_slot(uint8_t* __restrict__ slot, const uint32_t* image, int dlen,
                                           const uint32_t* acc, int64_t after) {
  const int t = threadIdx.x, csz = mppng::CHUNK_BYTES + dlen;
  uint32_t* dst = reinterpret_cast<uint32_t*>(slot);
  if (t == 0) {
    const uint32_t m1 = acc[ACC_S1] % mppng::ADLER_MOD, m2 = acc[ACC_S2] % mppng::ADLER_MOD;
    dst[0] = (uint32_t)csz;
    dst[1] = m1;
    dst[2] = mppng::adler_b_term(m1, m2, after);
    dst[3] = 0;
  }
  for (int i = t; i < (csz + 3) / 4; i += PT) dst[SLOT_HEAD / 4 + i] = image[i];
}

// F: the format's IHDR fields BIT_DEPTH and COLOUR_TYPE, and row_bytes(w)
template <class F>
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
    b[24] = F::BIT_DEPTH, b[25] = F::COLOUR_TYPE, b[26] = 0, b[27] = 0, b[28] = 0;
    store_be32(b + 29, crc_small(b + 12, 17));
    for (int i = 0; i < mppng::HEAD_BYTES; ++i) file[i] = b[i];
  }
  if (is_last && t == 0) {
    const uint64_t N = (uint64_t)h * F::row_bytes(w);
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

// the band kernel, then the file kernel, on st: one workgroup per (band, image) each
template <class F, class Src>
hipError_t launch_band_and_file(void (*band_kernel)(const Src*, int, int, uint8_t*, size_t), size_t lds, const Src* src,
                                int64_t n, int h, int w, int nb, size_t slot, uint8_t* out, int64_t out_stride,
                                int64_t* sizes, void* work, hipStream_t st) {
  const dim3 grid((unsigned)nb, (unsigned)n);
  hipLaunchKernelGGL(band_kernel, grid, dim3(PT), lds, st, src, h, w, static_cast<uint8_t*>(work), slot);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(png_file_kernel<F>, grid, dim3(PT), 0, st, static_cast<const uint8_t*>(work), slot, h, w, out,
                     out_stride, sizes);
  return hipGetLastError();
}

}  // namespace

}  // namespace mp
