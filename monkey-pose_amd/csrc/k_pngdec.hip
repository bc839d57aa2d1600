// PNG files to pixels on the device (include/monkeypose_pngdec.h).  The rule is pngdec_rule.hpp; the
// three kernels here run it through policies of their own, one file a workgroup, on the caller's
// stream.  A file's slot in `work` carries it from kernel to kernel: a 16-byte head (its status so
// far, the length of its zlib stream), the zlib stream, the raw stream.
//
//   pngdec_parse_kernel     256 threads a file.  The chunk walk (mppd::parse_file) is the same in every
//                           thread: all read the same header bytes.  A chunk's CRC is computed in 256
//                           shares -- thread t takes the t-th ceil(bytes / 256) bytes with the table in
//                           LDS, its CRC times x^(8 bytes after it) (png_rule.hpp's crc_shift / crc_mul)
//                           is its share, and the XOR of the shares is the chunk's CRC -- and an IDAT's
//                           payload is copied to the slot's zlib stream by all threads together.
//   pngdec_inflate_kernel   one wave a file.  Every lane runs mppd::inflate's symbol loop on the same
//                           values (the bit buffer and table entries are made scalar with
//                           readfirstlane); the lanes share the work around it:
//                             input    refilled into LDS 4 KiB at a time, a dword a lane, zero past the end
//                             tables   the lead lane counts and sorts, the lanes fill the direct table
//                                      (11 bits; longer codes go bit by bit through count / symbol)
//                             output   a circular window of 64 KiB in LDS: a literal is one byte from
//                                      lane 0, a match is copied by the lanes together, byte j from
//                                      pos - dist + j mod dist (the dist = 1 run among them: all sources
//                                      lie before the match)
//                             flush    every 16 KiB the window's oldest unflushed part goes to the raw
//                                      stream in 16-byte pieces, a piece a lane; the two Adler-32 terms
//                                      are summed from the flushed pieces (each byte weighted by the
//                                      bytes that follow it, as the encoder's s1 / B terms are) and
//                                      added up over the lanes once at the end -- integers, so the order
//                                      does not matter
//   pngdec_unfilter_kernel  256 threads a file, a skewed wavefront: thread r owns row r of a pass of
//                           256 rows and runs one segment of 12 bytes (4 pixels of RGB, 6 of gray16)
//                           behind row r - 1.  It keeps a and c in registers and takes b from the
//                           segment the thread above left in LDS one step earlier (double-buffered,
//                           one barrier a step); the last row of a pass is kept in LDS for the next.
//                           Before that it checks the filter bytes, zero-fills a failed file's image and
//                           writes status[i].  Finished pixels go to `out`: uint16 from the two
//                           big-endian bytes, uint8 otherwise.
//
// Bounds: parse_file reads inside [0, size) and writes at most `size` bytes of the zlib stream;
// the inflate input is masked at zlen; literals and matches are checked against the expected
// length by mppd::inflate before they are written, and the window index is masked; a flush writes
// whole 16-byte pieces inside the slot's raw stream, which is rounded up to 16.
#include <hip/hip_runtime.h>

#include "mp_kernels.hpp"
#include "png_rule.hpp"
#include "pngdec_rule.hpp"

namespace mp {

namespace {

constexpr int PT = 256;              // threads of the parse kernel
constexpr int WAVE = 64;
constexpr int WIN = 65536;           // the window: 32 KiB of history, a flush unit and a match, rounded up
constexpr int FLUSH = 16384;
constexpr int IN_BYTES = 4096;
constexpr int UNF_ROWS = 256;        // rows of a pass of the unfilter kernel (its threads)
constexpr int SEG = 12;              // bytes a thread runs behind the row above: whole pixels at bpp 1, 2, 3
static_assert(mppd::MAX_HW * 3 % SEG == 0, "the carried row is whole segments");
static_assert(32768 + FLUSH + 258 <= WIN, "history, the unflushed part and one match fit the window");

struct Slot {
  int32_t* head;
  uint8_t* z;
  uint8_t* raw;
};
__device__ inline Slot slot_of(uint8_t* work, size_t i, int h, int w, int format, int64_t file_stride) {
  uint8_t* s = work + i * (size_t)mppd::slot_bytes(h, w, format, file_stride);
  return {reinterpret_cast<int32_t*>(s), s + mppd::SLOT_HEAD, s + mppd::SLOT_HEAD + mppd::round16(file_stride)};
}

// ---- parse ---------------------------------------------------------------------------------------
struct DevParse {
  const uint32_t* tab;
  uint32_t* acc;
  int t;
  __device__ uint32_t crc(const uint8_t* p, int64_t n) {
    if (t == 0) *acc = 0;
    __syncthreads();
    const int64_t pc = (n + PT - 1) / PT, b0 = t * pc, b1 = b0 + pc < n ? b0 + pc : n;
    if (b1 > b0) {
      uint32_t c = 0xffffffffu;
      for (int64_t i = b0; i < b1; ++i) c = tab[(c ^ p[i]) & 0xffu] ^ (c >> 8);
      atomicXor(acc, mppng::crc_mul(mppng::crc_shift((uint32_t)(n - b1)), ~c));
    }
    __syncthreads();
    const uint32_t r = *acc;
    __syncthreads();
    return r;
  }
  __device__ void copy(uint8_t* dst, const uint8_t* src, int64_t n) {
    for (int64_t i = t; i < n; i += PT) dst[i] = src[i];
  }
};

__global__ __launch_bounds__(PT) void pngdec_parse_kernel(const uint8_t* __restrict__ files, int64_t file_stride,
                                                          const int64_t* __restrict__ sizes, int h, int w, int format,
                                                          uint8_t* __restrict__ work) {
  __shared__ uint32_t s_tab[256];
  __shared__ uint32_t s_acc;
  const int t = threadIdx.x;
  const size_t i = blockIdx.x;
  s_tab[t] = mppd::crc_table_entry((uint32_t)t);
  __syncthreads();
  int64_t size = sizes[i];
  if (size < 0 || size > file_stride) size = 0;
  const Slot s = slot_of(work, i, h, w, format, file_stride);
  DevParse io{s_tab, &s_acc, t};
  int64_t zlen = 0;
  const int st = mppd::parse_file(files + i * (size_t)file_stride, size, h, w, format, s.z, &zlen, io);
  if (t == 0) {
    s.head[0] = st;
    s.head[1] = (int32_t)zlen;       // at most file_stride <= 2^30
  }
}

// ---- inflate -------------------------------------------------------------------------------------
struct DevInflate {
  const uint8_t* z;
  int64_t zlen;
  uint8_t* raw;
  int64_t expect;
  uint8_t* win;
  uint32_t* in;
  mppd::Tables* T;
  unsigned long long* red;
  int ln;
  int64_t in_base, pos, flushed;
  unsigned long long s1, s2;
  uint32_t adler_;

  __device__ int lane() const { return ln; }
  __device__ int lanes() const { return WAVE; }
  __device__ bool lead() const { return ln == 0; }
  __device__ void sync() { __syncthreads(); }
  __device__ uint32_t uni(uint32_t v) const { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
  __device__ mppd::Tables& tables() { return *T; }

  __device__ uint32_t word(int64_t i) {
    if (i >= in_base + IN_BYTES) {   // the stream is read front to back
      __syncthreads();
      in_base = i;
      for (int k = ln; k < IN_BYTES / 4; k += WAVE) {
        const int64_t off = i + 4 * (int64_t)k;
        uint32_t v = 0;
        if (off < zlen) {
          v = *reinterpret_cast<const uint32_t*>(z + off);
          if (zlen - off < 4) v &= (1u << (8 * (int)(zlen - off))) - 1u;
        }
        in[k] = v;
      }
      __syncthreads();
    }
    return uni(in[(i - in_base) >> 2]);
  }

  __device__ void lit(uint8_t v) {
    if (ln == 0) win[pos & (WIN - 1)] = v;
    pos += 1;
    if (pos - flushed >= FLUSH) flush_unit();
  }
  __device__ void match(int dist, int len) {
    __syncthreads();                 // the bytes before the match are in the window
    const int p = (int)(pos & (WIN - 1));
    for (int j = ln; j < len; j += WAVE) {
      const int k = j < dist ? j : j % dist;
      win[(p + j) & (WIN - 1)] = win[(p - dist + k) & (WIN - 1)];
    }
    pos += len;
    if (pos - flushed >= FLUSH) flush_unit();
  }
  // the window's bytes [a, b) -> the raw stream, a a multiple of 16, b - a at most FLUSH + 258
  __device__ void flush_range(int64_t a, int64_t b) {
    const int pieces = (int)((b - a + 15) >> 4);
    for (int q = ln; q < pieces; q += WAVE) {
      const int64_t i0 = a + 16 * (int64_t)q;
      const uint4 v = *reinterpret_cast<const uint4*>(win + (i0 & (WIN - 1)));
      uint32_t d[4] = {v.x, v.y, v.z, v.w};
      const int valid = b - i0 < 16 ? (int)(b - i0) : 16;
      uint32_t p1 = 0, p2 = 0;
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        const uint32_t sh = 8u * (k & 3);
        if (k >= valid) d[k >> 2] &= ~(0xffu << sh);
        const uint32_t byte = (d[k >> 2] >> sh) & 0xffu;
        p1 += byte;
        p2 += (16u - k) * byte;
      }
      *reinterpret_cast<uint4*>(raw + i0) = make_uint4(d[0], d[1], d[2], d[3]);
      // byte k of the piece is followed by expect - (i0 + k) bytes, itself included: tail + (16 - k)
      int64_t tail = (expect - i0 - 16) % (int64_t)mppd::ADLER_MOD;
      if (tail < 0) tail += mppd::ADLER_MOD;
      s1 += p1;
      s2 += (unsigned long long)tail * p1 + p2;
    }
  }
  __device__ void flush_unit() {
    __syncthreads();
    flush_range(flushed, flushed + FLUSH);
    flushed += FLUSH;
    __syncthreads();
  }
  __device__ void finish() {
    __syncthreads();
    flush_range(flushed, pos);
    flushed = pos;
    red[ln] = s1;
    red[WAVE + ln] = s2 % mppd::ADLER_MOD;
    __syncthreads();
    unsigned long long a = 0, b = 0;
    for (int k = 0; k < WAVE; ++k) {
      a += red[k];
      b += red[WAVE + k];
    }
    const uint32_t A = (uint32_t)((1u + a) % mppd::ADLER_MOD);
    const uint32_t B = (uint32_t)(((unsigned long long)expect + b) % mppd::ADLER_MOD);
    adler_ = (B << 16) | A;
  }
  __device__ uint32_t adler() const { return adler_; }
};

__global__ __launch_bounds__(WAVE) void pngdec_inflate_kernel(uint8_t* __restrict__ work, int h, int w, int format,
                                                              int64_t file_stride) {
  __shared__ __attribute__((aligned(16))) uint8_t s_win[WIN];
  __shared__ uint32_t s_in[IN_BYTES / 4];
  __shared__ mppd::Tables s_T;
  __shared__ unsigned long long s_red[2 * WAVE];
  const Slot s = slot_of(work, blockIdx.x, h, w, format, file_stride);
  if (s.head[0] != 0) return;        // the same for every lane
  DevInflate io;
  io.z = s.z;
  io.zlen = s.head[1];
  io.raw = s.raw;
  io.expect = mppd::raw_bytes(h, w, format);
  io.win = s_win;
  io.in = s_in;
  io.T = &s_T;
  io.red = s_red;
  io.ln = threadIdx.x;
  io.in_base = -(int64_t)IN_BYTES;
  io.pos = io.flushed = 0;
  io.s1 = io.s2 = 0;
  io.adler_ = 0;
  const int st = mppd::inflate(io, io.zlen, io.expect);
  if (threadIdx.x == 0) s.head[0] = st;
}

// ---- unfilter ------------------------------------------------------------------------------------
template <int BPP>
__global__ __launch_bounds__(UNF_ROWS) void pngdec_unfilter_kernel(uint8_t* __restrict__ work, int h, int w, int format,
                                                                   int64_t file_stride, void* __restrict__ out,
                                                                   int32_t* __restrict__ status) {
  __shared__ uint8_t s_buf[2][UNF_ROWS][SEG];
  __shared__ uint8_t s_carry[mppd::MAX_HW * 3];
  const int t = threadIdx.x, rb = w * BPP;
  const size_t i = blockIdx.x;
  const Slot s = slot_of(work, i, h, w, format, file_stride);
  const uint8_t* raw = s.raw;
  uint8_t* o8 = static_cast<uint8_t*>(out) + i * (size_t)h * rb;
  uint16_t* o16 = static_cast<uint16_t*>(out) + i * (size_t)h * w;
  int st = s.head[0];
  if (st == 0) {
    int bad = 0;
    for (int r = t; r < h; r += UNF_ROWS) bad |= raw[(int64_t)r * (1 + rb)] > 4;
    if (__syncthreads_or(bad)) st = mppd::ST_FILTER;
  }
  if (t == 0) status[i] = st;
  if (st) {
    if (BPP == 2)
      for (int64_t k = t; k < (int64_t)h * w; k += UNF_ROWS) o16[k] = 0;
    else
      for (int64_t k = t; k < (int64_t)h * rb; k += UNF_ROWS) o8[k] = 0;
    return;
  }
  for (int k = t; k < rb; k += UNF_ROWS) s_carry[k] = 0;     // the row above row 0
  __syncthreads();
  const int nseg = (rb + SEG - 1) / SEG;
  for (int r0 = 0; r0 < h; r0 += UNF_ROWS) {
    const int rows = h - r0 < UNF_ROWS ? h - r0 : UNF_ROWS, r = r0 + t;
    const bool active = t < rows, carries = t == UNF_ROWS - 1 && r0 + UNF_ROWS < h;
    const uint8_t* src = raw + (int64_t)(active ? r : r0) * (1 + rb);
    const int ft = src[0];
    src += 1;
    // cur / upv hold the segment behind three bytes of history: a = cur[3 + k - BPP], c = upv[3 + k - BPP]
    uint8_t cur[SEG + 3], upv[SEG + 3];
    for (int q = 0; q < 3; ++q) cur[q] = upv[q] = 0;
    for (int step = 0; step < nseg + rows - 1; ++step) {
      const int seg = step - t;
      if (active && seg >= 0 && seg < nseg) {
        const int base = seg * SEG, len = rb - base < SEG ? rb - base : SEG;
        const uint8_t* up = t == 0 ? s_carry + base : s_buf[(step - 1) & 1][t - 1];
        uint8_t* mine = s_buf[step & 1][t];
#pragma unroll
        for (int k = 0; k < SEG; ++k) {
          if (k < len) {
            const uint8_t b = up[k];
            upv[3 + k] = b;
            const uint8_t v = mppd::unfilter_byte(ft, src[base + k], cur[3 + k - BPP], b, upv[3 + k - BPP]);
            cur[3 + k] = v;
            mine[k] = v;
            if (BPP == 2) {
              if (k & 1) o16[(size_t)r * w + ((base + k) >> 1)] = (uint16_t)((cur[3 + k - 1] << 8) | v);
            } else {
              o8[(size_t)r * rb + base + k] = v;
            }
          }
        }
        if (carries) {
#pragma unroll
          for (int k = 0; k < SEG; ++k)
            if (k < len) s_carry[base + k] = cur[3 + k];
        }
        // a segment that has a successor is full: its last three bytes are the next one's history
        for (int q = 0; q < 3; ++q) {
          cur[q] = cur[SEG + q];
          upv[q] = upv[SEG + q];
        }
      }
      __syncthreads();
    }
  }
}

}  // namespace

size_t pngdec_work_bytes(int64_t n, int h, int w, int format, int64_t file_stride) {
  return (size_t)n * (size_t)mppd::slot_bytes(h, w, format, file_stride);
}

hipError_t launch_png_decode(const uint8_t* files, int64_t file_stride, const int64_t* sizes, int64_t n, int h, int w,
                             int format, void* out, int32_t* status, void* work, hipStream_t st) {
  uint8_t* wk = static_cast<uint8_t*>(work);
  const dim3 grid((unsigned)n);
  hipLaunchKernelGGL(pngdec_parse_kernel, grid, dim3(PT), 0, st, files, file_stride, sizes, h, w, format, wk);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(pngdec_inflate_kernel, grid, dim3(WAVE), 0, st, wk, h, w, format, file_stride);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  switch (mppd::bpp(format)) {
    case 1:
      hipLaunchKernelGGL(pngdec_unfilter_kernel<1>, grid, dim3(UNF_ROWS), 0, st, wk, h, w, format, file_stride, out,
                         status);
      break;
    case 2:
      hipLaunchKernelGGL(pngdec_unfilter_kernel<2>, grid, dim3(UNF_ROWS), 0, st, wk, h, w, format, file_stride, out,
                         status);
      break;
    default:
      hipLaunchKernelGGL(pngdec_unfilter_kernel<3>, grid, dim3(UNF_ROWS), 0, st, wk, h, w, format, file_stride, out,
                         status);
  }
  return hipGetLastError();
}

}  // namespace mp
