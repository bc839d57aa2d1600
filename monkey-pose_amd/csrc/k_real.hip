// Preprocessing of recorded camera frames for the attention net (eval_model_on_real_data,
// train_cnn_networks_hgru.py:388-392 and 359) in one pass over the batch:
//
//   im = np.transpose(np.load(f))          raw is stored [w][h]; the net takes [h][w]
//   im[im < 1000] = 10000                  the gate, in the frame's own dtype
//   im[im > 3000] = 10000
//   images = input_image / image_max_depth cast to float32 (the placeholder), one float32 division
//
//   real_transpose_kernel  the stored layout: a 64 x 64 tile goes through LDS.  Reads run along h
//                          (the stored inner dimension, one element a lane: 128 B a wave for uint16,
//                          any alignment), the gated and divided float lands in tile[x][y] with rows
//                          of 65 words, and the stores run along w, a float4 a lane.
//                          Banks: a write is one x row, 32 consecutive words a half wave.  A read is
//                          tile[x + j][y] for 8 x-quads times 4 consecutive y a half wave, word
//                          (4q + j) * 65 + y = 4q + y + const (mod 32): 32 distinct banks.
//   real_plain_kernel      frames already [h][w]: elementwise, four pixels a thread (an 8- or 16-byte
//                          load, a float4 store) when both base pointers allow it, else one.
//
// Both are byte movers (2 + 4 or 4 + 4 bytes a pixel).  The division is the IEEE one: contraction is
// off and the file is built with correctly rounded float32 division (csrc/Makefile), so the result
// has numpy's bits; it is not a multiply by a reciprocal.
#include <type_traits>

#include "mp_kernels.hpp"

#pragma clang fp contract(off)

namespace mp {

namespace {

struct RealGate {
  int on;
  uint32_t ulo, uhi, ufill;   // uint16 frames: integer compares
  float flo, fhi, ffill;      // float32 frames: float32 compares (NaN passes, +-inf is gated)
  float md;                   // f32(image_max_depth)
};

template <typename PX>
__device__ __forceinline__ float real_px(PX v, const RealGate& g) {
  if constexpr (std::is_same<PX, uint16_t>::value) {
    uint32_t x = v;
    if (g.on && (x < g.ulo || x > g.uhi)) x = g.ufill;
    return (float)x / g.md;
  } else {
    float x = v;
    if (g.on && (x < g.flo || x > g.fhi)) x = g.ffill;
    return x / g.md;
  }
}

constexpr int RT = 64;        // tile edge
constexpr int RT_LD = RT + 1; // padded row (words)

// raw [n][W][H] -> out [n][H][W]; blockIdx.x = tile of the frame (x tiles fastest), blockIdx.y = frame
template <typename PX>
__global__ __launch_bounds__(256) void real_transpose_kernel(const PX* __restrict__ raw, int H, int W, int tiles_x,
                                                             RealGate g, float* __restrict__ out) {
  __shared__ float tile[RT][RT_LD];   // [x][y]
  const int t = threadIdx.x;
  const int x0 = (int)(blockIdx.x % tiles_x) * RT, y0 = (int)(blockIdx.x / tiles_x) * RT;
  const size_t fo = (size_t)blockIdx.y * H * W;
  const PX* src = raw + fo;
  float* dst = out + fo;
  {
    // 16 loads a thread, all issued before the first use; a pixel past the frame's edge reads the
    // edge pixel instead (in bounds), and its tile entry is never stored
    const int yl = t & 63, y = min(y0 + yl, H - 1);
    PX v[RT / 4];
#pragma unroll
    for (int k = 0; k < RT / 4; ++k) {
      const int x = min(x0 + (t >> 6) + 4 * k, W - 1);
      v[k] = src[(size_t)x * H + y];
    }
#pragma unroll
    for (int k = 0; k < RT / 4; ++k) tile[(t >> 6) + 4 * k][yl] = real_px<PX>(v[k], g);
  }
  __syncthreads();
  // a half wave: 8 quads of x (128 B of a row) times 4 rows; the two halves are the two row halves
  const int xl = ((t >> 5) & 1) * 32 + (t & 7) * 4, x = x0 + xl;
  if (x >= W) return;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int yl = k * 16 + (t >> 6) * 4 + ((t >> 3) & 3), y = y0 + yl;
    if (y >= H) continue;
    float* p = dst + (size_t)y * W + x;
    if (x + 4 <= W && (reinterpret_cast<uintptr_t>(p) & 15) == 0) {
      *reinterpret_cast<float4*>(p) = make_float4(tile[xl][yl], tile[xl + 1][yl], tile[xl + 2][yl], tile[xl + 3][yl]);
    } else {   // the row's tail, or a row that starts off a 16-byte boundary (W % 4 != 0)
      for (int j = 0; j < 4 && x + j < W; ++j) p[j] = tile[xl + j][yl];
    }
  }
}

template <typename PX, bool VEC>
__global__ __launch_bounds__(256) void real_plain_kernel(const PX* __restrict__ raw, int64_t total, RealGate g,
                                                         float* __restrict__ out) {
  const int64_t i0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * (VEC ? 4 : 1);
  if (i0 >= total) return;
  if constexpr (VEC) {
    if (i0 + 4 <= total) {
      using V4 = typename std::conditional<std::is_same<PX, uint16_t>::value, ushort4, float4>::type;
      const V4 v = *reinterpret_cast<const V4*>(raw + i0);
      *reinterpret_cast<float4*>(out + i0) =
          make_float4(real_px<PX>(v.x, g), real_px<PX>(v.y, g), real_px<PX>(v.z, g), real_px<PX>(v.w, g));
    } else {
      for (int64_t i = i0; i < total; ++i) out[i] = real_px<PX>(raw[i], g);
    }
  } else {
    out[i0] = real_px<PX>(raw[i0], g);
  }
}

template <typename PX>
hipError_t launch_real_t(const PX* raw, int64_t n, int H, int W, bool transposed, const RealGate& g, float* out,
                         hipStream_t st) {
  if (transposed && H > 1 && W > 1) {
    const int tiles_x = (W + RT - 1) / RT, tiles_y = (H + RT - 1) / RT;
    hipLaunchKernelGGL((real_transpose_kernel<PX>), dim3((unsigned)tiles_x * (unsigned)tiles_y, (unsigned)n), dim3(256),
                       0, st, raw, H, W, tiles_x, g, out);
    return hipGetLastError();
  }
  // [n][W][1] and [n][1][H] are their own transposes
  const int64_t total = n * H * W;
  const bool vec = (reinterpret_cast<uintptr_t>(raw) & (4 * sizeof(PX) - 1)) == 0 &&
                   (reinterpret_cast<uintptr_t>(out) & 15) == 0;
  const int64_t per = vec ? 1024 : 256;
  const int64_t nb = (total + per - 1) / per;
  if (nb > 0x7fffffff) return hipErrorInvalidValue;
  if (vec)
    hipLaunchKernelGGL((real_plain_kernel<PX, true>), dim3((unsigned)nb), dim3(256), 0, st, raw, total, g, out);
  else
    hipLaunchKernelGGL((real_plain_kernel<PX, false>), dim3((unsigned)nb), dim3(256), 0, st, raw, total, g, out);
  return hipGetLastError();
}

}  // namespace

// Arguments as validated by mp_real_frames_dev (uint16: lo, hi and fill are integers in [0, 65535]).
hipError_t launch_real_frames(const void* raw, bool u16, int64_t n, int H, int W, bool transposed, bool gate,
                              double lo, double hi, double fill, double max_depth, float* out, hipStream_t st) {
  RealGate g{};
  g.on = gate ? 1 : 0;
  g.md = (float)max_depth;
  if (gate) {
    if (u16) {
      g.ulo = (uint32_t)lo;
      g.uhi = (uint32_t)hi;
      g.ufill = (uint32_t)fill;
    } else {
      g.flo = (float)lo;
      g.fhi = (float)hi;
      g.ffill = (float)fill;
    }
  }
  if (u16) return launch_real_t(static_cast<const uint16_t*>(raw), n, H, W, transposed, g, out, st);
  return launch_real_t(static_cast<const float*>(raw), n, H, W, transposed, g, out, st);
}

}  // namespace mp
