// The detector path (SURVEY config 5) on the device: MonkeyDetector.calculateCoM of whole frames
// and getAbsoluteCoordinates of the pose output, the two steps that bracket the device crop
// (k_frame.hip) when the centre of mass comes from the detector itself, not the attention net.
//
//   com_chunk_kernel    calculateCoM (monkeydetector.py:66-83), first stage: a frame's flattened
//                       h * w elements are cut into the 2^Dc chunks of com_plan.hpp, one block each.
//                       The block reads its chunk with coalesced 16-byte loads, thresholds it
//                       (dc[dc < minDepth] = 0; dc[dc > maxDepth] = 0) into an LDS tile, counts the
//                       masks as integers, and sums the tile in numpy's float32 pairwise order:
//                       four lanes per group of one to three leaves, the groups combined on their
//                       paths.  One float and four integers per chunk go to the work buffer.
//   com_finish_kernel   one block per frame: the chunk sums added level by level (the complete top
//                       of numpy's recursion), the integer sums added, then the float64 operations
//                       of mp_crop.hip's center_of_mass.
//   com_u16_chunk_kernel / com_u16_finish_kernel
//                       calculateCoM of uint16 frames: the threshold of depth_u16.hpp as integer
//                       bounds, integer sums only (exact in any order), then the same float64 lines.
//   abs_joints_kernel   getAbsoluteCoordinates (monkeydetector.py:356-360) per joint.
//
// Bit-exact with the host mp_center_of_mass(MP_DEPTH_F32 / MP_DEPTH_U16) /
// MonkeyDetector.getAbsoluteCoordinates: every float operation is the host's, in its order;
// contraction is off.
#include "com_plan.hpp"
#include "depth_u16.hpp"
#include "mp_kernels.hpp"

#pragma clang fp contract(off)

namespace mp {

constexpr int COM_T = 256;
typedef unsigned long long u64;

__device__ __forceinline__ u64 wave_sum(u64 v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}

__global__ __launch_bounds__(COM_T) void com_chunk_kernel(const float* __restrict__ frames, int64_t hw, int W,
                                                          float frame_scale, float lo_t, float hi_t, int Dc,
                                                          float* __restrict__ part, u64* __restrict__ isum) {
#pragma clang fp contract(off)
  __shared__ __attribute__((aligned(16))) float tile[complan::CHUNK_CAP];
  __shared__ float gsum[complan::MAX_GROUPS];
  __shared__ u64 wsum[COM_T / 64][4];
  const int t = threadIdx.x;
  const int64_t f = blockIdx.y, c = blockIdx.x;
  int64_t lo = 0, m = hw;
  complan::descend(Dc, c, &lo, &m);   // this block's chunk [lo, lo + m) of the frame, m <= CHUNK_CAP
  const float* src = frames + f * hw + lo;

  // ---- threshold into the tile, integer mask sums -------------------------------------------
  unsigned np = 0, nz = 0;
  u64 sy = 0, sx = 0;
  auto take = [&](float raw, int i, unsigned y, unsigned x) {
    const float d = raw * frame_scale;
    const float v = (d < lo_t || d > hi_t) ? 0.f : d;
    tile[i] = v;
    const bool pos = v > 0.f;
    np += pos;
    sy += pos ? y : 0u;
    sx += pos ? x : 0u;
    nz += v != 0.f;
  };
  const unsigned uw = (unsigned)W;
  const bool vec = (reinterpret_cast<uintptr_t>(src) & 15) == 0;   // block-uniform
  const int nv = vec ? (int)(m / 4) : 0;
  for (int v4 = t; v4 < nv; v4 += COM_T) {
    const float4 q = *reinterpret_cast<const float4*>(src + 4 * v4);
    const unsigned idx = (unsigned)(lo + 4 * v4);   // h * w <= 2^30
    unsigned y = idx / uw, x = idx - y * uw;
    const float e[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      take(e[k], 4 * v4 + k, y, x);
      if (++x == uw) {
        x = 0;
        ++y;
      }
    }
  }
  for (int i = 4 * nv + t; i < (int)m; i += COM_T) {   // the chunk's last m % 4, or an unaligned chunk
    const unsigned idx = (unsigned)(lo + i);
    const unsigned y = idx / uw;
    take(src[i], i, y, idx - y * uw);
  }
  __syncthreads();

  // ---- the tile's float32 pairwise sum: 4 lanes per group ---------------------------------------
  const int E = complan::depth_for(m, complan::GROUP_CAP);
  const int g = t / complan::GROUP_LANES, q = t % complan::GROUP_LANES;
  // every lane of a wave runs the same three leaf slots (the shuffles below are convergent); a
  // lane without a group, or a group without that leaf, adds nothing
  int64_t glo = 0, gm = 0, llo[3] = {0, 0, 0}, llen[3] = {0, 0, 0};
  int nl = 0;
  if (g < (1 << E)) {
    gm = m;
    complan::descend(E, g, &glo, &gm);
    nl = complan::group_leaves(glo, gm, llo, llen);
  }
  float v[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int64_t s = llen[k];
    const float* a = tile + llo[k];
    float lane = 0.f;
    if (s >= 8) lane = complan::leaf_lane(a, s, q);
    const float u = lane + __shfl_xor(lane, 1, 64);   // (r0 + r1) + (r2 + r3) | (r4 + r5) + (r6 + r7)
    float res = u + __shfl_xor(u, 2, 64);
    if (s >= 8)
      res = complan::leaf_tail(a, s, res);
    else
      res = complan::leaf_short(a, s);                 // s = 0: an unused slot
    v[k] = res;
  }
  if (g < (1 << E) && q == 0) gsum[g] = complan::group_combine(nl, v[0], v[1], v[2]);
  __syncthreads();
  for (int w = (1 << E) / 2; w >= 1; w /= 2) {   // the groups on their paths, level by level
    float r = 0.f;
    if (t < w) r = gsum[2 * t] + gsum[2 * t + 1];
    __syncthreads();
    if (t < w) gsum[t] = r;
    __syncthreads();
  }

  // ---- integer sums (exact in any order) -----------------------------------------------------------
  u64 acc[4] = {(u64)np, sy, sx, (u64)nz};
#pragma unroll
  for (int k = 0; k < 4; ++k) acc[k] = wave_sum(acc[k]);
  if ((t & 63) == 0)
    for (int k = 0; k < 4; ++k) wsum[t / 64][k] = acc[k];
  __syncthreads();
  if (t == 0) {
    const int64_t P = (int64_t)1 << Dc;
    part[f * P + c] = gsum[0];
    for (int k = 0; k < 4; ++k) {
      u64 s = 0;
      for (int wv = 0; wv < COM_T / 64; ++wv) s += wsum[wv][k];
      isum[(f * P + c) * 4 + k] = s;
    }
  }
}

__global__ __launch_bounds__(COM_T) void com_finish_kernel(const float* __restrict__ part,
                                                           const u64* __restrict__ isum, int Dc,
                                                           double* __restrict__ coms) {
#pragma clang fp contract(off)
  __shared__ float ps[COM_T];
  __shared__ u64 wsum[COM_T / 64][4];
  const int t = threadIdx.x;
  const int64_t f = blockIdx.x, P = (int64_t)1 << Dc;
  const float* pf = part + f * P;
  const u64* is = isum + f * P * 4;
  // thread t adds the complete subtree of S consecutive chunk sums (S = P / 256 when P > 256): a
  // value is added to its left sibling as soon as both exist, which is the level-by-level order
  const int nt = P < COM_T ? (int)P : COM_T;
  const int64_t S = P / nt;
  if (t < nt) {
    float stk[32];
    int sp = 0;
    for (int64_t i = 0; i < S; ++i) {
      float v = pf[t * S + i];
      for (int64_t b = i; b & 1; b >>= 1) v = stk[--sp] + v;
      stk[sp++] = v;
    }
    ps[t] = stk[0];
  }
  u64 acc[4] = {0, 0, 0, 0};
  for (int64_t i = t; i < P; i += COM_T)
    for (int k = 0; k < 4; ++k) acc[k] += is[i * 4 + k];
  __syncthreads();
  for (int w = nt / 2; w >= 1; w /= 2) {
    float r = 0.f;
    if (t < w) r = ps[2 * t] + ps[2 * t + 1];
    __syncthreads();
    if (t < w) ps[t] = r;
    __syncthreads();
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) acc[k] = wave_sum(acc[k]);
  if ((t & 63) == 0)
    for (int k = 0; k < 4; ++k) wsum[t / 64][k] = acc[k];
  __syncthreads();
  if (t == 0) {
    u64 tot[4] = {0, 0, 0, 0};
    for (int k = 0; k < 4; ++k)
      for (int wv = 0; wv < COM_T / 64; ++wv) tot[k] += wsum[wv][k];
    const u64 npos = tot[0], sr = tot[1], sc = tot[2], num = tot[3];
    double com[3] = {0.0, 0.0, 0.0};
    if (num != 0) {   // mp_crop.hip center_of_mass
      const double cc0 = (double)sr / (double)npos, cc1 = (double)sc / (double)npos;
      const double s = (double)(0.f + ps[0]);
      com[0] = (cc1 * (double)num) / (double)num;
      com[1] = (cc0 * (double)num) / (double)num;
      com[2] = s / (double)num;
    }
    coms[3 * f] = com[0];
    coms[3 * f + 1] = com[1];
    coms[3 * f + 2] = com[2];
  }
}

size_t com_work_bytes(int64_t n, int64_t hw) {
  const int64_t P = (int64_t)1 << complan::depth_for(hw, complan::CHUNK_CAP);
  const size_t fl = ((size_t)(n * P) * sizeof(float) + 7) & ~(size_t)7;
  return fl + (size_t)(n * P) * 4 * sizeof(u64);
}

hipError_t launch_center_of_mass(const float* frames, int N, int H, int W, float frame_scale, float lo_t,
                                 float hi_t, double* coms, void* work, hipStream_t st) {
  const int64_t hw = (int64_t)H * W;
  const int Dc = complan::depth_for(hw, complan::CHUNK_CAP);
  const int64_t P = (int64_t)1 << Dc;
  float* part = static_cast<float*>(work);
  u64* isum = reinterpret_cast<u64*>(static_cast<char*>(work) + (((size_t)(N * P) * sizeof(float) + 7) & ~(size_t)7));
  hipLaunchKernelGGL(com_chunk_kernel, dim3((unsigned)P, (unsigned)N), dim3(COM_T), 0, st, frames, hw, W,
                     frame_scale, lo_t, hi_t, Dc, part, isum);
  hipLaunchKernelGGL(com_finish_kernel, dim3((unsigned)N), dim3(COM_T), 0, st, part, isum, Dc, coms);
  return hipGetLastError();
}

// ---- calculateCoM of uint16 frames (mp_center_of_mass(MP_DEPTH_U16)) -------------------------------
// Every sum of a uint16 frame is an integer (numpy's dc.sum() of a uint16 array is exact), so any
// partition gives the host's bits: no LDS tile, no pairwise plan.  A frame's h * w pixels are cut
// into chunks of U16_CHUNK, one block each (the float32 kernel's bytes per block).  The chunk is read
// with 16-byte loads (8 pixels) between a scalar head up to the first 16-byte boundary and a scalar
// tail: frame f starts at byte 2 * f * h * w of a buffer that may itself start at any even byte.
// Five integer sums per thread, wave shuffles, LDS, one record per chunk in the work buffer.
constexpr int U16_CHUNK = 8192;
constexpr int U16_SUMS = 5;   // positive count, row sum, column sum, non-zero count, value sum

__global__ __launch_bounds__(COM_T) void com_u16_chunk_kernel(const uint16_t* __restrict__ frames, int64_t hw, int W,
                                                              mpu16::ComBounds th, int P, u64* __restrict__ isum) {
  __shared__ u64 wsum[COM_T / 64][U16_SUMS];
  const int t = threadIdx.x;
  const int64_t f = blockIdx.y, c = blockIdx.x;
  const int64_t lo = c * U16_CHUNK;                                      // < hw: P = ceil(hw / U16_CHUNK)
  const int m = (int)(hw - lo < U16_CHUNK ? hw - lo : (int64_t)U16_CHUNK);
  const uint16_t* src = frames + f * hw + lo;

  unsigned np = 0, nz = 0;
  u64 sy = 0, sx = 0, sv = 0;
  auto take = [&](uint16_t raw, unsigned y, unsigned x) {
    const unsigned v = mpu16::com_out(raw, th) ? 0u : (unsigned)raw;   // dc[dc < min] = 0; dc[dc > max] = 0
    const bool pos = v > 0u;
    np += pos;
    sy += pos ? y : 0u;
    sx += pos ? x : 0u;
    nz += v != 0u;
    sv += v;
  };
  const unsigned uw = (unsigned)W;
  // block-uniform: the pixels before the first 16-byte boundary (src is 2-byte aligned)
  int head = (int)(((16 - (reinterpret_cast<uintptr_t>(src) & 15)) & 15) >> 1);
  if (head > m) head = m;
  const int nv = (m - head) / 8;
  for (int v8 = t; v8 < nv; v8 += COM_T) {
    const uint4 q = *reinterpret_cast<const uint4*>(src + head + 8 * v8);
    const unsigned idx = (unsigned)(lo + head + 8 * v8);   // h * w <= 2^30
    unsigned y = idx / uw, x = idx - y * uw;
    const unsigned e[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      take((uint16_t)(e[k >> 1] >> (16 * (k & 1))), y, x);
      if (++x == uw) {
        x = 0;
        ++y;
      }
    }
  }
  // the head (t < head) and the tail (the last (m - head) % 8): at most 7 pixels each
  const int i = t < head ? t : head + 8 * nv + (t - head);
  if (i < m) {
    const unsigned idx = (unsigned)(lo + i);
    const unsigned y = idx / uw;
    take(src[i], y, idx - y * uw);
  }

  u64 acc[U16_SUMS] = {(u64)np, sy, sx, (u64)nz, sv};
#pragma unroll
  for (int k = 0; k < U16_SUMS; ++k) acc[k] = wave_sum(acc[k]);
  if ((t & 63) == 0)
    for (int k = 0; k < U16_SUMS; ++k) wsum[t / 64][k] = acc[k];
  __syncthreads();
  if (t < U16_SUMS) {
    u64 s = 0;
    for (int wv = 0; wv < COM_T / 64; ++wv) s += wsum[wv][t];
    isum[(f * P + c) * U16_SUMS + t] = s;
  }
}

// one wave per frame: the chunk records added, then center_of_mass<uint16_t>'s float64 lines
__global__ __launch_bounds__(64) void com_u16_finish_kernel(const u64* __restrict__ isum, int P,
                                                            double* __restrict__ coms) {
#pragma clang fp contract(off)
  const int t = threadIdx.x;
  const int64_t f = blockIdx.x;
  const u64* is = isum + f * P * U16_SUMS;
  u64 acc[U16_SUMS] = {0, 0, 0, 0, 0};
  for (int i = t; i < P; i += 64)
    for (int k = 0; k < U16_SUMS; ++k) acc[k] += is[(int64_t)i * U16_SUMS + k];
#pragma unroll
  for (int k = 0; k < U16_SUMS; ++k) acc[k] = wave_sum(acc[k]);
  if (t == 0) {
    const u64 npos = acc[0], sr = acc[1], sc = acc[2], num = acc[3];
    double com[3] = {0.0, 0.0, 0.0};
    if (num != 0) {   // mp_crop.hip center_of_mass
      const double cc0 = (double)sr / (double)npos, cc1 = (double)sc / (double)npos;
      const double s = (double)acc[4];
      com[0] = (cc1 * (double)num) / (double)num;
      com[1] = (cc0 * (double)num) / (double)num;
      com[2] = s / (double)num;
    }
    coms[3 * f] = com[0];
    coms[3 * f + 1] = com[1];
    coms[3 * f + 2] = com[2];
  }
}

static int64_t com_u16_chunks(int64_t hw) { return (hw + U16_CHUNK - 1) / U16_CHUNK; }

size_t com_u16_work_bytes(int64_t n, int64_t hw) {
  return (size_t)(n * com_u16_chunks(hw)) * U16_SUMS * sizeof(u64);
}

hipError_t launch_center_of_mass_u16(const uint16_t* frames, int N, int H, int W, double min_depth, double max_depth,
                                     double* coms, void* work, hipStream_t st) {
  const int64_t hw = (int64_t)H * W;
  const int P = (int)com_u16_chunks(hw);   // <= 2^17
  u64* isum = static_cast<u64*>(work);
  hipLaunchKernelGGL(com_u16_chunk_kernel, dim3((unsigned)P, (unsigned)N), dim3(COM_T), 0, st, frames, hw, W,
                     mpu16::com_bounds(min_depth, max_depth), P, isum);
  hipLaunchKernelGGL(com_u16_finish_kernel, dim3((unsigned)N), dim3(64), 0, st, isum, P, coms);
  return hipGetLastError();
}

// getAbsoluteCoordinates (monkeydetector.py:356-360) of StreamPosePipeline.run's joints, one thread
// per joint: rel = pose * f32(cube_z / 2) (float32), + f32(uvdtoxyz(com)) (float64, rounded once),
// then xyztouvd: float32 x / z and y / z, widened, ux - q * fx and q * fy + uy in float64 rounded
// once, d = -z; z == 0 maps to the principal point.
__global__ __launch_bounds__(256) void abs_joints_kernel(mp_camera cam, const float* __restrict__ pose, int64_t total,
                                                         int joints, float half_z,
                                                         const double* __restrict__ coms, float* __restrict__ xyz,
                                                         float* __restrict__ uvd) {
#pragma clang fp contract(off)
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int64_t f = i / joints;
  float cx, cy, cz;
  com_uvd_to_xyz(cam, coms + 3 * f, &cx, &cy, &cz);
  const float rx = pose[3 * i] * half_z, ry = pose[3 * i + 1] * half_z, rz = pose[3 * i + 2] * half_z;
  const float x = rx + cx, y = ry + cy, z = rz + cz;
  xyz[3 * i] = x;
  xyz[3 * i + 1] = y;
  xyz[3 * i + 2] = z;
  float u = (float)cam.ux, v = (float)cam.uy;
  if (z != 0.f) {
    const double qx = (double)(x / z), qy = (double)(y / z);
    u = (float)(cam.ux - qx * cam.fx);
    v = (float)(qy * cam.fy + cam.uy);
  }
  uvd[3 * i] = u;
  uvd[3 * i + 1] = v;
  uvd[3 * i + 2] = -z;
}

hipError_t launch_abs_joints(const mp_camera& cam, const float* pose, int64_t n, int joints, const double* coms,
                             float* xyz, float* uvd, hipStream_t st) {
  const int64_t total = n * joints;
  const float half_z = (float)(cam.cube[2] / 2.0);
  hipLaunchKernelGGL(abs_joints_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, cam, pose, total,
                     joints, half_z, coms, xyz, uvd);
  return hipGetLastError();
}

}  // namespace mp
