// Frame-level kernels of the end-to-end chain frame -> CoM -> crop -> pose
// (train_cnn_networks_hgru.py:284-321 test_model, 61-74 prepare_data_test):
//
//   resize_bilinear_kernel  tf.image.resize_images(x, [128,128]) of the attention net
//                           (train_cnn_networks_hgru.py:439): TF1 BILINEAR, align_corners=False,
//                           legacy (non half-pixel) source coordinates.  Unfused float32 lerps in
//                           the TF kernel's order, so the result is bit-identical to it.
//   crop3d_kernel           cropArea3D(frame * max_depth, com = attention output * image size)
//                           / max_depth for every frame of the batch on the device -- the
//                           reference's per-image host loop (61-74) in one launch.  Geometry from
//                           crop_geom.hpp (shared with the host crop, so the integers agree).
//                           Also around given float64 CoMs (the detector path), of float32 or of
//                           uint16 frames (depth_u16.hpp: the pixel rules shared with the host).
//
// Both are HBM/latency bound byte movers: one thread per output element, coalesced along the
// innermost output axis.
#include <type_traits>

#include "crop_geom.hpp"
#include "depth_u16.hpp"
#include "mp_kernels.hpp"

#pragma clang fp contract(off)

namespace mp {

__global__ void resize_bilinear_kernel(const float* __restrict__ x, int N, int H, int W, int C, float* out, int Ho,
                                       int Wo, float hs, float ws) {
  const size_t total = (size_t)N * Ho * Wo * C;
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int c = (int)(i % C);
  size_t r = i / C;
  const int ox = (int)(r % Wo);
  r /= Wo;
  const int oy = (int)(r % Ho);
  const int n = (int)(r / Ho);
  // compute_interpolation_weights (LegacyScaler: in = out * scale)
  const float iy = (float)oy * hs, ix = (float)ox * ws;
  const float fy = floorf(iy), fx = floorf(ix);
  const int y0 = max((int)fy, 0), y1 = min((int)ceilf(iy), H - 1);
  const int x0 = max((int)fx, 0), x1 = min((int)ceilf(ix), W - 1);
  const float ly = iy - fy, lx = ix - fx;
  const float* b = x + (size_t)n * H * W * C + c;
  const float tl = b[((size_t)y0 * W + x0) * C], tr = b[((size_t)y0 * W + x1) * C];
  const float bl = b[((size_t)y1 * W + x0) * C], br = b[((size_t)y1 * W + x1) * C];
  // compute_lerp
  const float top = tl + (tr - tl) * lx;
  const float bot = bl + (br - bl) * lx;
  out[i] = top + (bot - top) * ly;
}

hipError_t launch_resize_bilinear(const float* x, int N, int H, int W, int C, float* out, int Ho, int Wo,
                                  hipStream_t st) {
  const size_t total = (size_t)N * Ho * Wo * C;
  // CalculateResizeScale(in, out, align_corners = false) = in / (float)out
  const float hs = (float)H / (float)Ho, ws = (float)W / (float)Wo;
  hipLaunchKernelGGL(resize_bilinear_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, x, N, H, W,
                     C, out, Ho, Wo, hs, ws);
  return hipGetLastError();
}

constexpr int CROP_PIX_PER_BLOCK = 1024;

// The CoM a crop starts from is a template argument, so the attention path's kernels are the code
// they were.  F64 = false: tr_res[im] * [image_orig_size[0], image_orig_size[1], image_max_depth]
// (float32 attention output * float64 scale).  F64 = true (mp_crop3d_dev_coms, the detector path):
// com_norm points at [n][3] float64 CoMs, taken as they are.
#define MP_CROP_COM_IN(com)                                                                     \
  double com[3] = {(double)com_norm[3 * f] * cs0, (double)com_norm[3 * f + 1] * cs1,            \
                   (double)com_norm[3 * f + 2] * cs2};                                          \
  if constexpr (F64) {                                                                          \
    const double* c64 = reinterpret_cast<const double*>(com_norm);                              \
    com[0] = c64[3 * f];                                                                        \
    com[1] = c64[3 * f + 1];                                                                    \
    com[2] = c64[3 * f + 2];                                                                    \
  }

// The frame's pixel type is the other: PX = float keeps the float32 rules below; PX = uint16_t (frames
// in mm, frame_scale 1) applies getCrop's uint16 rule of depth_u16.hpp and widens the stored value.
template <bool F64, typename PX>
__global__ __launch_bounds__(256) void crop3d_kernel(mp_camera cam, const PX* __restrict__ frames, int H, int W,
                                                     float frame_scale, const float* __restrict__ com_norm,
                                                     double cs0, double cs1, double cs2, int dsz,
                                                     float* __restrict__ patches, double* __restrict__ Ms,
                                                     double* __restrict__ coms_out, int32_t* __restrict__ status,
                                                     int refined) {
  __shared__ mpgeom::CropGeom g;
  __shared__ int st;
  const int f = blockIdx.y;
  if (threadIdx.x == 0) {
    // tr_res[im] * [image_orig_size[0], image_orig_size[1], image_max_depth] (float32 * float64), or
    // the docom-refined CoM crop_refine_kernel left in coms_out with the final status in status[f]
    // (the first crop's failure, or the refined crop's geometry status).  In the refined form every
    // block only READS coms_out / status (crop_refine_kernel, the previous launch, wrote them), so
    // no block's read races another block's write; unrefined, the other blocks never read them.
    MP_CROP_COM_IN(com)
    if (refined) {
      com[0] = coms_out[3 * f];
      com[1] = coms_out[3 * f + 1];
      com[2] = coms_out[3 * f + 2];
    }
    st = (refined && status[f] != mpgeom::CROP_OK) ? status[f] : mpgeom::crop_geometry(cam, com, H, W, dsz, &g);
    if (blockIdx.x == 0) {
      if (!refined) {
        status[f] = st;
        coms_out[3 * f] = com[0];
        coms_out[3 * f + 1] = com[1];
        coms_out[3 * f + 2] = com[2];
      }
      double M[9];
      if (st == mpgeom::CROP_OK) {
        mpgeom::crop_matrix(g, M);
      } else {
        for (int k = 0; k < 9; ++k) M[k] = 0.0;
      }
      for (int k = 0; k < 9; ++k) Ms[9 * f + k] = M[k];
    }
  }
  __syncthreads();
  const float md = (float)cam.max_depth;
  const PX* fr = frames + (size_t)f * H * W;
  float* dst = patches + (size_t)f * dsz * dsz;
  const int npix = dsz * dsz;
  for (int k = 0; k < CROP_PIX_PER_BLOCK / 256; ++k) {
    const int p = blockIdx.x * CROP_PIX_PER_BLOCK + k * 256 + threadIdx.x;
    if (p >= npix) break;
    float v = md;   // canvas: ones(dsize, float32) * maxDepth
    if (st == mpgeom::CROP_OK) {
      const int64_t y = p / dsz - g.offy, x = p % dsz - g.offx;
      if (y >= 0 && y < g.szh && x >= 0 && x < g.szw) {
        // getCrop value at the nearest-neighbour source pixel (padded region = 0, z threshold)
        const int64_t sy = mpgeom::nn_row(g, y) - g.pt, sx = mpgeom::nn_col(g, x) - g.pl;
        v = 0.f;
        if (sy >= 0 && sy < g.r1 - g.r0 && sx >= 0 && sx < g.c1 - g.c0) {
          if constexpr (std::is_same<PX, uint16_t>::value) {
            // uint16 frame: compared in float64, zstart stored truncated (depth_u16.hpp), then widened
            v = (float)mpu16::crop_px(fr[(g.r0 + sy) * W + (g.c0 + sx)], g.zstart, g.zend);
          } else {
            const float d = fr[(g.r0 + sy) * W + (g.c0 + sx)] * frame_scale;   // image * max_depth (float32)
            // float32 frame vs float64 bounds: compared in float32 (NumPy 1.x rule, crop_geom.hpp)
            if (mpgeom::f32_lt(d, g.zstart) && d != 0.f)
              v = (float)g.zstart;
            else if (mpgeom::f32_gt(d, g.zend) && d != 0.f)
              v = 0.f;
            else
              v = d;
          }
        }
      }
    }
    dst[p] = v / md;   // patches = crop / max_depth (train_cnn_networks_hgru.py:71)
  }
}

// cropArea3D's docom refinement (monkeydetector.py:287-300) on the device, one block per frame:
// calculateCoM of the first (padded, thresholded) crop -- integer mask sums (exact) and the crop's
// float32 sum in numpy 1.x's pairwise order (pairwise_sum_FLOAT: halves split at multiples of 8,
// blocks of <= 128 summed into 8 partial sums) -- then the allclose / isclose fallbacks and the
// shift back to frame coordinates.  The refined CoM goes to coms_out, which crop3d_kernel then uses.
// The pairwise tree's top D levels are complete (every node there holds >= 145 > 128 elements when
// n / 2^D >= 160, since a split loses at most 15 from the smaller half over D levels), so thread t
// sums the subtree on its D-bit path sequentially in numpy's order and the 2^D results are combined
// pairwise level by level, which is exactly numpy's recursion.
// A uint16 frame's crop is a uint16 array: calculateCoM's dc.sum() is then an exact integer sum, a
// fifth integer beside the mask sums, and there is no order to keep.
constexpr int REF_T = 256;
// getCrop's output (monkeydetector.py:177-213) at flat index i of the padded crop
__device__ float crop_getcrop_value(const mpgeom::CropGeom& g, const float* fr, int W, float frame_scale, int64_t i) {
  const int64_t y = i / g.cols, x = i - y * g.cols;
  const int64_t sy = y - g.pt, sx = x - g.pl;
  float v = 0.f;   // getCrop: the zero padding, else the z-thresholded frame pixel
  if (sy >= 0 && sy < g.r1 - g.r0 && sx >= 0 && sx < g.c1 - g.c0) {
    const float d = fr[(g.r0 + sy) * W + (g.c0 + sx)] * frame_scale;
    if (mpgeom::f32_lt(d, g.zstart) && d != 0.f)
      v = (float)g.zstart;
    else if (mpgeom::f32_gt(d, g.zend) && d != 0.f)
      v = 0.f;
    else
      v = d;
  }
  return v;
}

// calculateCoM's dc of that crop: dc[dc < minDepth] = 0; dc[dc > maxDepth] = 0 (float32 compares)
__device__ float crop_dc_value(const mpgeom::CropGeom& g, const float* fr, int W, float frame_scale,
                               const mp_camera& cam, int64_t i) {
  const float v = crop_getcrop_value(g, fr, W, frame_scale, i);
  return (mpgeom::f32_lt(v, cam.min_depth) || mpgeom::f32_gt(v, cam.max_depth)) ? 0.f : v;
}

// the same two values of a uint16 frame (depth_u16.hpp: float64 compares, uint16 stores)
__device__ uint16_t crop_getcrop_value(const mpgeom::CropGeom& g, const uint16_t* fr, int W, float, int64_t i) {
  const int64_t y = i / g.cols, x = i - y * g.cols;
  const int64_t sy = y - g.pt, sx = x - g.pl;
  if (sy >= 0 && sy < g.r1 - g.r0 && sx >= 0 && sx < g.c1 - g.c0)
    return mpu16::crop_px(fr[(g.r0 + sy) * W + (g.c0 + sx)], g.zstart, g.zend);
  return 0;
}

__device__ uint16_t crop_dc_value(const mpgeom::CropGeom& g, const uint16_t* fr, int W, float frame_scale,
                                  const mp_camera& cam, int64_t i) {
  const uint16_t v = crop_getcrop_value(g, fr, W, frame_scale, i);
  return mpu16::com_out(v, cam.min_depth, cam.max_depth) ? (uint16_t)0 : v;
}

// numpy's pairwise float32 sum of dc[lo, lo + n), iteratively (explicit stack of pending right halves)
__device__ float pairwise_dc(const mpgeom::CropGeom& g, const float* fr, int W, float fs, const mp_camera& cam,
                             int64_t lo, int64_t n) {
  // post-order evaluation: a node's value = left + right, computed with a small value stack
  int64_t st_lo[40], st_n[40];
  int st_state[40];
  float vals[40];
  int sp = 0, vp = 0;
  st_lo[0] = lo; st_n[0] = n; st_state[0] = 0; sp = 1;
  while (sp > 0) {
    const int k = sp - 1;
    const int64_t l = st_lo[k], m = st_n[k];
    if (m <= 128) {
      float r;
      if (m < 8) {
        r = 0.f;
        for (int64_t i = 0; i < m; ++i) r += crop_dc_value(g, fr, W, fs, cam, l + i);
      } else {
        float a[8];
        for (int j = 0; j < 8; ++j) a[j] = crop_dc_value(g, fr, W, fs, cam, l + j);
        int64_t i = 8;
        for (; i < m - (m % 8); i += 8)
          for (int j = 0; j < 8; ++j) a[j] += crop_dc_value(g, fr, W, fs, cam, l + i + j);
        r = ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));
        for (; i < m; ++i) r += crop_dc_value(g, fr, W, fs, cam, l + i);
      }
      vals[vp++] = r;
      --sp;
      continue;
    }
    int64_t n2 = m / 2;
    n2 -= n2 % 8;
    if (st_state[k] == 0) {            // descend left
      st_state[k] = 1;
      st_lo[sp] = l; st_n[sp] = n2; st_state[sp] = 0; ++sp;
    } else if (st_state[k] == 1) {     // then right
      st_state[k] = 2;
      st_lo[sp] = l + n2; st_n[sp] = m - n2; st_state[sp] = 0; ++sp;
    } else {                           // both done: left + right
      const float rgt = vals[--vp], lft = vals[--vp];
      vals[vp++] = lft + rgt;
      --sp;
    }
  }
  return vals[0];
}

template <bool F64, typename PX>
__global__ __launch_bounds__(REF_T) void crop_refine_kernel(mp_camera cam, const PX* __restrict__ frames, int H,
                                                            int W, float frame_scale, const float* __restrict__ com_norm,
                                                            double cs0, double cs1, double cs2, int dsz,
                                                            double* __restrict__ coms_out, int32_t* __restrict__ status) {
#pragma clang fp contract(off)
  __shared__ mpgeom::CropGeom g;
  __shared__ int st;
  __shared__ float part[REF_T];
  // a uint16 crop's value sum is a fifth integer sum (exact), in place of the pairwise float32 sum
  constexpr bool U16 = std::is_same<PX, uint16_t>::value;
  constexpr int NS = U16 ? 5 : 4;
  __shared__ long long isum[NS][REF_T];
  __shared__ int D;
  const int f = blockIdx.x, t = threadIdx.x;
  const PX* fr = frames + (size_t)f * H * W;
  if (t == 0) {
    MP_CROP_COM_IN(com)
    st = mpgeom::crop_geometry(cam, com, H, W, dsz, &g);
    const int64_t n = st == mpgeom::CROP_OK ? g.rows * g.cols : 0;
    int d = 0;
    while (d < 8 && (n >> (d + 1)) >= 160) ++d;
    D = d;
  }
  __syncthreads();
  if (st != mpgeom::CROP_OK) {   // the first crop already fails: crop3d_kernel reports it
    if (t == 0) {
      status[f] = st;
      coms_out[3 * f] = coms_out[3 * f + 1] = coms_out[3 * f + 2] = 0.0;
    }
    return;
  }
  const int64_t n = g.rows * g.cols;
  // integer sums of calculateCoM: positive count, row / column index sums, non-zero count
  long long np = 0, sy = 0, sx = 0, nz = 0;
  [[maybe_unused]] long long sv = 0;
  for (int64_t i = t; i < n; i += REF_T) {
    const PX v = crop_dc_value(g, fr, W, frame_scale, cam, i);
    if (v > PX(0)) {
      ++np;
      sy += i / g.cols;
      sx += i % g.cols;
    }
    nz += v != PX(0);
    if constexpr (U16) sv += v;
  }
  isum[0][t] = np; isum[1][t] = sy; isum[2][t] = sx; isum[3][t] = nz;
  if constexpr (U16) isum[4][t] = sv;
  // the float32 pairwise sum: thread t < 2^D sums the subtree on its path (uint16: nothing to do)
  const int nl = U16 ? 1 : 1 << D;
  if constexpr (!U16) {
    if (t < nl) {
      int64_t lo = 0, m = n;
      for (int b = D - 1; b >= 0; --b) {
        int64_t n2 = m / 2;
        n2 -= n2 % 8;
        if ((t >> b) & 1) { lo += n2; m -= n2; } else { m = n2; }
      }
      part[t] = pairwise_dc(g, fr, W, frame_scale, cam, lo, m);
    }
  }
  __syncthreads();
  for (int w = nl / 2; w >= 1; w /= 2) {   // combine the complete top levels in order
    float v = 0.f;
    if (t < w) v = part[2 * t] + part[2 * t + 1];
    __syncthreads();
    if (t < w) part[t] = v;
    __syncthreads();
  }
  for (int w = REF_T / 2; w >= 1; w /= 2) {   // integer sums (exact: any order)
    if (t < w)
      for (int k = 0; k < NS; ++k) isum[k][t] += isum[k][t + w];
    __syncthreads();
  }
  if (t == 0) {
    double com[3];
    const long long npos = isum[0][0], num = isum[3][0];
    if (num == 0) {
      com[0] = com[1] = com[2] = 0.0;
    } else {
      const double cc0 = (double)isum[1][0] / (double)npos, cc1 = (double)isum[2][0] / (double)npos;
      const double s = U16 ? (double)isum[NS - 1][0] : (double)(0.f + part[0]);
      com[0] = (cc1 * (double)num) / (double)num;
      com[1] = (cc0 * (double)num) / (double)num;
      com[2] = s / (double)num;
    }
    if (fabs(com[0]) <= 1e-8 && fabs(com[1]) <= 1e-8 && fabs(com[2]) <= 1e-8) {   // numpy.allclose(com, 0.)
      const int64_t cy = g.rows / 2, cx = g.cols / 2;
      com[2] = (double)crop_getcrop_value(g, fr, W, frame_scale, cy * g.cols + cx);   // cropped[h//2, w//2]
      if (fabs(com[2]) <= 1e-8) com[2] = 300.;
    }
    com[0] += (double)g.xstart;
    com[1] += (double)g.ystart;
    coms_out[3 * f] = com[0];
    coms_out[3 * f + 1] = com[1];
    coms_out[3 * f + 2] = com[2];
    // the second crop's geometry status, so that crop3d_kernel only reads these words
    mpgeom::CropGeom g2;
    status[f] = mpgeom::crop_geometry(cam, com, H, W, dsz, &g2);
  }
}

template <bool F64, typename PX>
static hipError_t launch_crop3d_t(const mp_camera& cam, const PX* frames, int N, int H, int W, float frame_scale,
                                  const float* com_norm, const double com_scale[3], int dsz, float* patches,
                                  double* Ms, double* coms_out, int32_t* status, hipStream_t st, bool docom) {
  const int nb = (dsz * dsz + CROP_PIX_PER_BLOCK - 1) / CROP_PIX_PER_BLOCK;
  if (docom)
    hipLaunchKernelGGL((crop_refine_kernel<F64, PX>), dim3(N), dim3(REF_T), 0, st, cam, frames, H, W, frame_scale,
                       com_norm, com_scale[0], com_scale[1], com_scale[2], dsz, coms_out, status);
  hipLaunchKernelGGL((crop3d_kernel<F64, PX>), dim3(nb, N), dim3(256), 0, st, cam, frames, H, W, frame_scale, com_norm,
                     com_scale[0], com_scale[1], com_scale[2], dsz, patches, Ms, coms_out, status, docom ? 1 : 0);
  return hipGetLastError();
}

hipError_t launch_crop3d(const mp_camera& cam, const float* frames, int N, int H, int W, float frame_scale,
                         const float* com_norm, const double com_scale[3], int dsz, float* patches, double* Ms,
                         double* coms_out, int32_t* status, hipStream_t st, bool docom) {
  return launch_crop3d_t<false, float>(cam, frames, N, H, W, frame_scale, com_norm, com_scale, dsz, patches, Ms, coms_out,
                                status, st, docom);
}

// the same crop around given float64 CoMs [N][3] (device memory, not aliasing coms_out)
hipError_t launch_crop3d_coms(const mp_camera& cam, const float* frames, int N, int H, int W, float frame_scale,
                              const double* coms, int dsz, float* patches, double* Ms, double* coms_out,
                              int32_t* status, hipStream_t st, bool docom) {
  const double unit[3] = {1.0, 1.0, 1.0};   // unused by the float64 form
  return launch_crop3d_t<true, float>(cam, frames, N, H, W, frame_scale, reinterpret_cast<const float*>(coms), unit,
                                      dsz, patches, Ms, coms_out, status, st, docom);
}

// ... of uint16 frames in mm (MP_DEPTH_U16; there is no normalised form, so no frame scale)
hipError_t launch_crop3d_coms_u16(const mp_camera& cam, const uint16_t* frames, int N, int H, int W,
                                  const double* coms, int dsz, float* patches, double* Ms, double* coms_out,
                                  int32_t* status, hipStream_t st, bool docom) {
  const double unit[3] = {1.0, 1.0, 1.0};
  return launch_crop3d_t<true, uint16_t>(cam, frames, N, H, W, 1.0f, reinterpret_cast<const float*>(coms), unit, dsz,
                                         patches, Ms, coms_out, status, st, docom);
}

// hidden_init 'random' (hgru_module.py:879-887) drawn on the device: element i of O0 is
// f32((2u - 1) * limit), u = (splitmix64(i * golden + key) >> 11) * 2^-53 -- the counter-based
// generator of monkey-pose_amd/weights.py (uniform01 / sym_uniform), so a draw is reproducible on the
// host bit for bit.  Double arithmetic with contraction off, as numpy evaluates it.
__device__ __forceinline__ uint64_t splitmix_mix(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

__global__ __launch_bounds__(256) void hidden_uniform_kernel(float* __restrict__ out, int64_t n, uint64_t key,
                                                             double limit) {
#pragma clang fp contract(off)
  const int64_t i0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
  if (i0 >= n) return;
  float v[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const uint64_t z = splitmix_mix((uint64_t)(i0 + k) * 0x9E3779B97F4A7C15ull + key);
    const double u = (double)(z >> 11) * (1.0 / 9007199254740992.0);
    v[k] = (float)((2.0 * u - 1.0) * limit);
  }
  if (i0 + 4 <= n) {
    *reinterpret_cast<float4*>(out + i0) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
    for (int k = 0; i0 + k < n; ++k) out[i0 + k] = v[k];
  }
}

static uint64_t fnv1a64(const char* s) {
  uint64_t h = 0xCBF29CE484222325ull;
  for (; *s; ++s) {
    h ^= (uint8_t)*s;
    h *= 0x100000001B3ull;
  }
  return h;
}

hipError_t launch_hidden_uniform(float* out, int64_t n, uint64_t seed, double limit, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  const uint64_t key = fnv1a64("h2_init") ^ (seed * 0x2545F4914F6CDD1Dull);
  const int64_t nb = (n + 1023) / 1024;
  hipLaunchKernelGGL(hidden_uniform_kernel, dim3((unsigned)nb), dim3(256), 0, st, out, n, key, limit);
  return hipGetLastError();
}

}  // namespace mp
