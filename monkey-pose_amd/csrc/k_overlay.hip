// Joint overlays on the device (mp_overlay_dev): the depth frame through a colour map with joint
// markers and skeleton lines drawn on it, out[n][h][w][3] uint8 RGB -- the picture the reference's
// inference entries end with (plt.imshow(frame); plt.scatter(uvd); save_result_image).  The rule
// (colour index, eligible centres, disc and bone coverage, the order) is overlay_geom.hpp, the one
// text the CPU test evaluates on the host too.
//
//   overlay_kernel   a gather over pixel tiles: a block of 256 threads owns OT_W x OT_H = 128 x 8
//                    pixels of one frame, four consecutive pixels a thread.  (OT_G > 1 gives a thread
//                    that many groups of four, eight rows apart, and the block a 128 x 8 OT_G tile:
//                    at OT_G = 4 the bare colour map ran 7 - 26 % faster and a scene with joints
//                    14 % slower, profiles/overlay/README.md; the scene is what the kernel is for.)
//     loads    one 8-byte (uint16) or 16-byte (float32) load a thread where the address is aligned
//              to it and the four pixels are inside the row, else up to four single loads; issued
//              before anything else.  A half wave reads 256 / 512 contiguous bytes of a row.
//     list     the frame's eligible centres go to LDS (S * J <= 512, two a thread), then the
//              S * (nb + J) primitives are tested, 256 a round in drawing order, for a bounding box
//              that meets the tile; a wave ballot and the waves' counts give every survivor its
//              place, so the LDS list keeps the drawing order (worst case 4 * (128 + 256) entries
//              of 16 bytes).  A bone is kept only if its line passes within th / 2 of the tile
//              (bone_meets: the tile's corners against the line), not merely its box.  A thread
//              walks the list from its end, testing its four pixels against each entry with s, c
//              and L2 as ints (BonePlan), until all four are covered: the last primitive wins.  An
//              empty list costs the pixel nothing.
//     stores   out rows are 3 * w bytes at any byte offset.  A thread packs its four pixels into
//              three dwords; a row of the tile is laid into LDS shifted by (row address & 15), the
//              sub-dword part of that shift by a funnel shift with the previous lane's last dword
//              (three conflict-free ds_write_b32 a lane: the lane stride is 3 words).  LDS byte k of
//              a row then belongs at global (row address & ~15) + k, and the row leaves as aligned
//              16-byte chunks, one a lane; the first and last chunk of a row, where they are
//              partial, leave as single bytes.  Nothing outside out[3 * n * h * w] is touched.
//
//   transform_joints_kernel   the uvd half of getRelativeCoordinates (monkeydetector.py:341-354) for
//                    a batch: one thread a joint, float64, not fused.
//
// Built with -ffp-contract=off and the correctly rounded float32 division (csrc/Makefile): the colour
// index has numpy's bits.
#include <type_traits>

#include "mp_kernels.hpp"
#include "mp_runtime.hpp"

#pragma clang fp contract(off)

#include "overlay_geom.hpp"

namespace mp {

namespace {

constexpr int OT_W = 128, OT_G = 1, OT_H = 8 * OT_G;     // the tile; 256 threads x OT_G groups of 4 pixels
constexpr int OT_ROW = ((15 + 3 * OT_W + 15) / 16) * 16;  // bytes of a shifted tile row in LDS (416)
constexpr int OT_CHUNKS = OT_ROW / 16;                   // 26 <= 32 lanes of a row
constexpr uint32_t NO_CENTER = 0x80008000u;              // (-32768, -32768): outside the eligible range

struct __attribute__((aligned(16))) OverlayPrim {
  uint32_t p, d;   // centre P and d = Q - P, x | y << 16 as int16 (a disc: d = 0)
  uint32_t c;      // r | g << 8 | b << 16 | (radius or thickness) << 24 | bone << 31
  int32_t L2;      // d . d
};

// by value in the kernel arguments: the skeleton and the styles, validated on the host
struct OverlayScene {
  uint8_t bones[mpovl::MAX_BONES][2];
  uint32_t marker[mpovl::MAX_SETS];   // rgb | radius << 24
  uint32_t bone[mpovl::MAX_SETS];     // rgb | thickness << 24 | 1 << 31
};

__device__ __forceinline__ uint32_t pack_xy(int x, int y) { return ((uint32_t)x & 0xffffu) | ((uint32_t)y << 16); }
__device__ __forceinline__ int unpack_x(uint32_t v) { return (int)(int16_t)(v & 0xffffu); }
__device__ __forceinline__ int unpack_y(uint32_t v) { return (int)(int16_t)(v >> 16); }

// frames [n][h][w]; blockIdx.x = tile of the frame (x tiles fastest), blockIdx.y = frame
template <typename PX>
__global__ __launch_bounds__(256) void overlay_kernel(const PX* __restrict__ frames, int H, int W, int tiles_x,
                                                      float lo, float hi, const uint8_t* __restrict__ lut,
                                                      const float* __restrict__ joints, int S, int J, int nb,
                                                      OverlayScene sc, uint8_t* __restrict__ out) {
  __shared__ uint32_t s_lut[256];
  __shared__ uint32_t s_cen[mpovl::MAX_SETS * mpovl::MAX_JOINTS];
  __shared__ OverlayPrim s_list[mpovl::MAX_PRIMS];
  __shared__ int s_wcnt[2][4];
  __shared__ __attribute__((aligned(16))) uint32_t s_rgb[OT_H][OT_ROW / 4];

  const int t = threadIdx.x;
  const int x0 = (int)(blockIdx.x % tiles_x) * OT_W, y0 = (int)(blockIdx.x / tiles_x) * OT_H;
  const size_t f = blockIdx.y, fo = f * (size_t)H * W;
  const int row = t >> 5, xl = (t & 31) * 4;   // group g of this thread: tile row row + 8 g
  const int x = x0 + xl;

  // the OT_G x 4 pixels of this thread, as float (a uint16 converts exactly), every load issued before
  // the first use; outside the frame: unused
  float d[OT_G][4];
#pragma unroll
  for (int g = 0; g < OT_G; ++g) {
    const int y = y0 + row + 8 * g;
    d[g][0] = d[g][1] = d[g][2] = d[g][3] = 0.f;
    if (y < H && x < W) {
      const PX* p = frames + fo + (size_t)y * W + x;
      if (x + 4 <= W && (reinterpret_cast<uintptr_t>(p) & (4 * sizeof(PX) - 1)) == 0) {
        using V4 = typename std::conditional<std::is_same<PX, uint16_t>::value, ushort4, float4>::type;
        const V4 v = *reinterpret_cast<const V4*>(p);
        d[g][0] = (float)v.x, d[g][1] = (float)v.y, d[g][2] = (float)v.z, d[g][3] = (float)v.w;
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (x + j < W) d[g][j] = (float)p[j];
      }
    }
  }

  // the colour table as one word an entry, and the frame's centres
  s_lut[t] = (uint32_t)lut[3 * t] | ((uint32_t)lut[3 * t + 1] << 8) | ((uint32_t)lut[3 * t + 2] << 16);
  const int nj = S * J;
  for (int i = t; i < nj; i += 256) {
    const float* uv = joints + (f * (size_t)nj + i) * 3;
    int cu = 0, cv = 0;
    const bool oku = mpovl::center(uv[0], &cu), okv = mpovl::center(uv[1], &cv);
    s_cen[i] = oku && okv ? pack_xy(cu, cv) : NO_CENTER;
  }
  __syncthreads();

  // the primitives whose box meets the tile, in drawing order
  const int per = nb + J, total = S * per;
  const int tx1 = min(x0 + OT_W, W), ty1 = min(y0 + OT_H, H);
  int count = 0;
  for (int base = 0, it = 0; base < total; base += 256, ++it) {
    const int idx = base + t;
    OverlayPrim pr{};
    bool keep = false;
    if (idx < total) {
      const int s = idx / per, k = idx - s * per;
      if (k < nb) {
        const uint32_t q = s_cen[s * J + sc.bones[k][1]];
        pr.p = s_cen[s * J + sc.bones[k][0]];
        pr.c = sc.bone[s];
        if (pr.p != NO_CENTER && q != NO_CENTER && pr.p != q) {   // P == Q: L2 = 0 covers nothing
          const int th = (int)((pr.c >> 24) & 15u);
          const mpovl::BonePlan b = mpovl::bone_plan(unpack_x(pr.p), unpack_y(pr.p), unpack_x(q), unpack_y(q), th);
          pr.d = pack_xy(b.dx, b.dy);
          pr.L2 = b.L2;
          keep = mpovl::bone_meets(b, th, x0, y0, tx1, ty1);
        }
      } else {
        pr.p = s_cen[s * J + (k - nb)];
        pr.c = sc.marker[s];
        const int cu = unpack_x(pr.p), cv = unpack_y(pr.p);
        keep = pr.p != NO_CENTER && mpovl::box_meets(cu, cv, cu, cv, (int)((pr.c >> 24) & 15u), x0, y0, tx1, ty1);
      }
    }
    const unsigned long long b = __ballot(keep);
    if ((t & 63) == 0) s_wcnt[it & 1][t >> 6] = __popcll(b);
    __syncthreads();   // the counts; two buffers, so the next round's writes need no second barrier
    int before = 0, all = 0;
#pragma unroll
    for (int wv = 0; wv < 4; ++wv) {
      const int c = s_wcnt[it & 1][wv];
      before += wv < (t >> 6) ? c : 0;
      all += c;
    }
    if (keep) s_list[count + before + __popcll(b & ((1ull << (t & 63)) - 1ull))] = pr;
    count += all;
  }
  if (count) __syncthreads();   // uniform: every thread has the same count

  const int tw = min(OT_W, W - x0);   // pixels of a tile row inside the frame
#pragma unroll
  for (int g = 0; g < OT_G; ++g) {
    const int trow = row + 8 * g, y = y0 + trow;
    // colours: the depth colour, then the last primitive of the list that covers the pixel
    uint32_t col[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) col[j] = s_lut[mpovl::color_index(d[g][j], lo, hi)];
    unsigned open = 15u;   // the pixels of this group no primitive has covered yet
    for (int k = count - 1; k >= 0 && open; --k) {
      const OverlayPrim pr = s_list[k];   // one address a block: a broadcast read
      const int px = unpack_x(pr.p), py = unpack_y(pr.p), gr = (int)((pr.c >> 24) & 15u);
      const mpovl::BonePlan b = mpovl::bone_plan(px, py, unpack_x(pr.d), unpack_y(pr.d), pr.L2, gr);
      const bool bone = (pr.c >> 31) != 0;
      // the primitive's box against these four pixels first: most entries of a tile are nowhere
      // near them, and a wave (two tile rows) then skips the entry as a whole
      if (!mpovl::box_meets(px, py, px + b.dx, py + b.dy, gr, x, y, x + 4, y + 1)) continue;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const bool hit = bone ? mpovl::bone_covers(b, x + j, y) : mpovl::disc_covers(x + j, y, px, py, gr);
        if (hit && ((open >> j) & 1u)) {
          col[j] = pr.c & 0xffffffu;
          open &= ~(1u << j);
        }
      }
    }

    // 12 bytes a thread -> the tile row in LDS, shifted by the row's global address mod 16
    const size_t rowoff = 3 * (fo + (size_t)y * W + x0);
    const unsigned mis = (unsigned)((reinterpret_cast<uintptr_t>(out) + rowoff) & 15);
    {
      const uint32_t A = col[0] | (col[1] << 24);
      const uint32_t B = (col[1] >> 8) | (col[2] << 16);
      const uint32_t C = (col[2] >> 16) | (col[3] << 8);
      const uint32_t prevC = __shfl_up(C, 1, 64);   // lane 0 of a row: bytes in front of the row, never stored
      const unsigned sh = 32u - 8u * (mis & 3u);    // 32, 24, 16, 8
      auto funnel = [sh](uint32_t cur, uint32_t prev) {
        return (uint32_t)((((unsigned long long)cur << 32) | prev) >> sh);
      };
      uint32_t* dst = &s_rgb[trow][(mis >> 2) + 3 * (t & 31)];
      dst[0] = funnel(A, prevC);
      dst[1] = funnel(B, A);
      dst[2] = funnel(C, B);
      if ((t & 31) == 31) dst[3] = funnel(0u, C);
    }
  }
  __syncthreads();

  // LDS bytes [mis, mis + 3 * tw) of a row -> out, 16-byte chunk c at global (row address - mis) + 16 c
  const int chunk = t & 31;
#pragma unroll
  for (int g = 0; g < OT_G; ++g) {
    const int trow = row + 8 * g, y = y0 + trow;
    const size_t rowoff = 3 * (fo + (size_t)y * W + x0);               // only used where y < H
    const unsigned mis = (unsigned)((reinterpret_cast<uintptr_t>(out) + rowoff) & 15);
    if (y < H && chunk < OT_CHUNKS) {
      const int lo_b = (int)mis, hi_b = (int)mis + 3 * tw;
      const int c0 = chunk * 16, c1 = c0 + 16;
      uint8_t* gp = out + rowoff;             // the row's first byte = LDS byte lo_b
      if (c0 >= lo_b && c1 <= hi_b) {
        *reinterpret_cast<uint4*>(gp + (c0 - lo_b)) = *reinterpret_cast<const uint4*>(&s_rgb[trow][c0 / 4]);
      } else if (c1 > lo_b && c0 < hi_b) {
        const uint8_t* src = reinterpret_cast<const uint8_t*>(&s_rgb[trow][0]);
        for (int k = max(lo_b, c0); k < min(hi_b, c1); ++k) gp[k - lo_b] = src[k];
      }
    }
  }
}

__global__ __launch_bounds__(256) void transform_joints_kernel(const float* __restrict__ uvd,
                                                               const double* __restrict__ Ms, int64_t total,
                                                               int joints, float* __restrict__ out) {
#pragma clang fp contract(off)
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const double* M = Ms + 9 * (i / joints);
  const double u = (double)uvd[3 * i], v = (double)uvd[3 * i + 1];
  const double t0 = (u * M[0] + v * M[1]) + M[2];
  const double t1 = (u * M[3] + v * M[4]) + M[5];
  const double t2 = (u * M[6] + v * M[7]) + M[8];
  out[3 * i] = (float)(t0 / t2);
  out[3 * i + 1] = (float)(t1 / t2);
  out[3 * i + 2] = uvd[3 * i + 2];
}

template <typename PX>
hipError_t launch_overlay_t(const PX* frames, int n, int H, int W, float lo, float hi, const uint8_t* lut,
                            const float* joints, int S, int J, int nb, const OverlayScene& sc, uint8_t* out,
                            hipStream_t st) {
  const int tiles_x = (W + OT_W - 1) / OT_W, tiles_y = (H + OT_H - 1) / OT_H;
  hipLaunchKernelGGL((overlay_kernel<PX>), dim3((unsigned)tiles_x * (unsigned)tiles_y, (unsigned)n), dim3(256), 0, st,
                     frames, H, W, tiles_x, lo, hi, lut, joints, S, J, nb, sc, out);
  return hipGetLastError();
}

}  // namespace

}  // namespace mp

extern "C" {

int mp_overlay_dev(const void* frames, int depth_dtype, int64_t n, int64_t h, int64_t w, float lo, float hi,
                   const uint8_t* lut, const float* joints_uvd, int64_t S, int64_t J, const int32_t* bones, int64_t nb,
                   const mp_overlay_style* style, uint8_t* out, void* stream) {
  return guard([&] {
    if (!frames || !lut || !style || !out) fail(MP_ERR_ARG, "mp_overlay_dev: null pointer");
    if (depth_dtype != MP_DEPTH_F32 && depth_dtype != MP_DEPTH_U16)
      fail(MP_ERR_ARG, "mp_overlay_dev: unknown depth dtype");
    const bool u16 = depth_dtype == MP_DEPTH_U16;
    if (n <= 0 || n > 65535 || h <= 0 || w <= 0 || h > mpovl::MAX_HW || w > mpovl::MAX_HW)
      fail(MP_ERR_SHAPE, "mp_overlay_dev: bad shape (n <= 65535, h and w <= 4096)");
    if (S < 1 || S > mpovl::MAX_SETS || J < 0 || J > mpovl::MAX_JOINTS || nb < 0 || nb > mpovl::MAX_BONES)
      fail(MP_ERR_SHAPE, "mp_overlay_dev: 1 <= S <= 4, 0 <= J <= 128, 0 <= nb <= 256");
    if (J > 0 && !joints_uvd) fail(MP_ERR_ARG, "mp_overlay_dev: null joints");
    if (nb > 0 && !bones) fail(MP_ERR_ARG, "mp_overlay_dev: null bones");
    if (reinterpret_cast<uintptr_t>(frames) & (u16 ? 1 : 3))
      fail(MP_ERR_ARG, "mp_overlay_dev: frames must be aligned to their element size");
    if (reinterpret_cast<uintptr_t>(joints_uvd) & 3) fail(MP_ERR_ARG, "mp_overlay_dev: joints must be 4-byte aligned");
    if (!std::isfinite(lo) || !std::isfinite(hi) || hi == lo)
      fail(MP_ERR_ARG, "mp_overlay_dev: lo and hi must be finite and differ");
    if (style->struct_size != sizeof(mp_overlay_style))
      fail(MP_ERR_ARG, "mp_overlay_dev: mp_overlay_style.struct_size is not sizeof(mp_overlay_style)");
    mp::OverlayScene sc{};
    for (int s = 0; s < (int)S; ++s) {
      const mp_overlay_set_style& a = style->sets[s];
      if (a.radius > mpovl::MAX_RADIUS || a.thickness < 1 || a.thickness > mpovl::MAX_THICK)
        fail(MP_ERR_ARG, "mp_overlay_dev: radius is 0..15 and thickness 1..15");
      sc.marker[s] = (uint32_t)a.marker_rgb[0] | ((uint32_t)a.marker_rgb[1] << 8) | ((uint32_t)a.marker_rgb[2] << 16) |
                     ((uint32_t)a.radius << 24);
      sc.bone[s] = (uint32_t)a.bone_rgb[0] | ((uint32_t)a.bone_rgb[1] << 8) | ((uint32_t)a.bone_rgb[2] << 16) |
                   ((uint32_t)a.thickness << 24) | (1u << 31);
    }
    for (int64_t k = 0; k < 2 * nb; ++k) {
      if (bones[k] < 0 || bones[k] >= J) fail(MP_ERR_ARG, "mp_overlay_dev: a bone index is outside 0..J-1");
      sc.bones[k / 2][k % 2] = (uint8_t)bones[k];
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    hip_check(u16 ? mp::launch_overlay_t(static_cast<const uint16_t*>(frames), (int)n, (int)h, (int)w, lo, hi, lut,
                                         joints_uvd, (int)S, (int)J, (int)nb, sc, out, st)
                  : mp::launch_overlay_t(static_cast<const float*>(frames), (int)n, (int)h, (int)w, lo, hi, lut,
                                         joints_uvd, (int)S, (int)J, (int)nb, sc, out, st),
              "overlay");
  });
}

int mp_transform_joints_dev(const float* joints_uvd, const double* Ms, int64_t n, int64_t joints, float* out,
                            void* stream) {
  return guard([&] {
    if (!joints_uvd || !Ms || !out) fail(MP_ERR_ARG, "mp_transform_joints_dev: null pointer");
    if (n <= 0 || joints <= 0 || joints > 65535 || n > ((int64_t)1 << 24))
      fail(MP_ERR_SHAPE, "mp_transform_joints_dev: bad shape");
    if ((reinterpret_cast<uintptr_t>(joints_uvd) & 3) || (reinterpret_cast<uintptr_t>(out) & 3) ||
        (reinterpret_cast<uintptr_t>(Ms) & 7))
      fail(MP_ERR_ARG, "mp_transform_joints_dev: misaligned pointer");
    const int64_t total = n * joints;
    hipLaunchKernelGGL(mp::transform_joints_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), joints_uvd, Ms, total, (int)joints, out);
    hip_check(hipGetLastError(), "transform_joints");
  });
}

}  // extern "C"
