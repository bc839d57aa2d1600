// The drawing rule of a joint overlay (the picture test_model, eval_model_on_real_data and the
// validation block of train_model end with: plt.imshow(frame); plt.scatter(uvd), and
// save_result_image's labels / results / skeleton lines), stated once for the kernel (k_overlay.hip)
// and for a host evaluator (the CPU test).  Plain C++, contraction off: every float operation below is
// one IEEE float32 operation, every coverage test is integer arithmetic.
//
// out[n][h][w][3] uint8 RGB.  A pixel takes the colour of the LAST primitive that covers it, in the
// order: for s = 0 .. S-1: the bones of set s in list order, then its joints in index order.  No
// primitive: the depth colour.  No blending, no atomics, nothing depends on block order.
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MP_OVL_HD __host__ __device__
#else
#define MP_OVL_HD
#endif

#include <cmath>
#include <cstdint>

namespace mpovl {

constexpr int MAX_HW = 4096;       // h, w
constexpr int MAX_SETS = 4;        // S
constexpr int MAX_JOINTS = 128;    // J
constexpr int MAX_BONES = 256;     // nb
constexpr int MAX_RADIUS = 15;     // r in 0..15 (0: one pixel)
constexpr int MAX_THICK = 15;      // th in 1..15
constexpr int MAX_PRIMS = MAX_SETS * (MAX_JOINTS + MAX_BONES);
constexpr float C_MIN = -4096.f;   // eligible centres: C_MIN <= floor(u + 0.5) <= C_MAX
constexpr float C_MAX = 8191.f;

// depth colour: the index into lut[256][3] of frame value d (a uint16 pixel converts exactly)
MP_OVL_HD inline int color_index(float d, float lo, float hi) {
  const float x = (d - lo) / (hi - lo);
  if (!(x >= 0.f)) return 0;       // also NaN
  if (x >= 1.f) return 255;
  const float p = x * 255.f;
  return (int)(p + 0.5f);
}

// the pixel a joint coordinate is centred on; false: not eligible (NaN and +-inf fail the compares)
MP_OVL_HD inline bool center(float u, int* c) {
  const float f = floorf(u + 0.5f);
  if (!(f >= C_MIN && f <= C_MAX)) return false;
  *c = (int)f;
  return true;
}

MP_OVL_HD inline bool disc_covers(int x, int y, int cu, int cv, int r) {
  const int dx = x - cu, dy = y - cv;       // |dx|, |dy| < 2^14: the squares fit an int
  return dx * dx + dy * dy <= r * r;
}

// the segment between eligible centres P and Q, th pixels thick; the caps are left to the markers.
// Pixels are in [0, 4096) and centres in [-4096, 8191]: |e| < 2^13.1, |d| < 2^13.6, so |c| < 2^29
// and 4 c^2 < 2^60 fits int64; th^2 L2 < 2^8 * 2^28.2.
MP_OVL_HD inline bool bone_covers(int x, int y, int px, int py, int qx, int qy, int th) {
  const int64_t dx = (int64_t)qx - px, dy = (int64_t)qy - py;
  const int64_t L2 = dx * dx + dy * dy;
  const int64_t ex = (int64_t)x - px, ey = (int64_t)y - py;
  const int64_t s = ex * dx + ey * dy;
  const int64_t c = ex * dy - ey * dx;
  return L2 > 0 && 0 <= s && s <= L2 && 4 * c * c <= (int64_t)th * th * L2;
}

// The same bone prepared once (k_overlay.hip keeps d and L2 with the primitive): s, c and L2 as ints.
// For pixels in [0, 4096) and centres in [-4096, 8191]: |e| <= 8191 and |d| <= 12287, so |s| and |c|
// are at most 2 * 8191 * 12287 < 2^28 and L2 <= 2 * 12287^2 < 2^29: none of them leaves an int, and
// only 4 c^2 and th^2 L2 need 64 bits.  The same values as above, so the same answer.
struct BonePlan {
  int px, py, dx, dy, L2;
  int64_t lim;   // th^2 L2
};
MP_OVL_HD inline BonePlan bone_plan(int px, int py, int dx, int dy, int L2, int th) {
  return BonePlan{px, py, dx, dy, L2, (int64_t)(th * th) * L2};
}
MP_OVL_HD inline BonePlan bone_plan(int px, int py, int qx, int qy, int th) {
  const int dx = qx - px, dy = qy - py;
  return bone_plan(px, py, dx, dy, dx * dx + dy * dy, th);
}
MP_OVL_HD inline bool bone_covers(const BonePlan& b, int x, int y) {
  const int ex = x - b.px, ey = y - b.py;
  const int s = ex * b.dx + ey * b.dy;
  const int c = ex * b.dy - ey * b.dx;
  return b.L2 > 0 && 0 <= s && s <= b.L2 && 4 * ((int64_t)c * c) <= b.lim;
}

// whether a primitive's bounding box (a disc's: its radius; a bone's: the segment's box grown by th,
// which holds every pixel within th / 2 of the segment) meets the pixel rectangle [x0, x1) x [y0, y1)
MP_OVL_HD inline bool box_meets(int px, int py, int qx, int qy, int grow, int x0, int y0, int x1, int y1) {
  const int ax = (px < qx ? px : qx) - grow, bx = (px < qx ? qx : px) + grow;
  const int ay = (py < qy ? py : qy) - grow, by = (py < qy ? qy : py) + grow;
  return ax < x1 && bx >= x0 && ay < y1 && by >= y0;
}

// whether a bone can cover a pixel of the rectangle [x0, x1) x [y0, y1) (inside [0, 4096)^2): its box,
// then its line.  c is linear in the pixel, so over the rectangle |c| is smallest at a corner unless
// the corners' signs differ; a rectangle whose nearest corner is farther than th / 2 from the line
// holds no covered pixel.  Conservative: never false for a rectangle with a covered pixel.
MP_OVL_HD inline bool bone_meets(const BonePlan& b, int th, int x0, int y0, int x1, int y1) {
  if (!box_meets(b.px, b.py, b.px + b.dx, b.py + b.dy, th, x0, y0, x1, y1)) return false;
  const int ex0 = x0 - b.px, ex1 = x1 - 1 - b.px, ey0 = y0 - b.py, ey1 = y1 - 1 - b.py;
  const int c00 = ex0 * b.dy - ey0 * b.dx, c10 = ex1 * b.dy - ey0 * b.dx;
  const int c01 = ex0 * b.dy - ey1 * b.dx, c11 = ex1 * b.dy - ey1 * b.dx;
  const int lo = c00 < c10 ? c00 : c10, hi = c00 < c10 ? c10 : c00;
  const int lo2 = c01 < c11 ? c01 : c11, hi2 = c01 < c11 ? c11 : c01;
  const int mn = lo < lo2 ? lo : lo2, mx = hi > hi2 ? hi : hi2;
  if (mn <= 0 && mx >= 0) return true;
  const int64_t m = mn > 0 ? mn : -(int64_t)mx;
  return 4 * m * m <= b.lim;
}

}  // namespace mpovl
