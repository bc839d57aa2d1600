// Split plan of the device calculateCoM's depth sum (k_detect.hip): numpy 1.x's float32 pairwise
// summation (pairwise_sum_FLOAT, numpy/core/src/umath/loops_utils.h.src; mp_crop.hip
// pairwise_sum_f32) of a flattened frame, cut into pieces that blocks, 4-lane groups and lanes sum
// independently and that are then added in the recursion's own order.  Plain C++: host code (the
// CPU test's evaluator below) and the kernels include the same functions, so the plan the GPU runs
// is the plan the CPU test checks against the oracle bit for bit.
//
// The recursion: a node of m > 128 elements splits into a left half of (m / 2 rounded down to a
// multiple of 8) elements and the rest; a node of 8 <= m <= 128 is a leaf summed into 8 strided
// accumulators r[j] += a[i + j], combined ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)), then the
// m % 8 tail elements one by one; fewer than 8 elements are summed one by one.
//
// Sizes: a child is within 7.5 of half its parent, so a node d levels below a node of m elements
// holds more than m / 2^d - 16 and fewer than m / 2^d + 16 elements.  depth_for(m, cap) is the
// smallest d with (m >> d) + 16 <= cap: every node at that depth holds at most cap elements, and
// (for d >= 1) every node above it more than cap - 32 > 128 elements (cap >= 256), i.e. the top d
// levels are complete and the 2^d nodes at depth d, addressed by their d-bit path, are added
// pairwise level by level exactly as the recursion adds them.  A frame too small for a level
// simply gets fewer pieces (d = 0: one).
//
//   frame   -> 2^Dc chunks, Dc = depth_for(h * w, CHUNK_CAP): one block each, staged in LDS
//   chunk   -> 2^E groups,  E  = depth_for(m, GROUP_CAP): four lanes each
//   group   -> 1 - 3 leaves (<= 256 elements: a leaf; or a left leaf and a right node of at most
//              135 elements, itself a leaf or two leaves)
//   leaf    -> lane q of 4 keeps accumulators 2q and 2q + 1
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MP_PLAN_HD __host__ __device__
#else
#define MP_PLAN_HD
#endif

#include <cstdint>

namespace complan {

constexpr int64_t LEAF = 128;         // numpy's PW_BLOCKSIZE
constexpr int64_t CHUNK_CAP = 4096;   // elements of one block's LDS tile
constexpr int64_t GROUP_CAP = 256;
constexpr int GROUP_LANES = 4;
constexpr int MAX_GROUPS = 32;        // 2^depth_for(CHUNK_CAP, GROUP_CAP)

MP_PLAN_HD inline int64_t left_len(int64_t m) {
  const int64_t n2 = m / 2;
  return n2 - n2 % 8;
}

MP_PLAN_HD inline int depth_for(int64_t m, int64_t cap) {
  int d = 0;
  while ((m >> d) + 16 > cap) ++d;
  return d;
}

// the node on the d-bit path `path` (most significant bit first, 0 = left) below [*lo, *lo + *m)
MP_PLAN_HD inline void descend(int d, int64_t path, int64_t* lo, int64_t* m) {
  for (int b = d - 1; b >= 0; --b) {
    const int64_t n2 = left_len(*m);
    if ((path >> b) & 1) {
      *lo += n2;
      *m -= n2;
    } else {
      *m = n2;
    }
  }
}

// the leaves of a group [lo, lo + m), m <= GROUP_CAP; unused slots get length 0.  Its sum is
// v0 (one leaf), v0 + v1 (two), or v0 + (v1 + v2) (three: the right node split once more).
MP_PLAN_HD inline int group_leaves(int64_t lo, int64_t m, int64_t llo[3], int64_t llen[3]) {
  llo[0] = llo[1] = llo[2] = lo;
  llen[0] = m;
  llen[1] = llen[2] = 0;
  if (m <= LEAF) return 1;
  const int64_t L = left_len(m), R = m - L;   // L <= 128: a leaf
  llen[0] = L;
  llo[1] = lo + L;
  llen[1] = R;
  if (R <= LEAF) return 2;
  const int64_t RL = left_len(R);             // R <= 135: two leaves
  llen[1] = RL;
  llo[2] = lo + L + RL;
  llen[2] = R - RL;
  return 3;
}

MP_PLAN_HD inline float group_combine(int nleaves, float v0, float v1, float v2) {
  if (nleaves == 1) return v0;
  if (nleaves == 2) return v0 + v1;
  return v0 + (v1 + v2);
}

// lane q's share of a leaf a[0, s), 8 <= s <= 128: accumulators 2q and 2q + 1, added
MP_PLAN_HD inline float leaf_lane(const float* a, int64_t s, int q) {
  float r0 = a[2 * q], r1 = a[2 * q + 1];
  const int64_t end = s - s % 8;
  for (int64_t i = 8; i < end; i += 8) {
    r0 += a[i + 2 * q];
    r1 += a[i + 2 * q + 1];
  }
  return r0 + r1;
}

// after the four lane values are combined (t0 + t1) + (t2 + t3): the m % 8 tail
MP_PLAN_HD inline float leaf_tail(const float* a, int64_t s, float res) {
  for (int64_t i = s - s % 8; i < s; ++i) res += a[i];
  return res;
}

// a leaf of fewer than 8 elements (only a whole frame of h * w < 8 is one)
MP_PLAN_HD inline float leaf_short(const float* a, int64_t s) {
  float r = 0.f;
  for (int64_t i = 0; i < s; ++i) r += a[i];
  return r;
}

// 2^d values on d-bit paths, added level by level (in place)
MP_PLAN_HD inline float combine_paths(float* v, int d) {
  for (int w = (1 << d) / 2; w >= 1; w /= 2)
    for (int i = 0; i < w; ++i) v[i] = v[2 * i] + v[2 * i + 1];
  return v[0];
}

#if !defined(__HIP_DEVICE_COMPILE__)
// ---- the plan evaluated on the host, step for step as the kernels run it -------------------------
inline float eval_leaf(const float* a, int64_t s) {
  if (s < 8) return leaf_short(a, s);
  float t[GROUP_LANES];
  for (int q = 0; q < GROUP_LANES; ++q) t[q] = leaf_lane(a, s, q);
  return leaf_tail(a, s, (t[0] + t[1]) + (t[2] + t[3]));
}

inline float eval_chunk(const float* a, int64_t m) {   // one block: a = the chunk's tile
  const int E = depth_for(m, GROUP_CAP);
  float g[MAX_GROUPS];
  for (int64_t p = 0; p < ((int64_t)1 << E); ++p) {
    int64_t lo = 0, len = m, llo[3], llen[3];
    descend(E, p, &lo, &len);
    const int nl = group_leaves(lo, len, llo, llen);
    float v[3] = {0.f, 0.f, 0.f};
    for (int k = 0; k < nl; ++k) v[k] = eval_leaf(a + llo[k], llen[k]);
    g[p] = group_combine(nl, v[0], v[1], v[2]);
  }
  return combine_paths(g, E);
}

// the float32 pairwise sum of a[0, n) through the plan; parts: scratch of 2^depth_for(n, CHUNK_CAP)
inline float eval_host(const float* a, int64_t n, float* parts) {
  const int D = depth_for(n, CHUNK_CAP);
  for (int64_t c = 0; c < ((int64_t)1 << D); ++c) {
    int64_t lo = 0, m = n;
    descend(D, c, &lo, &m);
    parts[c] = eval_chunk(a + lo, m);
  }
  return 0.f + combine_paths(parts, D);   // numpy's reduce starts from the identity
}
#endif

}  // namespace complan
