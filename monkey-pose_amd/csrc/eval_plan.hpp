// Order of the per-frame reductions of the device evaluation (k_eval.hip): numpy's nanmean / nanmax
// over the J <= 128 joint distances of one frame, float32.  Plain C++: host code (the CPU test's
// evaluator below) and the kernel include the same functions, so the order the GPU runs is the order
// the CPU test checks against numpy bit for bit.
//
// nanmean(d, axis=1) of a float32 row: NaN replaced by 0, numpy's pairwise sum, divided by the count
// of non-NaN elements.  For J <= 128 the pairwise sum is one leaf (loops_utils.h.src):
//   J < 8         the elements one by one;
//   8 <= J <= 128 eight accumulators r[k] = a[k]; r[k] += a[i + k] for every further full block of 8;
//                 ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)); then the J % 8 tail one by one.
// numpy's recursion starts above 128 elements; MAX_JOINTS is that limit.
//
// On the device one wave owns a frame: lane k < 8 keeps accumulator k (lane_acc), three xor-shuffles
// add them in the order above (float addition commutes bit for bit on non-NaN values), lane 0 adds
// the tail.
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MP_EVAL_HD __host__ __device__
#else
#define MP_EVAL_HD
#endif

#include <cmath>
#include <cstdint>

namespace evalplan {

constexpr int MAX_JOINTS = 128;      // numpy's PW_BLOCKSIZE: one leaf, no recursion
constexpr int MAX_THRESHOLDS = 1024;

// a[0, J) with NaN already replaced by 0.  Accumulator k of a leaf of J >= 8 elements.
MP_EVAL_HD inline float lane_acc(const float* a, int J, int k) {
  float r = a[k];
  const int end = J - J % 8;
  for (int i = 8; i < end; i += 8) r += a[i + k];
  return r;
}

MP_EVAL_HD inline float combine8(const float r[8]) {
  return ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
}

// after the eight accumulators are combined: the J % 8 tail
MP_EVAL_HD inline float leaf_tail(const float* a, int J, float res) {
  for (int i = J - J % 8; i < J; ++i) res += a[i];
  return res;
}

// J < 8
MP_EVAL_HD inline float short_sum(const float* a, int J) {
  float r = 0.f;
  for (int i = 0; i < J; ++i) r += a[i];
  return r;
}

// numpy's reduce starts from the identity; the mean is one float32 division (numpy divides in
// float64 and rounds to float32: the same bits, 53 >= 2 * 24 + 2)
MP_EVAL_HD inline float finish_mean(float sum, int cnt) {
  if (cnt == 0) return NAN;
  return (0.f + sum) / (float)cnt;
}

#if !defined(__HIP_DEVICE_COMPILE__)
// ---- one frame on the host, step for step as the kernel runs it ----------------------------------
// d[0, J): the joint distances (NaN allowed); scratch: J floats
inline void frame_stats_host(const float* d, int J, float* scratch, float* mean, float* mx, int* cnt) {
  int c = 0;
  float m = -1.f;   // distances are >= 0
  for (int i = 0; i < J; ++i) {
    const bool nan = d[i] != d[i];
    scratch[i] = nan ? 0.f : d[i];
    if (!nan) {
      ++c;
      m = d[i] > m ? d[i] : m;
    }
  }
  float s;
  if (J < 8) {
    s = short_sum(scratch, J);
  } else {
    float r[8];
    for (int k = 0; k < 8; ++k) r[k] = lane_acc(scratch, J, k);
    s = leaf_tail(scratch, J, combine8(r));
  }
  *mean = finish_mean(s, c);
  *mx = c ? m : NAN;
  *cnt = c;
}
#endif

}  // namespace evalplan
