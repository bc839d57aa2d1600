// The validation pass on the device: what lies between a labelled batch and a metric
// (train_cnn_networks_hgru.py:160-173, 229-237; pose_evaluation.py:30-88, 136-186).
//
//   rel_labels_kernel        the label half of prepare_data (train_cnn_networks_hgru.py:52-56), one
//                            thread per joint: clip((label - f32(uvdtoxyz(com))) / f32(cube_z / 2), -1, 1).
//   com_from_joints_kernel   tfMonkeyDetector.calculateCoMfrom3DJoints (tf_monkeydetector.py:66-71) and
//                            the driver's normalisation (166), one thread per frame.
//   joint_error_kernel       one wave per frame, lanes over joints (two per lane above 64): the joint
//                            distances and numpy's nanmean / nanmax over them in the float32 order of
//                            eval_plan.hpp.
//   eval_accumulate_kernel   adds a batch to the evaluator state: block 0 runs the float64 sums in
//                            frame order (one thread per joint, one for the frame means) and the
//                            integer maximum; every further block owns 256 thresholds.
//   eval_reset_kernel, eval_summary_kernel
//
// The work is tiny (n * J joints): few launches and no host step, not bandwidth, is the aim.  Every
// float operation is numpy's, in its order; contraction is off; fp32 '/' and sqrtf are correctly
// rounded (no fast-math).  No floating-point atomics anywhere: the state's bytes are a function of
// the sequence of calls alone.
#include "eval_plan.hpp"
#include "mp_kernels.hpp"

#pragma clang fp contract(off)

namespace mp {

typedef unsigned long long u64;

// the evaluator state: this header, then joint_sum f64[J], joint_cnt u64[J], within_max u64[T],
// within_mean u64[T], thresholds f32[T]
struct EvalHdr {
  u64 frames, valid;
  double sum_mean;
  uint32_t maxbits, any, J, T, err, pad;
};
static_assert(sizeof(EvalHdr) == 48, "EvalHdr layout");

struct EvalState {
  EvalHdr* h;
  double* joint_sum;
  u64* joint_cnt;
  u64* within_max;
  u64* within_mean;
  float* thr;
};

__host__ __device__ inline EvalState eval_state(void* p, int J, int T) {
  char* c = static_cast<char*>(p);
  EvalState s;
  s.h = reinterpret_cast<EvalHdr*>(c);
  s.joint_sum = reinterpret_cast<double*>(c + sizeof(EvalHdr));
  s.joint_cnt = reinterpret_cast<u64*>(s.joint_sum + J);
  s.within_max = s.joint_cnt + J;
  s.within_mean = s.within_max + T;
  s.thr = reinterpret_cast<float*>(s.within_mean + T);
  return s;
}

size_t eval_state_bytes(int J, int T) {
  return (sizeof(EvalHdr) + (size_t)J * 16 + (size_t)T * 16 + (size_t)T * 4 + 7) & ~(size_t)7;
}

// dist [n][J], frame_mean [n], frame_max [n] when the caller does not ask for them
size_t eval_work_bytes(int64_t n, int J) { return (((size_t)n * J + 2 * (size_t)n) * sizeof(float) + 7) & ~(size_t)7; }

__global__ __launch_bounds__(256) void rel_labels_kernel(mp_camera cam, const float* __restrict__ labels,
                                                         int64_t total, int joints, float half_z,
                                                         const double* __restrict__ coms, float* __restrict__ rel) {
#pragma clang fp contract(off)
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int64_t f = i / joints;
  float c[3];
  com_uvd_to_xyz(cam, coms + 3 * f, &c[0], &c[1], &c[2]);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float v = (labels[3 * i + k] - c[k]) / half_z;
    rel[3 * i + k] = v < -1.f ? -1.f : (v > 1.f ? 1.f : v);   // numpy.clip: a NaN stays a NaN
  }
}

hipError_t launch_rel_labels(const mp_camera& cam, const float* labels, int64_t n, int joints, const double* coms,
                             float* rel, hipStream_t st) {
  const int64_t total = n * joints;
  const float half_z = (float)(cam.cube[2] / 2.0);
  hipLaunchKernelGGL(rel_labels_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, cam, labels, total,
                     joints, half_z, coms, rel);
  return hipGetLastError();
}

__global__ __launch_bounds__(64) void com_from_joints_kernel(const float* __restrict__ labels, int64_t n, int joints,
                                                             float ux, float uy, float fx, float fy, float s0,
                                                             float s1, float s2, float* __restrict__ com) {
#pragma clang fp contract(off)
  const int64_t f = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (f >= n) return;
  const float* a = labels + f * joints * 3;
  float x = a[0], y = a[1], z = a[2];   // labels.mean(axis=1): the joints one by one, float32
  for (int j = 1; j < joints; ++j) {
    x += a[3 * j];
    y += a[3 * j + 1];
    z += a[3 * j + 2];
  }
  const float nj = (float)joints;
  x = x / nj;
  y = y / nj;
  z = z / nj;
  const float u = ux - (x / z) * fx;   // TF's xyztouvd: float32, no z == 0 guard
  const float v = uy + (y / z) * fy;
  const float d = -z;
  com[3 * f] = u / s0;
  com[3 * f + 1] = v / s1;
  com[3 * f + 2] = d / s2;
}

hipError_t launch_com_from_joints(const mp_camera& cam, const float* labels, int64_t n, int joints, float s0,
                                  float s1, float s2, float* com, hipStream_t st) {
  hipLaunchKernelGGL(com_from_joints_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, labels, n, joints,
                     (float)cam.ux, (float)cam.uy, (float)cam.fx, (float)cam.fy, s0, s1, s2, com);
  return hipGetLastError();
}

constexpr int ERR_WAVES = 4;   // frames per block of joint_error_kernel

__global__ __launch_bounds__(64 * ERR_WAVES) void joint_error_kernel(const float* __restrict__ labels,
                                                                    const float* __restrict__ results, int64_t n,
                                                                    int J, float scale, float* __restrict__ dist,
                                                                    float* __restrict__ frame_mean,
                                                                    float* __restrict__ frame_max) {
#pragma clang fp contract(off)
  __shared__ float a[ERR_WAVES][evalplan::MAX_JOINTS];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t f = (int64_t)blockIdx.x * ERR_WAVES + wv;
  const bool valid = f < n;   // wave-uniform
  int c = 0;
  float m = -1.f;             // below every distance
  if (valid) {
    for (int j = lane; j < J; j += 64) {
      const float* L = labels + (f * J + j) * 3;
      const float* R = results + (f * J + j) * 3;
      const float dx = L[0] * scale - R[0] * scale;
      const float dy = L[1] * scale - R[1] * scale;
      const float dz = L[2] * scale - R[2] * scale;
      const float d = sqrtf(((dx * dx) + (dy * dy)) + dz * dz);
      dist[f * J + j] = d;
      const bool nan = d != d;
      a[wv][j] = nan ? 0.f : d;
      if (!nan) {
        ++c;
        m = d > m ? d : m;
      }
    }
  }
  __syncthreads();
  if (!valid) return;
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    c += __shfl_xor(c, o, 64);
    const float mo = __shfl_xor(m, o, 64);
    m = mo > m ? mo : m;
  }
  float s;
  if (J < 8) {
    s = evalplan::short_sum(a[wv], J);
  } else {
    const float r = lane < 8 ? evalplan::lane_acc(a[wv], J, lane) : 0.f;
    const float u = r + __shfl_xor(r, 1, 64);   // r0 + r1 | r2 + r3 | r4 + r5 | r6 + r7
    const float v = u + __shfl_xor(u, 2, 64);   // (r0 + r1) + (r2 + r3) | (r4 + r5) + (r6 + r7)
    const float w = v + __shfl_xor(v, 4, 64);
    s = evalplan::leaf_tail(a[wv], J, w);
  }
  if (lane == 0) {
    frame_mean[f] = evalplan::finish_mean(s, c);
    frame_max[f] = c ? m : NAN;
  }
}

struct ThrChunk {
  float v[256];
};

// zeroes the state (the launch with base == 0) and stores thresholds [base, base + cnt)
__global__ __launch_bounds__(256) void eval_reset_kernel(void* state, int J, int T, int base, int cnt, ThrChunk tc) {
  const EvalState s = eval_state(state, J, T);
  const int t = threadIdx.x;
  if (base == 0) {
    u64* w = reinterpret_cast<u64*>(state);
    const int words = (int)((sizeof(EvalHdr) + (size_t)J * 16 + (size_t)T * 16) / 8);
    for (int i = t; i < words; i += 256) w[i] = 0;
    __syncthreads();
    if (t == 0) {
      s.h->J = (uint32_t)J;
      s.h->T = (uint32_t)T;
    }
  }
  if (t < cnt) s.thr[base + t] = tc.v[t];
}

hipError_t launch_eval_reset(void* state, int J, int T, const float* thresholds_host, hipStream_t st) {
  int base = 0;
  do {
    ThrChunk tc;
    const int cnt = T - base < 256 ? T - base : 256;
    for (int i = 0; i < 256; ++i) tc.v[i] = i < cnt ? thresholds_host[base + i] : 0.f;
    hipLaunchKernelGGL(eval_reset_kernel, dim3(1), dim3(256), 0, st, state, J, T, base, cnt, tc);
    base += 256;
  } while (base < T);
  return hipGetLastError();
}

__global__ __launch_bounds__(256) void eval_accumulate_kernel(void* state, const float* __restrict__ dist,
                                                              const float* __restrict__ frame_mean,
                                                              const float* __restrict__ frame_max, int64_t n, int J,
                                                              int T) {
#pragma clang fp contract(off)
  const EvalState s = eval_state(state, J, T);
  const int t = threadIdx.x;
  if (s.h->J != (uint32_t)J || s.h->T != (uint32_t)T) {   // reset for another shape: nothing is touched
    if (blockIdx.x == 0 && t == 0) s.h->err = 1;
    return;
  }
  if (blockIdx.x > 0) {   // 256 thresholds per block: counts are integers
    const int k = (int)(blockIdx.x - 1) * 256 + t;
    if (k >= T) return;
    const float thr = s.thr[k];
    u64 cmax = 0, cmean = 0;
    for (int64_t f = 0; f < n; ++f) {   // a NaN compares false, as in numpy
      cmax += frame_max[f] <= thr;
      cmean += frame_mean[f] <= thr;
    }
    s.within_max[k] += cmax;
    s.within_mean[k] += cmean;
    return;
  }
  if (t < J) {   // waves 0 and 1: one joint each, the frames in order
    double acc = s.joint_sum[t];
    u64 cnt = s.joint_cnt[t];
    for (int64_t f = 0; f < n; ++f) {
      const float d = dist[f * J + t];
      if (d == d) {
        acc += (double)d;
        ++cnt;
      }
    }
    s.joint_sum[t] = acc;
    s.joint_cnt[t] = cnt;
  } else if (t == 128) {   // wave 2: the frame means in order
    double acc = s.h->sum_mean;
    u64 valid = s.h->valid;
    for (int64_t f = 0; f < n; ++f) {
      const float m = frame_mean[f];
      if (m == m) {
        acc += (double)m;
        ++valid;
      }
    }
    s.h->sum_mean = acc;
    s.h->valid = valid;
    s.h->frames += (u64)n;
  } else if (t >= 192) {   // wave 3: non-negative floats order as their bits
    uint32_t mb = 0, any = 0;
    for (int64_t f = t - 192; f < n; f += 64) {
      const float m = frame_max[f];
      if (m == m) {
        const uint32_t b = __float_as_uint(m);
        mb = b > mb ? b : mb;
        any = 1;
      }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      const uint32_t ob = __shfl_xor(mb, o, 64);
      mb = ob > mb ? ob : mb;
      any |= __shfl_xor(any, o, 64);
    }
    if (t == 192) {
      s.h->maxbits = mb > s.h->maxbits ? mb : s.h->maxbits;
      s.h->any |= any;
    }
  }
}

hipError_t launch_eval_accumulate(void* state, const float* labels, const float* results, int64_t n, int J, int T,
                                  float scale, float* dist, float* frame_mean, float* frame_max, hipStream_t st) {
  hipLaunchKernelGGL(joint_error_kernel, dim3((unsigned)((n + ERR_WAVES - 1) / ERR_WAVES)), dim3(64 * ERR_WAVES), 0,
                     st, labels, results, n, J, scale, dist, frame_mean, frame_max);
  hipLaunchKernelGGL(eval_accumulate_kernel, dim3((unsigned)(1 + (T + 255) / 256)), dim3(256), 0, st, state, dist,
                     frame_mean, frame_max, n, J, T);
  return hipGetLastError();
}

// frames, valid_frames, mean_error, max_error, joint_mean[J], within_max[T], within_mean[T]
__global__ __launch_bounds__(256) void eval_summary_kernel(const void* state, int J, int T, double* __restrict__ out) {
#pragma clang fp contract(off)
  const EvalState s = eval_state(const_cast<void*>(state), J, T);
  const int len = 4 + J + 2 * T;
  const bool bad = s.h->J != (uint32_t)J || s.h->T != (uint32_t)T || s.h->err != 0;
  const double frames = (double)s.h->frames;
  for (int i = threadIdx.x; i < len; i += 256) {
    double v;
    if (bad) {
      v = NAN;
    } else if (i == 0) {
      v = frames;
    } else if (i == 1) {
      v = (double)s.h->valid;
    } else if (i == 2) {
      v = s.h->valid ? s.h->sum_mean / (double)s.h->valid : NAN;
    } else if (i == 3) {
      v = s.h->any ? (double)__uint_as_float(s.h->maxbits) : NAN;
    } else if (i < 4 + J) {
      const int j = i - 4;
      v = s.joint_cnt[j] ? s.joint_sum[j] / (double)s.joint_cnt[j] : NAN;
    } else if (i < 4 + J + T) {
      v = (double)s.within_max[i - 4 - J] / frames * 100.;
    } else {
      v = (double)s.within_mean[i - 4 - J - T] / frames * 100.;
    }
    out[i] = v;
  }
}

hipError_t launch_eval_summary(const void* state, int J, int T, double* out, hipStream_t st) {
  hipLaunchKernelGGL(eval_summary_kernel, dim3(1), dim3(256), 0, st, state, J, T, out);
  return hipGetLastError();
}

}  // namespace mp
