// Epilogue kernels of the general ContextualCircuit loop (mp_abi.hip var_circuit): every aux variant
// outside the fused pose configuration runs  conv -> plain P map -> one of these two kernels  per
// half-step.  The per-channel rule is circuit_var.hpp's; this file adds the map traffic and the two
// 64x64 1x1 gate products.
//
// One wave per 32-pixel row segment, values held in the v_mfma 32x32 accumulator layout (register r
// of lane (h, x) = channel 32n + 8(r>>2) + 4h + (r&3) of pixel x), so the gate products run on the
// MFMA gate fragments (gate() below) with no lane movement and every map access is a 16-byte load
// or store per lane, one pass over each map.  The state maps X, O, I and the conv inputs are C8; P
// is C8 from the direct convs and the FFT path's P layout (C4: fft_dev.hpp pp_index) from
// launch_fft_inv.  The variant is wave-uniform: its branches are scalar.
#include "circuit_var.hpp"
#include "fft_dev.hpp"

namespace mp {

using namespace mpcv;

template <bool PC4>
__device__ __forceinline__ size_t p_index(int b, int q, int y, int x, int e, int H, int W) {
  return PC4 ? pp_index(b, q, y, x, e, H, W) : c8_index(b, q, y, x, e, H, W);
}

// the 64x64 1x1 gate product of one 32-pixel segment.  The bounded nonlinearities (tanh, hard_tanh)
// keep the states inside the f16x3 split's range (|v| < 255, fft_dev.hpp gate_x3), so their gates run
// as three f16 MFMA products, 768 issue cycles a gate; relu, selu and leaky_relu states are
// unbounded and take conv_epi.hpp's exact fp32 MFMA (4096 cycles a gate)
template <int NL>
__device__ __forceinline__ void gate(const CvArgs& a, bool out_gate, const f32x16 (&V)[2], f32x16 (&Y)[2], int lane) {
  if constexpr (NL == NL_TANH || NL == NL_HARD_TANH)
    gate_x3(static_cast<const f16x8*>(out_gate ? a.or_x3 : a.ir_x3), V, Y, lane, out_gate ? a.or_us : a.ir_us);
  else
    gate_mm(out_gate ? a.gpk_or : a.gpk_ir, V, Y, lane);
}

__device__ __forceinline__ f32x4 vec4(const float* vecs, int id, int c) {
  return *reinterpret_cast<const f32x4*>(vecs + id * 64 + c);
}

// input half: I' = rule_in(P1, X, O, I) -> a.I (in place); with output_gru_gates also
// B_in = I' * sigmoid(I' . o_r + o_b) -> a.Bin (otherwise the next conv reads I' itself)
template <bool PC4, int NL>
__global__ __launch_bounds__(256) void circuit_in_kernel(CvArgs a, int nseg) {
  const int lane = threadIdx.x & 63, h = lane >> 5;
  const int seg = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (seg >= nseg) return;
  const CircuitVariant v = a.v;
  const int H = a.H, W = a.W, xs = W / 32;
  const int x = (seg % xs) * 32 + (lane & 31);
  const int y = (seg / xs) % H, b = seg / xs / H;
  const bool reads_o = v.integration != INT_MELY, reads_i = reads_prev_i(v);
  f32x16 V[2], Y[2];
  if (v.blend_in) {   // g1 = sigmoid(O . i_r + i_b)
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const f32x4 ov = *reinterpret_cast<const f32x4*>(a.O + c8_index(b, 4 * n + g, y, x, 4 * h, H, W));
#pragma unroll
        for (int j = 0; j < 4; ++j) V[n][4 * g + j] = ov[j];
      }
    gate<NL>(a, false, V, Y, lane);
  }
#pragma unroll
  for (int n = 0; n < 2; ++n)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int c = 32 * n + 8 * g + 4 * h;
      const size_t idx = c8_index(b, 4 * n + g, y, x, 4 * h, H, W);
      const f32x4 pv = *reinterpret_cast<const f32x4*>(a.P + p_index<PC4>(b, 4 * n + g, y, x, 4 * h, H, W));
      const f32x4 xv = *reinterpret_cast<const f32x4*>(a.X + idx);
      f32x4 ov = {}, iv = {};
      if (v.blend_in) {
#pragma unroll
        for (int j = 0; j < 4; ++j) ov[j] = V[n][4 * g + j];
      } else if (reads_o) {
        ov = *reinterpret_cast<const f32x4*>(a.O + idx);
      }
      if (reads_i) iv = *reinterpret_cast<const f32x4*>(a.I + idx);
      const f32x4 lat = vec4(a.vecs, V_LAT, c), be = vec4(a.vecs, V_BETA, c), nu = vec4(a.vecs, V_NU, c);
      const f32x4 xi = vec4(a.vecs, CV_XI, c), ib = vec4(a.vecs, V_IB, c);
      f32x4 o;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int r = 4 * g + j;
        const InConst k{lat[j], be[j], nu[j], xi[j]};
        const float g1p = v.blend_in ? Y[n][r] + ib[j] : 0.f;
        o[j] = rule_in<NL>(v, pv[j], xv[j], ov[j], iv[j], g1p, k);
        V[n][r] = o[j];
      }
      *reinterpret_cast<f32x4*>(a.I + idx) = o;
    }
  if (v.out_gates) {   // B_in = I' * sigmoid(I' . o_r + o_b)        729-743
    gate<NL>(a, true, V, Y, lane);
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int c = 32 * n + 8 * g + 4 * h;
        const f32x4 ob = vec4(a.vecs, V_OB, c);
        f32x4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = V[n][4 * g + j] * sigmoid(Y[n][4 * g + j] + ob[j]);
        *reinterpret_cast<f32x4*>(a.Bin + c8_index(b, 4 * n + g, y, x, 4 * h, H, W)) = o;
      }
  }
}

// output half: O' = rule_out(P2, I', O) -> a.O (in place); then, unless this is the last step,
// with gru_gates the next conv's input A_in = O' * sigmoid(O' . i_r + i_b) -> a.Ain (without them the
// conv reads O' itself); on the last step the NHWC fp32 result -> a.out
// (three blocks a CU: 3 waves per SIMD inside 168 registers with no scratch; unbounded it took 182
// with the accumulators in AGPRs, 2 waves, and four blocks spill)
template <bool PC4, int NL>
__global__ __launch_bounds__(256, 3) void circuit_out_kernel(CvArgs a, int nseg) {
  const int lane = threadIdx.x & 63, h = lane >> 5;
  const int seg = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (seg >= nseg) return;
  const CircuitVariant v = a.v;
  const int H = a.H, W = a.W, xs = W / 32;
  const int x = (seg % xs) * 32 + (lane & 31);
  const int y = (seg / xs) % H, b = seg / xs / H;
  f32x16 V[2], Y[2];
#pragma unroll
  for (int n = 0; n < 2; ++n)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const f32x4 iv = *reinterpret_cast<const f32x4*>(a.I + c8_index(b, 4 * n + g, y, x, 4 * h, H, W));
#pragma unroll
      for (int j = 0; j < 4; ++j) V[n][4 * g + j] = iv[j];
    }
  if (v.blend_out) gate<NL>(a, true, V, Y, lane);   // g2 = sigmoid(I' . o_r + o_b)
#pragma unroll
  for (int n = 0; n < 2; ++n)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int c = 32 * n + 8 * g + 4 * h;
      const size_t idx = c8_index(b, 4 * n + g, y, x, 4 * h, H, W);
      const f32x4 pv = *reinterpret_cast<const f32x4*>(a.P + p_index<PC4>(b, 4 * n + g, y, x, 4 * h, H, W));
      f32x4 ov = {};
      if (v.blend_out) ov = *reinterpret_cast<const f32x4*>(a.O + idx);
      const f32x4 lat = vec4(a.vecs, V_LAT, c), ga = vec4(a.vecs, V_GAMMA, c), ka = vec4(a.vecs, V_KAPPA, c);
      const f32x4 om = vec4(a.vecs, V_OMEGA, c), ze = vec4(a.vecs, CV_ZETA, c), ob = vec4(a.vecs, V_OB, c);
      f32x4 o;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int r = 4 * g + j;
        const OutConst k{lat[j], ga[j], ka[j], om[j], ze[j]};
        const float g2p = v.blend_out ? Y[n][r] + ob[j] : 0.f;
        o[j] = rule_out<NL>(v, pv[j], V[n][r], ov[j], g2p, a.rho, k);
        V[n][r] = o[j];
      }
      *reinterpret_cast<f32x4*>(a.O + idx) = o;
    }
  if (a.out) {   // last step: O_T as the NHWC fp32 result
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int c = 32 * n + 8 * g + 4 * h;
        f32x4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = V[n][4 * g + j];
        *reinterpret_cast<f32x4*>(a.out + (((size_t)b * H + y) * W + x) * C + c) = o;
      }
  } else if (v.gru_gates) {   // A_in = O' * sigmoid(O' . i_r + i_b)        696-711
    gate<NL>(a, false, V, Y, lane);
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int c = 32 * n + 8 * g + 4 * h;
        const f32x4 ib = vec4(a.vecs, V_IB, c);
        f32x4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = V[n][4 * g + j] * sigmoid(Y[n][4 * g + j] + ib[j]);
        *reinterpret_cast<f32x4*>(a.Ain + c8_index(b, 4 * n + g, y, x, 4 * h, H, W)) = o;
      }
  }
}

template <bool PC4, int NL>
static void launch_half(int half, const CvArgs& a, int nseg, hipStream_t st) {
  if (half == 0)
    hipLaunchKernelGGL((circuit_in_kernel<PC4, NL>), dim3((nseg + 3) / 4), dim3(256), 0, st, a, nseg);
  else
    hipLaunchKernelGGL((circuit_out_kernel<PC4, NL>), dim3((nseg + 3) / 4), dim3(256), 0, st, a, nseg);
}

template <bool PC4>
static hipError_t launch_nl(int half, const CvArgs& a, int nseg, hipStream_t st) {
  switch (a.v.nl) {
    case NL_TANH: launch_half<PC4, NL_TANH>(half, a, nseg, st); break;
    case NL_RELU: launch_half<PC4, NL_RELU>(half, a, nseg, st); break;
    case NL_SELU: launch_half<PC4, NL_SELU>(half, a, nseg, st); break;
    case NL_LEAKY_RELU: launch_half<PC4, NL_LEAKY_RELU>(half, a, nseg, st); break;
    case NL_HARD_TANH: launch_half<PC4, NL_HARD_TANH>(half, a, nseg, st); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

static hipError_t launch_cv(int half, const CvArgs& a, int B, hipStream_t st) {
  if (B <= 0 || a.H <= 0 || a.W <= 0 || a.W % 32 || a.integration_ok() == false) return hipErrorInvalidValue;
  if (a.p_fft && !c4_width_ok(a.W)) return hipErrorInvalidValue;
  const long nseg = (long)B * a.H * (a.W / 32);
  if (nseg > (1L << 30)) return hipErrorInvalidValue;
  // the FFT path hands P over as a C4 map
  return a.p_fft ? launch_nl<true>(half, a, (int)nseg, st) : launch_nl<false>(half, a, (int)nseg, st);
}

hipError_t launch_circuit_in(const CvArgs& a, int B, hipStream_t st) {
  if (!a.P || !a.X || !a.O || !a.I || !a.vecs || !a.gpk_ir || !a.gpk_or || !a.ir_x3 || !a.or_x3 || (a.v.out_gates && !a.Bin))
    return hipErrorInvalidValue;
  return launch_cv(0, a, B, st);
}

hipError_t launch_circuit_out(const CvArgs& a, int B, hipStream_t st) {
  if (!a.P || !a.O || !a.I || !a.vecs || !a.gpk_ir || !a.gpk_or || !a.ir_x3 || !a.or_x3 || (!a.out && a.v.gru_gates && !a.Ain))
    return hipErrorInvalidValue;
  return launch_cv(1, a, B, st);
}

}  // namespace mp
