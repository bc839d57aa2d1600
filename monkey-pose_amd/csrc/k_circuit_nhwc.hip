// Epilogue kernels of the channel-general ContextualCircuit loop (mp_abi.hip nhwc_circuit): the loop a
// circuit of any channel count k in [4, 256] runs.  Every map -- the states X, O, I, the conv result P,
// the gated conv inputs A_in / B_in and the gate pre-activations g1p / g2p -- is NHWC fp32 [n,h,w,k],
// so one half-step is purely per element: element e of a map is channel e % k of pixel e / k, and the
// two kernels below are flat passes over the maps with circuit_var.hpp's rule in the middle.
//
// The convs (p_r * A_in, and the two 1x1 gate products with i_b / o_b as their bias) run on the graph
// runtime's implicit-GEMM launchers.  Where a gated conv input needs the gate of the value a kernel
// has just written (B_in = I' sigmoid(I' . o_r + o_b), A_in = O' sigmoid(O' . i_r + i_b)), the 1x1
// product runs between the rule kernel and circuit_gate_kernel (rule -> gate conv -> multiply):
// a k x k product per pixel inside an elementwise kernel would need its own MFMA tiling per k.
//
// VW = 4 (k % 4 == 0): one 16-byte access per map and thread, the four channels of one pixel;
// VW = 1: one float per thread -- at k = 25 a pixel's channels start at a 4-byte boundary only.
// One pass over each map, no LDS, no scratch.  The variant is wave-uniform: its branches are scalar.
#include "mp_kernels.hpp"

namespace mp {

using namespace mpcv;

namespace {

template <int VW>
struct Pack {
  float v[VW];
};

template <int VW>
__device__ __forceinline__ Pack<VW> ld(const float* __restrict__ p, int64_t e) {
  Pack<VW> r;
  if constexpr (VW == 4) {
    const f32x4 t = *reinterpret_cast<const f32x4*>(p + e);
#pragma unroll
    for (int j = 0; j < 4; ++j) r.v[j] = t[j];
  } else {
    r.v[0] = p[e];
  }
  return r;
}

template <int VW>
__device__ __forceinline__ void st(float* __restrict__ p, int64_t e, const Pack<VW>& r) {
  if constexpr (VW == 4)
    *reinterpret_cast<f32x4*>(p + e) = f32x4{r.v[0], r.v[1], r.v[2], r.v[3]};
  else
    p[e] = r.v[0];
}

template <int VW>
__device__ __forceinline__ Pack<VW> zero() {
  Pack<VW> r;
#pragma unroll
  for (int j = 0; j < VW; ++j) r.v[j] = 0.f;
  return r;
}

}  // namespace

// input half: I' = rule_in(P1, X, O, I, g1p) -> a.I (in place)
template <int NL, int VW>
__global__ __launch_bounds__(256) void circuit_nhwc_in_kernel(CnArgs a, int64_t nitem) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= nitem) return;
  const CircuitVariant v = a.v;
  const int64_t e = i * VW;
  const int k = a.k, c = (int)(e % k);
  const bool reads_o = v.integration != INT_MELY, reads_i = reads_prev_i(v);
  const Pack<VW> pv = ld<VW>(a.P, e), xv = ld<VW>(a.X, e);
  const Pack<VW> ov = reads_o ? ld<VW>(a.O, e) : zero<VW>();
  const Pack<VW> iv = reads_i ? ld<VW>(a.I, e) : zero<VW>();
  const Pack<VW> gv = v.blend_in ? ld<VW>(a.G, e) : zero<VW>();
  const Pack<VW> lat = ld<VW>(a.vecs, V_LAT * k + c), be = ld<VW>(a.vecs, V_BETA * k + c);
  const Pack<VW> nu = ld<VW>(a.vecs, V_NU * k + c), xi = ld<VW>(a.vecs, CV_XI * k + c);
  Pack<VW> o;
#pragma unroll
  for (int j = 0; j < VW; ++j)
    o.v[j] = rule_in<NL>(v, pv.v[j], xv.v[j], ov.v[j], iv.v[j], gv.v[j], InConst{lat.v[j], be.v[j], nu.v[j], xi.v[j]});
  st<VW>(a.I, e, o);
}

// output half: O' = rule_out(P2, I', O, g2p, rho[t]) -> a.O (in place), and on the last step also the
// NHWC result a.out
template <int NL, int VW>
__global__ __launch_bounds__(256) void circuit_nhwc_out_kernel(CnArgs a, int64_t nitem) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= nitem) return;
  const CircuitVariant v = a.v;
  const int64_t e = i * VW;
  const int k = a.k, c = (int)(e % k);
  const Pack<VW> pv = ld<VW>(a.P, e), iv = ld<VW>(a.I, e);
  const Pack<VW> ov = v.blend_out ? ld<VW>(a.O, e) : zero<VW>();
  const Pack<VW> gv = v.blend_out ? ld<VW>(a.G, e) : zero<VW>();
  const Pack<VW> lat = ld<VW>(a.vecs, V_LAT * k + c), ga = ld<VW>(a.vecs, V_GAMMA * k + c);
  const Pack<VW> ka = ld<VW>(a.vecs, V_KAPPA * k + c), om = ld<VW>(a.vecs, V_OMEGA * k + c);
  const Pack<VW> ze = ld<VW>(a.vecs, CV_ZETA * k + c);
  Pack<VW> o;
#pragma unroll
  for (int j = 0; j < VW; ++j)
    o.v[j] = rule_out<NL>(v, pv.v[j], iv.v[j], ov.v[j], gv.v[j], a.rho,
                          OutConst{lat.v[j], ga.v[j], ka.v[j], om.v[j], ze.v[j]});
  st<VW>(a.O, e, o);
  if (a.out) st<VW>(a.out, e, o);
}

// the gated conv input of the value just computed: dst = src * sigmoid(gp), gp the 1x1 gate conv's
// output (bias included).  Per element, whatever k is: 16-byte accesses whenever the map's length allows
template <int VW>
__global__ __launch_bounds__(256) void circuit_gate_kernel(const float* __restrict__ src, const float* __restrict__ gp,
                                                           float* __restrict__ dst, int64_t nitem) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= nitem) return;
  const int64_t e = i * VW;
  const Pack<VW> s = ld<VW>(src, e), g = ld<VW>(gp, e);
  Pack<VW> o;
#pragma unroll
  for (int j = 0; j < VW; ++j) o.v[j] = s.v[j] * sigmoid(g.v[j]);
  st<VW>(dst, e, o);
}

namespace {

template <int NL, int VW>
void launch_half(int half, const CnArgs& a, int64_t nitem, hipStream_t st) {
  const dim3 grid((unsigned)((nitem + 255) / 256));
  if (half == 0)
    hipLaunchKernelGGL((circuit_nhwc_in_kernel<NL, VW>), grid, dim3(256), 0, st, a, nitem);
  else
    hipLaunchKernelGGL((circuit_nhwc_out_kernel<NL, VW>), grid, dim3(256), 0, st, a, nitem);
}

template <int VW>
hipError_t launch_nl(int half, const CnArgs& a, int64_t nitem, hipStream_t st) {
  switch (a.v.nl) {
    case NL_TANH: launch_half<NL_TANH, VW>(half, a, nitem, st); break;
    case NL_RELU: launch_half<NL_RELU, VW>(half, a, nitem, st); break;
    case NL_SELU: launch_half<NL_SELU, VW>(half, a, nitem, st); break;
    case NL_LEAKY_RELU: launch_half<NL_LEAKY_RELU, VW>(half, a, nitem, st); break;
    case NL_HARD_TANH: launch_half<NL_HARD_TANH, VW>(half, a, nitem, st); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

// maps of up to 2^24 pixels x 256 channels: at most 2^32 elements, 2^22 blocks of 256 float4 items
constexpr int64_t CN_MAX_ELEMS = (int64_t)1 << 32;

hipError_t launch_cn(int half, const CnArgs& a, hipStream_t st) {
  if (a.k < 1 || a.npix < 1 || a.npix * a.k > CN_MAX_ELEMS || a.v.integration >= INT_COUNT) return hipErrorInvalidValue;
  const int64_t total = a.npix * a.k;
  return a.k % 4 == 0 ? launch_nl<4>(half, a, total / 4, st) : launch_nl<1>(half, a, total, st);
}

}  // namespace

hipError_t launch_circuit_nhwc_in(const CnArgs& a, hipStream_t st) {
  if (!a.P || !a.X || !a.O || !a.I || !a.vecs || (a.v.blend_in && !a.G)) return hipErrorInvalidValue;
  return launch_cn(0, a, st);
}

hipError_t launch_circuit_nhwc_out(const CnArgs& a, hipStream_t st) {
  if (!a.P || !a.O || !a.I || !a.vecs || (a.v.blend_out && !a.G)) return hipErrorInvalidValue;
  return launch_cn(1, a, st);
}

hipError_t launch_circuit_nhwc_gate(const float* src, const float* gp, float* dst, int64_t total, hipStream_t st) {
  if (!src || !gp || !dst || total < 1 || total > CN_MAX_ELEMS) return hipErrorInvalidValue;
  const bool v4 = total % 4 == 0;
  const int64_t nitem = v4 ? total / 4 : total;
  const dim3 grid((unsigned)((nitem + 255) / 256));
  if (v4)
    hipLaunchKernelGGL(circuit_gate_kernel<4>, grid, dim3(256), 0, st, src, gp, dst, nitem);
  else
    hipLaunchKernelGGL(circuit_gate_kernel<1>, grid, dim3(256), 0, st, src, gp, dst, nitem);
  return hipGetLastError();
}

}  // namespace mp
