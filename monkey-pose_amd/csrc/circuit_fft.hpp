// Geometry of the channel-general loop's FFT association-field conv (k_circuit_fft.hip), shared by its
// kernels, its launchers and the host loop (mp_abi.hip cn_conv_fft): plain host / device constexpr
// arithmetic on the channel count k (k % 4 == 0, 4 <= k <= 256).
//
//   spectra  S[b][cq][f]  cq < k / 4 channel groups, f = fy * 37 + fx < 2664, 32 B per entry:
//                         8 f16 hi | 8 f16 lo of SPEC_SCALE * (re, im) of channels 4 cq .. 4 cq + 3
//            Y[b][cq][f]  the same index, 4 complex64
//   weights  Gc[f][hi|lo][cq < cqp][co < cop]  one f16x8 = (re, im) of G[ci = 4 cq .. 4 cq + 3][co] * wscale,
//                         cqp = k / 4 rounded up to even (a K step of the product is two groups),
//                         cop = k rounded up to 32 (an M block); the padding is zeros
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace mp {

constexpr int CNF_NF = 72 * 37;          // frequencies of the 72 x 72 real-input transform
constexpr int CNF_MAX_HW = 64;           // largest map side: 64 + 15 / 2 = 71 <= 72, no wrap-around
constexpr int CNF_NI = 32;               // images per spectral-product tile
constexpr size_t CNF_WS_BYTES = (size_t)1 << 30;   // S + Y of one conv chunk

__host__ __device__ constexpr int cnf_nq(int k) { return (k + 3) / 4; }
__host__ __device__ constexpr int cnf_cqp(int k) { return (cnf_nq(k) + 1) / 2 * 2; }
__host__ __device__ constexpr int cnf_cop(int k) { return (k + 31) / 32 * 32; }
__host__ __device__ constexpr int cnf_nmr(int k) { return (k + 63) / 64; }      // 128-row M ranges
// bytes of one image's S (or Y)
__host__ __device__ constexpr size_t cnf_image_bytes(int k) { return (size_t)cnf_nq(k) * CNF_NF * 32; }
// images per conv chunk: the largest multiple of the product's image tile whose S + Y fit
// CNF_WS_BYTES, and at least one tile
__host__ __device__ constexpr int cnf_chunk(int k) {
  const size_t t = CNF_WS_BYTES / (2 * cnf_image_bytes(k)) / CNF_NI;
  return (int)(t < 1 ? 1 : t) * CNF_NI;
}
__host__ __device__ constexpr size_t cnf_weight_bytes(int k) {
  return (size_t)CNF_NF * 2 * cnf_cqp(k) * cnf_cop(k) * 16;
}

}  // namespace mp
