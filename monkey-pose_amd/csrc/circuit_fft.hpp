// Geometry of the channel-general loop's FFT association-field conv (k_circuit_fft.hip), shared by its
// kernels, its launchers and the host loop (mp_abi.hip cn_conv_fft): plain host / device constexpr
// arithmetic on the channel count k (k % 4 == 0, 4 <= k <= 256) and on the map's tile plan.  An "image"
// b of the spectra is one 64 x 64 window of a map: the whole map under MP_CN_CONV_FFT, one tile of the
// plan below under MP_CN_CONV_FFT_TILED.
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
constexpr int CNF_MAX_HW = 64;           // largest window side: 64 + 15 / 2 = 71 <= 72, no wrap-around
constexpr int CNF_NI = 32;               // images (windows) per spectral-product tile
constexpr size_t CNF_WS_BYTES = (size_t)1 << 30;   // S + Y of one conv chunk

// The tile plan (overlap-save, MP_CN_CONV_FFT_TILED), separable per axis: an axis of length L under a
// filter of size ssf (radius R = ssf / 2) is cut into cnf_tiles(L, ssf) windows of CNF_MAX_HW positions.
//   L <= 64: one tile, window origin 0, the L outputs at local index 0 .. L - 1 (MP_CN_CONV_FFT's geometry:
//            the transform's zero pad 64 .. 71 absorbs the filter's reach)
//   L >  64: step T = 64 - 2 R; tile i owns map positions [i T, min((i + 1) T, L)), its window covers
//            [i T - R, i T - R + 64) (zeros outside the map) and its outputs sit at local index
//            R + (pos - i T), so every read local +- R stays inside [0, 63]
__host__ __device__ constexpr int cnf_tile_step(int ssf) { return CNF_MAX_HW - 2 * (ssf / 2); }
__host__ __device__ constexpr int cnf_tiles(int L, int ssf) {
  return L <= CNF_MAX_HW ? 1 : (L + cnf_tile_step(ssf) - 1) / cnf_tile_step(ssf);
}
// first map position tile i owns, map position of its window's local index 0, local index of its first
// output, number of positions it owns
__host__ __device__ constexpr int cnf_tile_pos(int L, int ssf, int i) { return L <= CNF_MAX_HW ? 0 : i * cnf_tile_step(ssf); }
__host__ __device__ constexpr int cnf_tile_origin(int L, int ssf, int i) {
  return L <= CNF_MAX_HW ? 0 : i * cnf_tile_step(ssf) - ssf / 2;
}
__host__ __device__ constexpr int cnf_tile_out0(int L, int ssf) { return L <= CNF_MAX_HW ? 0 : ssf / 2; }
__host__ __device__ constexpr int cnf_tile_count(int L, int ssf, int i) {
  return L <= CNF_MAX_HW ? L
                         : ((i + 1) * cnf_tile_step(ssf) < L ? cnf_tile_step(ssf) : L - i * cnf_tile_step(ssf));
}

// a map and the tiles of it one launch transforms: tiles t0 .. of the batch's n * ty * tx (image-major,
// then tile row, then tile column)
struct CnfMap {
  int H, W, ssf;   // map height and width, filter size
  int ty, tx;      // cnf_tiles(H, ssf), cnf_tiles(W, ssf)
  int t0;          // the launch's first tile
};

__host__ __device__ constexpr int cnf_nq(int k) { return (k + 3) / 4; }
__host__ __device__ constexpr int cnf_cqp(int k) { return (cnf_nq(k) + 1) / 2 * 2; }
__host__ __device__ constexpr int cnf_cop(int k) { return (k + 31) / 32 * 32; }
__host__ __device__ constexpr int cnf_nmr(int k) { return (k + 63) / 64; }      // 128-row M ranges
// bytes of one window's S (or Y)
__host__ __device__ constexpr size_t cnf_image_bytes(int k) { return (size_t)cnf_nq(k) * CNF_NF * 32; }
// windows per conv chunk: the largest multiple of the product's image tile whose S + Y fit
// CNF_WS_BYTES, and at least one tile
__host__ __device__ constexpr int cnf_chunk(int k) {
  const size_t t = CNF_WS_BYTES / (2 * cnf_image_bytes(k)) / CNF_NI;
  return (int)(t < 1 ? 1 : t) * CNF_NI;
}
__host__ __device__ constexpr size_t cnf_weight_bytes(int k) {
  return (size_t)CNF_NF * 2 * cnf_cqp(k) * cnf_cop(k) * 16;
}

}  // namespace mp
