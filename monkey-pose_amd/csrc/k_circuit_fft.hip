// The channel-general loop's FFT association-field conv (mp_circuit_set_nhwc_conv MP_CN_CONV_FFT and
// MP_CN_CONV_FFT_TILED): the SAME conv P = p_r * A of NHWC fp32 maps [n, h, w, k], k % 4 == 0, as three
// launches over the map's tiles (circuit_fft.hpp: the tile plan; one tile when h, w <= 64, which is all
// MP_CN_CONV_FFT takes, else overlap-save windows of 64 x 64)
//   cn_fft_fwd    A [n,h,w,k]  -> S   72 x 72 real-input FFT per (tile, 4-channel group), f16 hi / lo split
//   cn_spec_gemm  S, Gc        -> Y   per frequency Y[b][co] = sum_ci S[b][ci] G[ci][co], f16x3 on the matrix cores
//   cn_fft_inv    Y            -> P   inverse FFT, the pixels the tile owns stored at their map position
// on the 72-point transforms of fft_dev.hpp.  Layouts and the padding rules: circuit_fft.hpp.  The
// 64-channel loops keep their own kernels (k_fft.hip, k_fft4.hip); nothing here is shared with them
// but fft_dev.hpp.
//
// Every kernel computes a tile from that tile alone and in an order that depends on k alone, so an
// output does not depend on the batch, on the image's place in it or on the conv chunk its tiles fall in.
//
// Range: S holds SPEC_SCALE * (the transform of a window), bounded by SPEC_SCALE * sum|v| over the window,
// in f16: a conv input must keep min(h, 64) * min(w, 64) * max|v| / 64 inside f16 range (65504), as on the
// 64-channel FFT path.
#include "circuit_fft.hpp"
#include "fft_dev.hpp"
#include "mp_kernels.hpp"

namespace mp {

namespace {

static_assert(CNF_NF == NF, "circuit_fft.hpp restates the frequency count");
constexpr int CF_TLD = 65;                  // pitch (complex) of the forward transpose T[fx][c][y]
constexpr int CF_RLD = 73;                  // pitch (complex) of the inverse's parked rows R[2 y + p][x]
constexpr int CF_LDS = FX * 4 * CF_TLD;     // complex elements of a transform block's LDS (76,960 B)
static_assert(128 * CF_RLD <= CF_LDS && 64 * 4 * FX <= CF_LDS, "LDS plan of the inverse");
constexpr int CF_FS = FX * 4;               // stride of one fy step in 8-byte units (f = fy * 37 + fx)

// Block -> (tile, channel group), XCD-aware.  The k / 4 groups of a pixel are 16 bytes each, so eight
// neighbouring groups share every 128-byte line of the map; workgroups are dispatched round-robin over
// the 8 XCDs (blocks i and i + 8 share one), so the eight groups of a (tile, line) unit are placed 8
// blocks apart: one L2 moves each line once.  64 blocks = 8 units x 8 groups.
__device__ __forceinline__ bool cf_block(int blk, int n, int nq, int& b, int& cq) {
  const int nl = (nq + 7) >> 3;
  const int within = blk & 63, unit = (blk >> 6) * 8 + (within & 7);
  b = unit / nl;
  cq = 8 * (unit - b * nl) + (within >> 3);
  return b < n && cq < nq;
}
int cf_grid(int n, int k) { return (n * ((cnf_nq(k) + 7) / 8) + 7) / 8 * 64; }

// The tiles of a launch: tile t of the launch is tile t0 + t of the maps' n * ty * tx, image-major then
// tile row then tile column, and S / Y hold it at index t (a conv chunk may begin and end inside an image).
struct CfTile {
  int b;        // image
  int oy, ox;   // map position of the window's local (0, 0); negative in a leading halo
  int ly, lx;   // local index of the first output the tile owns
  int py, px;   // its map position
  int cy, cx;   // outputs the tile owns
};
// TILED false: every image is one tile (g.ty == g.tx == 1, h, w <= 64), the plan's constants folded
template <bool TILED>
__device__ __forceinline__ CfTile cf_tile(const CnfMap& g, int t) {
  if constexpr (!TILED) return CfTile{g.t0 + t, 0, 0, 0, 0, 0, 0, g.H, g.W};
  const int gt = g.t0 + t, tpi = g.ty * g.tx;
  CfTile r;
  r.b = gt / tpi;
  const int rem = gt - r.b * tpi, iy = rem / g.tx, ix = rem - iy * g.tx;
  r.oy = cnf_tile_origin(g.H, g.ssf, iy);
  r.ox = cnf_tile_origin(g.W, g.ssf, ix);
  r.ly = cnf_tile_out0(g.H, g.ssf);
  r.lx = cnf_tile_out0(g.W, g.ssf);
  r.py = cnf_tile_pos(g.H, g.ssf, iy);
  r.px = cnf_tile_pos(g.W, g.ssf, ix);
  r.cy = cnf_tile_count(g.H, g.ssf, iy);
  r.cx = cnf_tile_count(g.W, g.ssf, ix);
  return r;
}

// forward: one block per (tile, 4-channel group).  Row phase (128 threads): window row y, channel pair
// p, the two real rows packed as one complex transform; LDS transpose; column phase (148 threads):
// column (fx, c) of the 37-column half spectrum.  Window rows and columns outside the map are zeros of the
// transform: such rows, leading or trailing, are neither loaded nor transformed (the column phase
// reads them as zeros, never from LDS), such columns are loaded from a clamped (live) address and
// zeroed.  The two instantiations run the same arithmetic in the same order: a map of one tile gives the
// same bytes through either (the launchers send it through TILED false, MP_CN_CONV_FFT's kernel).
template <bool TILED>
__global__ __launch_bounds__(FNT, 2) void cn_fft_fwd_kernel(const float* __restrict__ src, void* __restrict__ S, int n,
                                                            CnfMap g, int k) {
  __shared__ cpx T[CF_LDS];
  int b, cq;
  if (!cf_block(blockIdx.x, n, k >> 2, b, cq)) return;
  const CfTile tl = cf_tile<TILED>(g, b);
  const int H = g.H, W = g.W;
  const int tid = threadIdx.x;
  if (tid < 128) {
    const int y = tid >> 1, p = tid & 1;
    const int my = tl.oy + y;
    if (my >= 0 && my < H) {   // a lane pair shares y: both lanes of every DPP exchange below are active
      cpx v[72];
      // lane p of the row's pair loads all 4 channels of pixel 2 j + p (one 16-byte load at stride 4 k
      // bytes), then the pair swaps the channel pair the other lane transforms (quad_perm [1,0,3,2])
      const float* row = src + ((size_t)tl.b * H + my) * W * k + 4 * cq;
#pragma unroll
      for (int j = 0; j < 32; ++j) {
        const int x = tl.ox + 2 * j + p;
        f32x4 u = *reinterpret_cast<const f32x4*>(row + (size_t)min(max(x, 0), W - 1) * k);
        if (x < 0 || x >= W) u = f32x4{0.f, 0.f, 0.f, 0.f};
        const cpx lo = {u[0], u[1]}, hi = {u[2], u[3]};
        const cpx mine = p ? hi : lo, send = p ? lo : hi;
        const cpx recv = {__int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(send.x), 0xB1, 0xF, 0xF, false)),
                          __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(send.y), 0xB1, 0xF, 0xF, false))};
        v[2 * j] = p ? recv : mine;
        v[2 * j + 1] = p ? mine : recv;
      }
#pragma unroll
      for (int x = 64; x < 72; ++x) v[x] = {0.f, 0.f};
      fft72<-1>(v);
      // Z = FFT(a + i b):  A[f] = (Z[f] + conj Z[-f]) / 2,  B[f] = (Z[f] - conj Z[-f]) / (2i)
#pragma unroll
      for (int f = 0; f < FX; ++f) {
        const cpx zk = v[f], zm = v[(72 - f) % 72];
        const cpx A = cfma(zm, cpx{1.f, -1.f}, zk) * 0.5f;
        const cpx B = cfma(swp(zk), cpx{1.f, -1.f}, swp(zm)) * 0.5f;
        T[(f * 4 + 2 * p) * CF_TLD + y] = A;
        T[(f * 4 + 2 * p + 1) * CF_TLD + y] = B;
      }
    }
  }
  lds_barrier();
  if (tid >= FX * 4) return;
  const int fx = tid >> 2, c = tid & 3;
  cpx v[72];
#pragma unroll
  for (int y = 0; y < 72; ++y)   // rows outside the map: never written
    v[y] = (y < 64 && tl.oy + y >= 0 && tl.oy + y < H) ? T[tid * CF_TLD + y] : cpx{0.f, 0.f};
  fft72<-1>(v);
  // the 32-byte entry of (f, cq): [hi c0 | hi c1 | hi c2 | hi c3 | lo c0 | lo c1 | lo c2 | lo c3], 4 B
  // each = f16 (re, im); lane c of the quad stores bytes 8 c .. 8 c + 7 (two quad_perms regroup the
  // halves), so at one fy a wave's 16 columns x 4 channels are 512 contiguous bytes
  typedef unsigned u32x2_t __attribute__((ext_vector_type(2)));
  u32x2_t* dst = reinterpret_cast<u32x2_t*>(S) + (((size_t)b * (k >> 2) + cq) * NF + fx) * 4 + c;
  const bool hi_half = c < 2;
#pragma unroll
  for (int fy = 0; fy < 72; ++fy) {
    const float re = v[fy].x * SPEC_SCALE, im = v[fy].y * SPEC_SCALE;
    const _Float16 hr = (_Float16)re, hm = (_Float16)im;
    const f16x2 hv = {hr, hm}, lv = {(_Float16)(re - (float)hr), (_Float16)(im - (float)hm)};
    const int hb = __builtin_bit_cast(int, hv), lb = __builtin_bit_cast(int, lv);
    const int h0 = __builtin_amdgcn_mov_dpp(hb, 0x88, 0xF, 0xF, false);   // quad_perm [0,2,0,2]
    const int l0 = __builtin_amdgcn_mov_dpp(lb, 0x88, 0xF, 0xF, false);
    const int h1 = __builtin_amdgcn_mov_dpp(hb, 0xDD, 0xF, 0xF, false);   // quad_perm [1,3,1,3]
    const int l1 = __builtin_amdgcn_mov_dpp(lb, 0xDD, 0xF, 0xF, false);
    const u32x2_t w = {(unsigned)(hi_half ? h0 : l0), (unsigned)(hi_half ? h1 : l1)};
    __builtin_nontemporal_store(w, dst + fy * CF_FS);
  }
}

// inverse: Y -> P, the forward kernel run backwards (columns, LDS transpose, Hermitian-extended row
// pairs; only the window rows that hold outputs), the rows parked in LDS and the cy x cx pixels the tile
// owns stored pixel-major at their map position, 16 bytes each, times unscale
template <bool TILED>
__global__ __launch_bounds__(FNT, 2) void cn_fft_inv_kernel(const void* __restrict__ Y, float* __restrict__ P, int n,
                                                            CnfMap g, int k, float unscale) {
  __shared__ cpx T[CF_LDS];
  int b, cq;
  if (!cf_block(blockIdx.x, n, k >> 2, b, cq)) return;
  const CfTile tl = cf_tile<TILED>(g, b);
  const int tid = threadIdx.x;
  if (tid < FX * 4) {
    const int fx = tid >> 2, c = tid & 3;
    const cpx* src = static_cast<const cpx*>(Y) + (((size_t)b * (k >> 2) + cq) * NF + fx) * 4 + c;
    cpx v[72];
#pragma unroll
    for (int fy = 0; fy < 72; ++fy) v[fy] = src[fy * CF_FS];
    fft72<1>(v);
#pragma unroll
    for (int y = 0; y < 64; ++y) T[(y * 4 + c) * FX + fx] = v[y];
  }
  lds_barrier();
  const int y = tid >> 1, p = tid & 1;
  const bool live = tid < 128 && y >= tl.ly && y < tl.ly + tl.cy;
  {
    cpx v[72];
    if (live) {
      // C[f] = A[f] + i B[f];  C[72 - f] from A[72 - f] = conj A[f], B[72 - f] = conj B[f]
      const int ta = (y * 4 + 2 * p) * FX, tb = ta + FX;
#pragma unroll
      for (int f = 0; f < FX; ++f) {
        const cpx A = T[ta + f], B = T[tb + f];
        v[f] = cfma(swp(B), cpx{-1.f, 1.f}, A);
        if (f > 0 && f < FX - 1) v[72 - f] = cfma(A, cpx{1.f, -1.f}, swp(B));
      }
      fft72<1>(v);
    }
    lds_barrier();   // every inverse row has read T
    if (live) {
#pragma unroll
      for (int x = 0; x < 64; ++x) T[tid * CF_RLD + x] = v[x];
    }
  }
  lds_barrier();
  float* dst = P + (((size_t)tl.b * g.H + tl.py) * g.W + tl.px) * k + 4 * cq;
  for (int i = tid; i < tl.cy * tl.cx; i += FNT) {
    const int yy = i / tl.cx, x = i - yy * tl.cx;
    const int r = 2 * (tl.ly + yy) * CF_RLD + tl.lx + x;
    const cpx a = T[r], c = T[r + CF_RLD];
    *reinterpret_cast<f32x4*>(dst + ((size_t)yy * g.W + x) * k) = f32x4{a.x, a.y, c.x, c.y} * unscale;
  }
}

// spectral product: per frequency f the real product D[m][j] = sum_kk A[m][kk] Bm[kk][j] on
// v_mfma_f32_32x32x16_f16 in the f16x3 split (lo hi + hi lo + hi hi, fp32 accumulation), with
//   m  = output row: (re | im) of output channel co, 128 rows = 64 channels per block (an M range),
//   kk = 2 ci + (re | im) of input channel ci, a K step of 16 = the two channel groups 2 t, 2 t + 1,
//   j  = image, 32 per block.
// B fragment (lane half h, image j; K step t): the 8 hi (lo) halves of S group 2 t + h of image j.
// A fragment (lane half h, row i): (re, im) of G[ci = 8 t + 4 h .. + 3][co], with the imaginary halves
// negated for the re rows (gr, -gi) and the halves swapped for the im rows (gi, gr), derived in
// registers from the compact weights Gc.  Block = 4 consecutive frequencies (one per wave; one 128-B
// line of S / Y per (image, group)) x 32 images x one M range; the S tile is staged in LDS in K chunks
// of 8 groups (32 channels: [group][hi|lo][f][image], 33,792 B), the Y tile leaves through the same LDS
// one 32-channel block at a time.  Padding: a group past k / 4 (the second half of the last K step when
// k % 8 == 4, and the rest of the last chunk) is WRITTEN as zeros in LDS -- its weights are zero, but
// 0 x (whatever the LDS held) is not; output channels past k carry zero weights and are not stored;
// images past B are computed from clamped loads and dropped.  The blocks of one frequency quad run on
// one XCD (its weights leave HBM once).  Two blocks per CU: budgeted for three (168 VGPRs) the chunk's
// hoisted weight loads, the 64 accumulators and the next chunk's S lines spill 92 B / lane.
constexpr int CG_KC = 8;                          // channel groups per K chunk
constexpr int CG_SLD = CNF_NI + 1;                // S tile pitch (16-B units) per (group, part, f) row
constexpr int CG_YLD = 8 * 4 * 2 + 1;             // Y tile pitch (16-B units) per image
constexpr int CG_TILE = CG_KC * 2 * 4 * CG_SLD;   // 2112 x 16 B
static_assert(CNF_NI * CG_YLD <= CG_TILE, "the Y tile fits in the S tile's space");
constexpr int NQUAD = NF / 4;                     // 666 frequency quads
static_assert(NF % 4 == 0, "frequency quads");

__global__ __launch_bounds__(256, 2) void cn_spec_gemm_kernel(const uint4* __restrict__ S, const uint4* __restrict__ Gc,
                                                              uint4* __restrict__ Y, int B, int ngrp, int k) {
  __shared__ uint4 tile[CG_TILE];
  const int nq = k >> 2, cqp = cnf_cqp(k), cop = cnf_cop(k), nmr = cnf_nmr(k);
  const int inner = ngrp * nmr;
  const int q8 = blockIdx.x / (8 * inner), rem = blockIdx.x - q8 * 8 * inner;
  const int in = rem >> 3, quad = q8 * 8 + (rem & 7);
  if (quad >= NQUAD) return;
  const int grp = in / nmr, mr = in - grp * nmr;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, h = lane >> 5, j = lane & 31;
  const int img0 = grp * CNF_NI;
  const int f = 4 * quad + wv;
  const bool live1 = 64 * mr + 32 < cop;   // the M range's second 32-channel block exists
  const int nchunk = (nq + CG_KC - 1) / CG_KC, nt = cqp >> 1;
  // the chunk's S lines: 32 images x 8 groups x 128 B (4 f x [hi 16 B | lo 16 B]), 8 pieces a thread;
  // unconditional loads from clamped addresses, zeroed on the way into LDS
  uint4 pre[8];
  auto load_s = [&](int kc) {
#pragma unroll
    for (int it = 0; it < 8; ++it) {
      const int idx = it * 256 + tid, line = idx >> 3, piece = idx & 7;
      const int bl = line >> 3, cq = min(CG_KC * kc + (line & 7), nq - 1);
      const int b = min(img0 + bl, B - 1);
      pre[it] = S[(((size_t)b * nq + cq) * NF + 4 * quad) * 2 + piece];
    }
  };
  load_s(0);
  const uint4* gw = Gc + (size_t)f * 2 * cqp * cop + 64 * mr + j;
  const size_t gpart = (size_t)cqp * cop;
  f32x16 acc[4] = {};
  const uint4 m = {0x80000000u, 0x80000000u, 0x80000000u, 0x80000000u};
  for (int kc = 0; kc < nchunk; ++kc) {
#pragma unroll
    for (int it = 0; it < 8; ++it) {
      const int idx = it * 256 + tid, line = idx >> 3, piece = idx & 7;
      const int bl = line >> 3, cql = line & 7, ff = piece >> 1, part = piece & 1;
      const bool ok = img0 + bl < B && CG_KC * kc + cql < nq;
      tile[((cql * 2 + part) * 4 + ff) * CG_SLD + bl] = ok ? pre[it] : uint4{0, 0, 0, 0};
    }
    lds_barrier();
#pragma unroll
    for (int tt = 0; tt < CG_KC / 2; ++tt) {
      const int t = (CG_KC / 2) * kc + tt;
      if (t < nt) {   // block-uniform
        const int cql = 2 * tt + h;
        const uint4* g = gw + (size_t)(2 * t + h) * cop;
        const f16x8 sh = __builtin_bit_cast(f16x8, tile[((cql * 2 + 0) * 4 + wv) * CG_SLD + j]);
        const f16x8 sl = __builtin_bit_cast(f16x8, tile[((cql * 2 + 1) * 4 + wv) * CG_SLD + j]);
#pragma unroll
        for (int cb = 0; cb < 2; ++cb) {
          if (cb == 0 || live1) {
            const uint4 gh = g[32 * cb], gl = g[gpart + 32 * cb];
            // re rows: (gr, -gi) pairs; im rows: (gi, gr) pairs
            const f16x8 ah0 = __builtin_bit_cast(f16x8, gh ^ m), al0 = __builtin_bit_cast(f16x8, gl ^ m);
            const f16x8 ah1 = __builtin_bit_cast(f16x8, (gh >> 16) | (gh << 16));
            const f16x8 al1 = __builtin_bit_cast(f16x8, (gl >> 16) | (gl << 16));
            acc[cb] = mfma16(al0, sh, acc[cb]);
            acc[cb] = mfma16(ah0, sl, acc[cb]);
            acc[cb] = mfma16(ah0, sh, acc[cb]);
            acc[2 + cb] = mfma16(al1, sh, acc[2 + cb]);
            acc[2 + cb] = mfma16(ah1, sl, acc[2 + cb]);
            acc[2 + cb] = mfma16(ah1, sh, acc[2 + cb]);
          }
        }
      }
    }
    if (kc + 1 < nchunk) load_s(kc + 1);   // in flight across the barrier: the other waves' products cover it
    lds_barrier();   // every wave has read the tile
  }
  // ---- Y: lane (h, j), block cb, row group g: channels 64 mr + 32 cb + 8 g + 4 h + e, e < 4 ----
  f32x4* ytile = reinterpret_cast<f32x4*>(tile);
  auto store_block = [&](int cb, const f32x16& re, const f32x16& im) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int cql = 2 * g + h;
      ytile[j * CG_YLD + (cql * 4 + wv) * 2] = f32x4{re[4 * g], im[4 * g], re[4 * g + 1], im[4 * g + 1]};
      ytile[j * CG_YLD + (cql * 4 + wv) * 2 + 1] = f32x4{re[4 * g + 2], im[4 * g + 2], re[4 * g + 3], im[4 * g + 3]};
    }
    lds_barrier();
#pragma unroll
    for (int it = 0; it < 8; ++it) {
      const int idx = it * 256 + tid, line = idx >> 3, piece = idx & 7;
      const int bl = line >> 3, cql = line & 7, b = img0 + bl, cqo = 16 * mr + 8 * cb + cql;
      if (b < B && cqo < nq) st16(Y + (((size_t)b * nq + cqo) * NF + 4 * quad) * 2 + piece, tile[bl * CG_YLD + cql * 8 + piece]);
    }
    lds_barrier();
  };
  store_block(0, acc[0], acc[2]);
  if (live1) store_block(1, acc[1], acc[3]);   // block-uniform
}

// spectral weights at finalize, G[f][ci][co] = sum_taps w[ky][kx][ci][co] e^{-2 pi i (fy (R - ky) + fx (R - kx)) / 72} / 72^2
// (float64 accumulation, rounded to fp32), one thread per (f, group cq, co) = 4 ci: PACK 0 takes
// max|G| (one atomic per wave), PACK 1 writes the compact split weights, zeros in the padding.  No
// fp32 G is kept (1.4 GB at k = 256): the second pass computes it again.
template <int PACK>
__global__ __launch_bounds__(256) void cn_spec_weights_kernel(const float* __restrict__ w, int KS, int k, float wscale,
                                                              unsigned* __restrict__ mx, f16x8* __restrict__ Gc) {
  __shared__ double tc[FFT_N], ts[FFT_N];
  for (int i = threadIdx.x; i < FFT_N; i += blockDim.x) {
    double s, c;
    sincospi(2.0 * i / FFT_N, &s, &c);
    tc[i] = c;
    ts[i] = s;
  }
  __syncthreads();
  const int cqp = cnf_cqp(k), cop = cnf_cop(k);
  const size_t total = (size_t)NF * cqp * cop;
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  float amax = 0.f;
  if (idx < total) {
    const int co = (int)(idx % cop), cq = (int)(idx / cop % cqp), f = (int)(idx / ((size_t)cop * cqp));
    const int fy = f / FX, fx = f - fy * FX, R = KS / 2;
    double gr[4] = {0.0, 0.0, 0.0, 0.0}, gi[4] = {0.0, 0.0, 0.0, 0.0};
    if (co < k && 4 * cq < k) {   // k % 4 == 0: a group is whole or padding
      for (int ky = 0; ky < KS; ++ky)
        for (int kx = 0; kx < KS; ++kx) {
          int mm = (fy * (R - ky) + fx * (R - kx)) % FFT_N;
          if (mm < 0) mm += FFT_N;
          const double c = tc[mm], s = ts[mm];
          const float* wp = w + ((size_t)(ky * KS + kx) * k + 4 * cq) * k + co;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const double v = wp[(size_t)e * k];
            gr[e] += v * c;      // exp(-i theta) = cos - i sin
            gi[e] -= v * s;
          }
        }
    }
    const double inv = 1.0 / ((double)FFT_N * FFT_N);
    f16x8 hv, lv;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float g2[2] = {(float)(gr[e] * inv), (float)(gi[e] * inv)};
#pragma unroll
      for (int ri = 0; ri < 2; ++ri) {
        amax = fmaxf(amax, fabsf(g2[ri]));
        const float v = g2[ri] * wscale;
        const _Float16 hh = (_Float16)v;
        hv[2 * e + ri] = hh;
        lv[2 * e + ri] = (_Float16)(v - (float)hh);
      }
    }
    if constexpr (PACK) {
      Gc[((size_t)(f * 2 + 0) * cqp + cq) * cop + co] = hv;
      Gc[((size_t)(f * 2 + 1) * cqp + cq) * cop + co] = lv;
    }
  }
  if constexpr (!PACK) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) amax = fmaxf(amax, __shfl_xor(amax, o));
    if ((threadIdx.x & 63) == 0) atomicMax(mx, __float_as_uint(amax));   // non-negative floats order like their bits
  }
}

}  // namespace

hipError_t build_cn_spec_weights(const float* w, int ks, int k, void* Gc, float* unscale) {
  unsigned* mx = nullptr;
  hipError_t e = hipMalloc(&mx, sizeof(unsigned));
  if (e == hipSuccess) e = hipMemset(mx, 0, sizeof(unsigned));
  const size_t total = (size_t)NF * cnf_cqp(k) * cnf_cop(k);
  const dim3 grid((unsigned)((total + 255) / 256));
  if (e == hipSuccess) {
    hipLaunchKernelGGL(cn_spec_weights_kernel<0>, grid, dim3(256), 0, 0, w, ks, k, 1.0f, mx, static_cast<f16x8*>(nullptr));
    e = hipGetLastError();
  }
  unsigned bits = 0;
  if (e == hipSuccess) e = hipMemcpy(&bits, mx, sizeof(unsigned), hipMemcpyDeviceToHost);
  if (e == hipSuccess) {
    // one power-of-two scale per tensor putting max|G| at 2^13..2^14 (f16 max is 65504)
    float m;
    std::memcpy(&m, &bits, sizeof m);
    int ex = 0;
    if (m > 0.f) std::frexp(m, &ex);
    const float wscale = std::ldexp(1.0f, 14 - ex);
    *unscale = 1.0f / (wscale * SPEC_SCALE);
    hipLaunchKernelGGL(cn_spec_weights_kernel<1>, grid, dim3(256), 0, 0, w, ks, k, wscale, mx, static_cast<f16x8*>(Gc));
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (mx) (void)hipFree(mx);
  return e;
}

hipError_t launch_cn_fft_fwd(const float* act, void* S, int n, const CnfMap& g, int k, hipStream_t st) {
  if (g.ty * g.tx == 1)
    hipLaunchKernelGGL(cn_fft_fwd_kernel<false>, dim3(cf_grid(n, k)), dim3(FNT), 0, st, act, S, n, g, k);
  else
    hipLaunchKernelGGL(cn_fft_fwd_kernel<true>, dim3(cf_grid(n, k)), dim3(FNT), 0, st, act, S, n, g, k);
  return hipGetLastError();
}

hipError_t launch_cn_spec_gemm(const void* S, const void* Gc, void* Y, int n, int k, hipStream_t st) {
  const int ngrp = (n + CNF_NI - 1) / CNF_NI, nq8 = (NQUAD + 7) / 8;
  hipLaunchKernelGGL(cn_spec_gemm_kernel, dim3(nq8 * 8 * ngrp * cnf_nmr(k)), dim3(256), 0, st,
                     static_cast<const uint4*>(S), static_cast<const uint4*>(Gc), static_cast<uint4*>(Y), n, ngrp, k);
  return hipGetLastError();
}

hipError_t launch_cn_fft_inv(const void* Y, float* P, int n, const CnfMap& g, int k, float unscale, hipStream_t st) {
  if (g.ty * g.tx == 1)
    hipLaunchKernelGGL(cn_fft_inv_kernel<false>, dim3(cf_grid(n, k)), dim3(FNT), 0, st, Y, P, n, g, k, unscale);
  else
    hipLaunchKernelGGL(cn_fft_inv_kernel<true>, dim3(cf_grid(n, k)), dim3(FNT), 0, st, Y, P, n, g, k, unscale);
  return hipGetLastError();
}

}  // namespace mp
