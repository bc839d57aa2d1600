/* monkeypose.h -- C ABI of libmonkeypose.so, the MI355X (gfx950) inference path of the
 * monkey-pose regressors.
 *
 * The reference (krg-nandu/monkey-pose, TensorFlow 1.x / Python 2) has no FFI: its "operator API"
 * is a set of Python graph-builder classes.  Each entry point below replaces one of them; the
 * Python facade in monkey-pose_amd/ (hgru_pose.py, hgru_module.py) binds them with ctypes and
 * keeps the reference's class / method names and argument order.
 *
 *   reference interface                                        replaced by
 *   ---------------------------------------------------------  ------------------------------------
 *   hgru_pose.model.get_var / data_dict   hgru_pose.py:196-216  mp_set_weight, mp_finalize_weights
 *   hgru_pose.model.build(depth, output_shape, batch_norm,     mp_hgru_pose_fwd
 *     train_mode) -> .out_put             hgru_pose.py:47-105
 *   hgru_module.ContextualCircuit(X, timesteps, SRF, SSN, SSF, mp_hgru_circuit_fwd
 *     strides, padding, aux).build()      hgru_module.py:61-128, 872-959
 *   (tf.Session / device placement)       train_cnn_networks_hgru.py:95  mp_create / mp_destroy
 *
 * Conventions
 *   - Every tensor argument is a device pointer (hipMalloc'd or a torch CUDA tensor's data_ptr),
 *     fp32, contiguous, NHWC exactly as the reference feeds it (depth crops [n,128,128,1] =
 *     crop_mm / 10000, train_cnn_networks_hgru.py:50).  Output buffers are caller-owned.
 *   - Weights are identified by their TensorFlow variable names (e.g. "cnn/contextual_circuit/p_r",
 *     "cnn/fc_1/fc_1_weights"); a leading "cnn/" scope is optional.  The library copies them.
 *   - Calls on one context are serialised by the caller and are asynchronous on `stream`
 *     (a hipStream_t; NULL = default stream).  One context per device.
 *     Asynchronous means ordered: every function with a `stream` argument reads its device inputs after
 *     the work queued on `stream` before the call, and what it writes is complete for work queued on
 *     `stream` after it, also where the call fans out over private streams (the hGRU batch slices, the
 *     layer graph): those wait for an event of `stream` and `stream` waits for theirs.  No such function
 *     waits on the host, except that the first call of a context at a new batch or map shape may
 *     (workspace growth, a new graph plan, stream creation).  A context moves to another stream only
 *     behind an event recorded after its last call; different contexts share no device state.  Host
 *     arguments (cam, com_scale, thresholds, bones, style) are read before the call returns.
 *     (tests/stream_order_cases.py classifies every such function; INTEGRATION.md "Streams".)
 *   - Status: MP_OK (0) or a negative MP_ERR_*; mp_last_error() gives a thread-local message.
 *     No C++ exception crosses the ABI.  Shapes are validated on the host before any launch.
 */
#ifndef MONKEYPOSE_H
#define MONKEYPOSE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mp_ctx mp_ctx;

enum {
  MP_OK = 0,
  MP_ERR_ARG = -1,         /* bad argument / null pointer */
  MP_ERR_STATE = -2,       /* weights missing or not finalized */
  MP_ERR_HIP = -3,         /* HIP runtime error (message has hipGetErrorString) */
  MP_ERR_WEIGHT = -4,      /* unknown weight name or wrong shape */
  MP_ERR_SHAPE = -5,       /* unsupported input shape */
  MP_ERR_UNSUPPORTED = -6  /* option not implemented (e.g. train_mode) */
};

enum {
  MP_MODEL_HGRU_POSE = 1,    /* hgru_pose.model                (hgru_pose.py:6-216)        */
  MP_MODEL_HGRU_CIRCUIT = 2, /* hgru_module.ContextualCircuit  (hgru_module.py:54-959)     */
  MP_MODEL_DENSE = 3,        /* dense_model_struct  (train_dense_networks.py:211-509)      */
  MP_MODEL_HIER = 4,         /* hier_model_struct   (train_hier_networks.py:327-631)       */
  MP_MODEL_ATTN = 5,         /* attn_model_struct   (train_cnn_networks_hgru.py:422-525)   */
  MP_MODEL_GRAPH = 6         /* a recorded layer graph (mp_graph_set): dense_hier_model_struct
                                (train_dense_hier_networks.py:327-2507)                       */
};

enum { MP_MEM_HOST = 0, MP_MEM_DEVICE = 1 };
/* compute precision of the hGRU association-field convolutions (the rest of the path is fp32):
 *   MP_DTYPE_F32        exact fp32 (v_mfma_f32_32x32x2_f32, an fmaf chain)
 *   MP_DTYPE_F32_SPLIT  fp32-accurate "f16x3": each fp32 operand split into two power-of-two
 *                       scaled f16 halves (22 mantissa bits), three f16 MFMAs per product with fp32
 *                       accumulation; errors within a few fp32 ulps of the F32 path, 5.3x fewer
 *                       matrix-core cycles.  Needs map height and width multiples of 32.
 *   MP_DTYPE_F32_FFT    fp32 FFT convolution on a 72x72 grid (exact circular = SAME linear conv
 *                       for maps up to 64x64): fp32 72-point FFTs + a per-frequency complex
 *                       channel GEMM in the f16x3 split (three v_mfma_f32_32x32x16_f16 per complex
 *                       MAC term, fp32 accumulation); ~50x fewer FLOPs than direct at 15x15 taps,
 *                       error ~1e-6 of max|output|.  Needs map height in [1, 64], width 32 or 64.
 *   MP_DTYPE_BF16       the FFT path with bf16 spectra (input and output), bf16 spectral weights and
 *                       bf16 1x1 gate weights: one v_mfma_f32_32x32x16_bf16 product per MAC, fp32
 *                       accumulation, fp32 FFTs and elementwise math; the hGRU maps O / I / Og / P2
 *                       and the drive X stored as bf16; conv_2 / conv_3 and fc_1 run one f16
 *                       product per MAC (hi x hi of the f16x3 split, fp32 accumulation); conv_1,
 *                       the BNs and the fc_1 output stay fp32.  Error ~1e-3 of max|output| on the
 *                       pose (gate 5e-3), a few 1e-3 on the raw circuit state (SURVEY config 4). */
enum { MP_DTYPE_F32 = 0, MP_DTYPE_F32_SPLIT = 1, MP_DTYPE_F32_FFT = 2, MP_DTYPE_BF16 = 3 };
/* Magnitude windows.  Every path that is not plain MP_DTYPE_F32 holds its operands as f16 hi + lo behind a
 * power-of-two scale s: the value times s must stay below f16's 65504 (ceiling), and below 2^-14 / s the
 * halves are rounded on the grid 2^-24 / s, an absolute error of up to 2^-25 / s per value (floor; times
 * sum|w| in an output).  tests/test_gpu_magnitude.py runs each path from 2^-24 to the last octave below
 * 2^15.9 / s on its inputs.
 *   path                                          scale s              ceiling |a| <      floor 2^-25 / s
 *   graph runtime convs / FCs (k_igemm, k_fc)     1                    65504              2^-25
 *   pose conv_2 / conv_3 inputs (k_conv64x3)      16  (BB_ASCALE)      4094               2^-29
 *   64-channel direct hGRU convs, F32_SPLIT       1024  (ACT_SCALE)    63.97              2^-35
 *   hGRU 1x1 gates on the FFT paths (gate_x3)     256  (GATE_VSCALE)   255.9              2^-33
 *   spectra of every FFT conv (k_fft, k_fft4,     1/64  (SPEC_SCALE)   window sum |v|     2^-19 per spectrum
 *     k_circuit_fft)                                                     < 64 * 65504       entry
 *   fc_1's planes from the last row kernel        1                    65504              2^-25
 *   every packed weight tensor                    2^(14 - e),          none: max|w| * s is in [2^13, 2^14);
 *                                                 frexp(max|w|) = (m, e)  a weight below 2^-17 max|w| is off by
 *                                                                      up to 2^-25 / s instead of 2^-22 of itself
 *   MP_DTYPE_BF16 on the six-launch loop          2^-e of max|G|,      p_r's magnitude is taken out, as for a
 *     (MP_FFT4=0, or MP_BF16_MAPS=0): the         G = p_r's spectrum   weight tensor
 *     inverse FFTs' f16 intermediates (k_fft)
 * A weight set times 2^j gives the same packed bits and an output times 2^j, bit for bit.  Outside the window
 * the result is unspecified (non-finite values may appear); nothing checks it at run time. */

/* library version, (major << 16) | minor */
int mp_version(void);

/* thread-local description of the last error on this thread ("" if none) */
const char* mp_last_error(void);

/* create a context on HIP device `device` for model `model_kind` */
int mp_create(int device, int model_kind, mp_ctx** out);
void mp_destroy(mp_ctx* ctx);

/* copy one variable (fp32, row-major, TF shape) into the context; replaces
 * hgru_pose.get_var / tf.get_variable (hgru_pose.py:196-216, hgru_module.py:262-503) */
int mp_set_weight(mp_ctx* ctx, const char* name, const float* data, const int64_t* shape, int ndim,
                  int mem_kind);

/* replicate the weights set on ctxs[root] (mp_set_weight) into every other context of the list --
 * one per device, or several on one device -- device to device, as a binomial tree of peer copies
 * over xGMI: ceil(log2(nctx)) rounds, each round doubling the contexts that hold the weights, every
 * copy of a round in flight together, nothing staged through the host.  Each context then runs
 * its own mp_finalize_weights.  For one process driving several GPUs (SURVEY 8b's proposed
 * weight broadcast); one process per GPU broadcasts the blob with torch.distributed (RCCL) instead
 * (monkey-pose_amd/parallel.py).  Replaces loading data_dict / get_var once per device
 * (hgru_pose.py:196-216). */
int mp_bcast_weights(mp_ctx* const* ctxs, int nctx, int root);

/* fold BN, pack every weight into its kernel's fragment order; must follow the last
 * mp_set_weight and precede any forward call */
int mp_finalize_weights(mp_ctx* ctx, int compute_dtype);

/* pre-allocate the activation workspace for batches up to max_batch (otherwise grown lazily) */
int mp_reserve(mp_ctx* ctx, int64_t max_batch);

/* ContextualCircuit aux 'hidden_init' (hgru_module.py:875-892): the initial output state O0.
 * The initial I is never read by the hgru_pose aux (795-804). */
enum {
  MP_HIDDEN_GIVEN = 0,    /* o0 as passed ('random' with the caller's draw, e.g. for parity)  */
  MP_HIDDEN_ZEROS = 1,    /* O0 = zeros_like(X)                      (888-890); o0 unused */
  MP_HIDDEN_IDENTITY = 2, /* O0 = X, the circuit's drive             (876-878); o0 unused */
  MP_HIDDEN_RANDOM = 3    /* 'random' (879-887): a fresh draw on the device per call, xavier-uniform
                             with limit sqrt(6 / (k + k)); element i of the NHWC O0 is
                             f32((2u - 1) * limit), u = splitmix64(i * 0x9E3779B97F4A7C15 + key) >> 11
                             scaled by 2^-53, key = fnv1a64("h2_init") ^ (s * 0x2545F4914F6CDD1D),
                             s = rng_seed + rng_call (monkey-pose_amd/weights.py synth_hidden(seed=s)) */
};

/* hgru_pose.model.build (hgru_pose.py:47-105), inference:
 *   depth  [n, h, w, 1]   normalised depth crops (h = w = 128 in the reference)
 *   o0     [n, h/2, w/2, 64] initial hGRU output state (hidden_init='random',
 *          hgru_module.py:879-887, made explicit)
 *   out    [n, output_shape] joint coordinates / (cube_z / 2), joint-major (j*3 + {x,y,z}) */
int mp_hgru_pose_fwd(mp_ctx* ctx, const float* depth, int64_t n, int64_t h, int64_t w,
                     const float* o0, float* out, void* stream);

/* the reference model's readable intermediates (hgru_pose.py:50-103: m.conv1, m.pool1, m.conv2,
 * m.conv3, m.hgru, m.fc1, m.relu1); each a caller-owned device buffer, NULL = not wanted.
 * NHWC fp32 like the reference tensors; [n, 1024] for fc1 / relu1.  (The 0.1 layout; 0.2 keeps it.) */
typedef struct {
  float* conv1;  /* [n, h, w, 64]      relu(conv_1)                       (50)      */
  float* pool1;  /* [n, h/2, w/2, 64]  BN(max_pool(conv1))                (51-60)   */
  float* conv2;  /* [n, h/2, w/2, 64]  BN(relu(conv_2))                   (61-70)   */
  float* conv3;  /* [n, h/2, w/2, 64]  BN(relu(conv_3))                   (71-80)   */
  float* hgru;   /* [n, h/2, w/2, 64]  BN(O_T), the fc_1 input            (81-90)   */
  float* fc1;    /* [n, 1024]          fc_1 + bias (pre-activation)       (91)      */
  float* relu1;  /* [n, 1024]          BN(relu(fc1))                      (92-103)  */
} mp_pose_taps;

/* per-call options of mp_hgru_pose_fwd_ex / mp_hgru_circuit_fwd_opts (since 0.2).  struct_size =
 * sizeof(mp_fwd_opts) as the caller was compiled: the library reads that many bytes and no more,
 * and fields added by later versions keep their defaults for older callers.  Zero-initialise. */
typedef struct {
  uint64_t struct_size;
  int32_t hidden_init;        /* MP_HIDDEN_*; o0 may be NULL unless MP_HIDDEN_GIVEN */
  int32_t reserved;
  uint64_t rng_seed;          /* MP_HIDDEN_RANDOM: the draw of seed rng_seed + rng_call */
  uint64_t rng_call;          /*   (the caller's per-call counter: the reference re-draws per run) */
  /* store_states (hgru_module.py:889-915): every timestep's states, [n, T, h/2, w/2, 64] NHWC
   * (the reference's stack transposed to batch-major, 909-912).  states_O[:, t] = O_t after the
   * rho gain, states_I[:, t] = I_t.  (The reference's own stacks swap O and I on alternate steps:
   * full() takes (store_O, store_I) where the loop passes (store_I, store_O), hgru_module.py:825,
   * 897-908; here each stack holds what its name says.)  NULL = not wanted. */
  float* states_O;
  float* states_I;
  const mp_pose_taps* taps;   /* pose model only: the intermediates, or NULL */
} mp_fwd_opts;

/* mp_hgru_pose_fwd with options (opts may be NULL: the mp_hgru_pose_fwd defaults) */
int mp_hgru_pose_fwd_ex(mp_ctx* ctx, const float* depth, int64_t n, int64_t h, int64_t w, const float* o0,
                        float* out, const mp_fwd_opts* opts, void* stream);

/* mp_hgru_pose_fwd that also writes the requested intermediates (taps may be NULL) */
int mp_hgru_pose_fwd_taps(mp_ctx* ctx, const float* depth, int64_t n, int64_t h, int64_t w,
                          const float* o0, float* out, const mp_pose_taps* taps, void* stream);

/* ContextualCircuit(X, timesteps, ...).build() -> O  (hgru_module.py:872-959), hgru_pose aux:
 *   x, o0, o_out  [n, h, w, k] NHWC.  k is a property of the context: mp_finalize_weights takes it
 *   from "contextual_circuit/p_r" [S,S,k,k] (4 <= k <= 256; i_r / o_r [1,1,k,k], the vectors
 *   [1,1,1,k]; anything else is MP_ERR_WEIGHT), mp_info "channels" returns it, and the k passed here
 *   must equal it (MP_ERR_SHAPE) -- there is nothing to express about x beyond that.
 *   k == 64 runs the 64-channel loops below.  Any other k runs the channel-general loop (DESIGN.md
 *   3f: NHWC maps, the graph runtime's implicit-GEMM convs, the epilogue kernels of
 *   k_circuit_nhwc.hip): MP_DTYPE_F32_SPLIT or MP_DTYPE_F32 only -- MP_DTYPE_F32_FFT and
 *   MP_DTYPE_BF16 are MP_ERR_UNSUPPORTED at mp_finalize_weights, their spectral GEMM and map layouts
 *   being 64 wide -- with any h, w >= 1 (n * h * w <= 2^24), the pose aux run as its variant.
 *   With mp_circuit_set_nhwc_conv(MP_CN_CONV_FFT) that loop's association-field conv is an FFT conv
 *   (DESIGN.md 3g): k % 4 == 0, MP_DTYPE_F32_SPLIT, every h, w in [1, 64] (a larger map is
 *   MP_ERR_SHAPE before any launch, o_out untouched), and a conv input must keep
 *   h * w * max|v| / 64 inside f16 range (65504) -- the limit of the 64-channel FFT path.
 *   MP_CN_CONV_FFT_TILED is that conv on maps of any size (every h, w >= 1, n * h * w <= 2^24), cut
 *   into 64 x 64 windows: the range bound is per window, min(h, 64) * min(w, 64) * max|v| / 64.
 *   map size at k == 64, by the dtype the context was finalized with (MP_ERR_SHAPE otherwise, before any launch):
 *     MP_DTYPE_F32_FFT, MP_DTYPE_BF16   any h in [1, 64] (rows past h are zero padding of the 72-point
 *                                       transforms), w == 32 or w == 64
 *     MP_DTYPE_F32                      h % 16 == 0, w % 32 == 0
 *     MP_DTYPE_F32_SPLIT                h % 32 == 0, w % 32 == 0
 *   (tests/test_gpu_circuit_shapes.py runs each rule's accepted and rejected sizes)
 *   timesteps <= the length of the "contextual_circuit/rho" weight */
int mp_hgru_circuit_fwd(mp_ctx* ctx, const float* x, const float* o0, int64_t n, int64_t h,
                        int64_t w, int64_t k, int timesteps, float* o_out, void* stream);

/* mp_hgru_circuit_fwd with the aux 'hidden_init' (MP_HIDDEN_GIVEN / _ZEROS / _IDENTITY; o0 may be
 * NULL unless MP_HIDDEN_GIVEN) and 'store_states' (hgru_module.py:889-915): states_O / states_I,
 * each [n, timesteps, h, w, k] NHWC or NULL, receive every step's O_t (after the rho gain) and I_t */
int mp_hgru_circuit_fwd_ex(mp_ctx* ctx, const float* x, const float* o0, int64_t n, int64_t h, int64_t w,
                           int64_t k, int timesteps, int hidden_init, float* o_out, float* states_O,
                           float* states_I, void* stream);

/* mp_hgru_circuit_fwd with every option of mp_fwd_opts except taps (since 0.2) */
int mp_hgru_circuit_fwd_opts(mp_ctx* ctx, const float* x, const float* o0, int64_t n, int64_t h, int64_t w,
                             int64_t k, int timesteps, float* o_out, const mp_fwd_opts* opts, void* stream);

/* ---- ContextualCircuit variants (the general loop) --------------------------------------------
 * Every aux combination below runs through mp_hgru_circuit_fwd_var: per half-step the
 * association-field conv writes a plain P map and one epilogue kernel applies the variant's rule
 * (hgru_module.py:692-849).  The hgru_pose aux also runs here (for A/B against its fused loop).
 * MP_DTYPE_F32, _F32_SPLIT and _F32_FFT; MP_DTYPE_BF16 with a variant is MP_ERR_UNSUPPORTED. */
enum { MP_NL_TANH = 0, MP_NL_RELU = 1, MP_NL_SELU = 2, MP_NL_LEAKY_RELU = 3, MP_NL_HARD_TANH = 4 };
enum { MP_INT_ALTERNATE = 0, MP_INT_MELY = 1, MP_INT_CONTROL = 2 };
/* mp_circuit_variant.learned: the vectors that are weights ("contextual_circuit/<name>", [1,1,1,64]);
 * one that is not learned is the constant 1 (prepare_tensors, 404-497) and is never asked of the
 * caller.  kappa and omega are weights exactly when multiplicative_excitation is set. */
enum { MP_CV_BETA = 1, MP_CV_NU = 2, MP_CV_ZETA = 4, MP_CV_GAMMA = 8, MP_CV_XI = 16, MP_CV_KAPPA = 32, MP_CV_OMEGA = 64 };
/* struct_size = sizeof(mp_circuit_variant) as the caller was compiled (see mp_fwd_opts).  Zero-initialise. */
typedef struct {
  uint64_t struct_size;
  int32_t gru_gates;                 /* 709-711 */
  int32_t output_gru_gates;          /* 742-743 */
  int32_t multiplicative_excitation; /* 784-793, 808-819 */
  int32_t adaptation;                /* aux 'adapation': O' *= rho[t] (847-849); "contextual_circuit/rho"
                                        is needed only then */
  int32_t rectify;                   /* rectify_weights is False: P1 = min(P1, 0), P2 = max(P2, 0) */
  int32_t recurrent_nl;              /* MP_NL_* */
  int32_t integration;               /* MP_INT_* */
  int32_t learned;                   /* MP_CV_* mask of the learned vectors */
  int32_t lesion;                    /* MP_CV_BETA / _NU / _KAPPA / _OMEGA: the constant 0 (lesion_*) */
  int32_t reserved;
  /* MP_HIDDEN_RANDOM: O0 is the draw of seed rng_seed + rng_call, I0 that of rng_seed_i + rng_call
   * (the reference draws the two states independently, 880-887) */
  uint64_t rng_seed;
  uint64_t rng_seed_i;
  uint64_t rng_call;
} mp_circuit_variant;

/* fixes the variant an MP_MODEL_HGRU_CIRCUIT context will run; before mp_finalize_weights, which
 * then asks only for the weights this variant reads and prepares the general loop's form of p_r
 * (on MP_DTYPE_F32_FFT the six-launch spectral weights).  Such a context serves
 * mp_hgru_circuit_fwd_var only; one without serves the fused entries only (MP_ERR_STATE otherwise). */
int mp_circuit_set_variant(mp_ctx* ctx, const mp_circuit_variant* variant);

/* enable != 0: a 64-channel MP_MODEL_HGRU_CIRCUIT context runs the channel-general loop too (for a
 * cross-check of the two loops, and for map sizes the 64-channel tilings reject); before
 * mp_finalize_weights, with or without a variant.  Off by default: k == 64 then takes the 64-channel
 * loops exactly as before.  Contexts of any other k run that loop whatever this says. */
int mp_circuit_set_nhwc_loop(mp_ctx* ctx, int enable);

/* the algorithm of the channel-general loop's association-field conv (the compute dtype keeps naming the
 * arithmetic): MP_CN_CONV_DIRECT, the default, is the implicit-GEMM conv; MP_CN_CONV_FFT a forward FFT,
 * an f16x3 spectral product per frequency and an inverse FFT on a 72 x 72 grid (k_circuit_fft.hip,
 * DESIGN.md 3g); MP_CN_CONV_FFT_TILED (since 0.3, additive) the same conv on maps of any size by
 * overlap-save: the map is cut into windows of at most 64 x 64, each goes through the
 * 72 x 72 transforms, and the outputs whose whole filter support lay inside the window are kept.  On a
 * map with h, w <= 64 it is one window and equals MP_CN_CONV_FFT bit for bit.  Before
 * mp_finalize_weights, with or without a variant; MP_ERR_STATE on a finalized
 * context, MP_ERR_ARG for another value.  With either FFT conv set, mp_finalize_weights is
 * MP_ERR_UNSUPPORTED, before any launch, for a context that is not on the channel-general loop (k == 64
 * without mp_circuit_set_nhwc_loop: 64 channels have MP_DTYPE_F32_FFT), for k % 4 != 0, and for any
 * dtype but MP_DTYPE_F32_SPLIT; under MP_CN_CONV_FFT a call with h > 64 or w > 64 is MP_ERR_SHAPE.
 * Spectra are kept for at most mp_info "nhwc_fft_chunk" windows (images, up to 64 x 64) at a time (S + Y
 * within 1 GiB): a larger batch is walked in chunks, which may begin and end inside an image and change
 * no bit of any output.  Range: a conv input (O, I or their gated forms) must keep
 * min(h, 64) * min(w, 64) * max|v| / 64 inside f16 range: a window's sum bounds its spectrum, so a
 * tanh-bounded state uses 64 of the range at any map size. */
#define MP_CN_CONV_DIRECT 0
#define MP_CN_CONV_FFT 1
#define MP_CN_CONV_FFT_TILED 2
int mp_circuit_set_nhwc_conv(mp_ctx* ctx, int conv);

/* MP_CN_CONV_FFT_TILED's tile plan along one axis of length L (L >= 1) under a filter of size ssf (3, 5 or
 * 15; R = ssf / 2), on the host (no GPU; the arithmetic the kernels compile, circuit_fft.hpp).  Returns
 * the tile count and fills, per tile i: origin[i], the map position of the window's local index 0
 * (the window is [origin, origin + 64), zeros outside the map); out0[i], the local index of its first
 * output; count[i], the outputs it owns (map positions origin + out0 .. origin + out0 + count - 1).
 * L <= 64: one tile {0, 0, L}.  L > 64: step T = 64 - 2 R, ceil(L / T) tiles {i T - R, R, min(T, L - i T)}.
 * MP_ERR_ARG for another ssf, L < 1, a null array, or cap (the arrays' length) below the tile count. */
int mp_cn_fft_tiles_host(int L, int ssf, int cap, int32_t* origin, int32_t* out0, int32_t* count);

/* ContextualCircuit(X, timesteps, ..., aux).build() for the context's variant.  x, o0, i0, o_out,
 * i_out [n, h, w, 64] NHWC fp32; states_O / states_I [n, timesteps, h, w, 64] or NULL (every step's
 * O_t after the rho gain / I_t).  hidden_init as in mp_fwd_opts, for both states (875-892): o0 and
 * i0 are read with MP_HIDDEN_GIVEN only, and i0 only by a variant that reads the previous I
 * (gru_gates unset with alternate / mely integration, or mely at all); i_out may be NULL.  variant:
 * the flags the context was finalized with (MP_ERR_STATE if they differ) and this call's rng fields.
 * Map sizes: the per-dtype rules of mp_hgru_circuit_fwd (MP_DTYPE_F32_FFT: any h in [1, 64], w 32 or
 * 64; MP_DTYPE_F32: h % 16 == 0, w % 32 == 0; MP_DTYPE_F32_SPLIT: h % 32 == 0, w % 32 == 0), and
 * n * h * w <= 2^24.  On the channel-general loop (k != 64, or mp_circuit_set_nhwc_loop) every 64
 * above is the context's k and any h, w >= 1 is taken; with MP_CN_CONV_FFT (mp_circuit_set_nhwc_conv)
 * h, w in [1, 64], and every conv input keeps h * w * max|v| / 64 inside f16 range; with
 * MP_CN_CONV_FFT_TILED any h, w >= 1 again, the bound being min(h, 64) * min(w, 64) * max|v| / 64. */
int mp_hgru_circuit_fwd_var(mp_ctx* ctx, const float* x, const float* o0, const float* i0, int64_t n, int64_t h,
                            int64_t w, int64_t k, int timesteps, int hidden_init, const mp_circuit_variant* variant,
                            float* o_out, float* i_out, float* states_O, float* states_I, void* stream);

/* the variant's per-channel rule on host arrays (no GPU; the code the epilogue kernels compile):
 * half 0: out = I' from P1, x, o, i (the previous I), gate = O . i_r + i_b
 * half 1: out = O' from P2 (in p), i = I', o, gate = I' . o_r + o_b; x is not read
 * p is the conv result before lateral_bias.  All arrays [npix][64]; consts [8][64] in the order
 * lateral_bias, beta, nu, xi, gamma, kappa, omega, zeta, holding the values the variant resolves to. */
int mp_circuit_var_rule_host(const mp_circuit_variant* variant, int half, int64_t npix, const float* p,
                             const float* x, const float* o, const float* i, const float* gate,
                             const float* consts, float rho, float* out);

/* dense_model_struct.build(depth, output_shape) -> .output  (train_dense_networks.py:223-408):
 *   depth [n, h, w, 1] (h, w multiples of 32 in the reference's 128x128), out [n, output_shape] */
int mp_dense_fwd(mp_ctx* ctx, const float* depth, int64_t n, int64_t h, int64_t w, float* out,
                 void* stream);

/* hier_model_struct.build(depth, output_shape, P_shape, R_shape, M_shape, I_shape, T_shape)
 * (train_hier_networks.py:338-530): outs[0] = .output [n, output_shape], outs[1..5] =
 * .p_output .r_output .m_output .i_output .t_output [n, *_shape] (sizes = the fc_3 widths) */
int mp_hier_fwd(mp_ctx* ctx, const float* depth, int64_t n, int64_t h, int64_t w, float* const* outs,
                void* stream);

/* attn_model_struct.build(depth, output_shape) -> .out_put  (train_cnn_networks_hgru.py:436-525),
 * the attention (centre-of-mass) regressor, inference (BN from moving statistics, no dropout):
 *   frames [n, h, w, 1] normalised full depth frames (image / image_max_depth,
 *          train_cnn_networks_hgru.py:116; 424 x 512 in the reference), resized to 128 x 128
 *   out    [n, output_shape] (u, v, d) / (image_orig_size[0], image_orig_size[1], image_max_depth) */
int mp_attn_fwd(mp_ctx* ctx, const float* frames, int64_t n, int64_t h, int64_t w, float* out, void* stream);

/* the attention net's readable intermediates (train_cnn_networks_hgru.py:439-512); each a caller-owned
 * device buffer, NULL = not wanted.  NHWC fp32.  aconv_1 is fused with its pool, so there is no conv1. */
typedef struct {
  float* resized;  /* [n, 128, 128, 1]    the resized input (the frames themselves at 128 x 128)  (439)     */
  float* conv2;    /* [n, 64, 64, 128]    relu(aconv_2 + b), before the pool                      (452)     */
  float* conv3;    /* [n, 32, 32, 256]    relu(aconv_3 + b)                                       (464)     */
  float* conv4;    /* [n, 16, 16, 512]    relu(aconv_4 + b)                                       (476)     */
  float* conv5;    /* [n, 8, 8, 1024]     relu(aconv_5 + b)                                       (488)     */
  float* pool1;    /* [n, 64, 64, 64]     BN(max_pool(relu(aconv_1 + b)))                         (440-450) */
  float* pool2;    /* [n, 32, 32, 128]    BN(max_pool(conv2))                                     (453-462) */
  float* pool3;    /* [n, 16, 16, 256]    BN(max_pool(conv3))                                     (465-474) */
  float* pool4;    /* [n, 8, 8, 512]      BN(max_pool(conv4))                                     (477-486) */
  float* pool5;    /* [n, 4, 4, 1024]     BN(max_pool(conv5)), the afc_1 input                    (489-498) */
  float* relu1;    /* [n, 1024]           BN(relu(afc_1))                                         (500-512) */
} mp_attn_taps;

/* mp_attn_fwd that also writes the requested intermediates (taps may be NULL: exactly mp_attn_fwd's
 * launches).  Each tap is copied on `stream` right after its producer, before its buffer is reused.
 * After a forward, mp_info "attn_path:<aconv_2 .. aconv_5>" reports the kernel each conv took. */
int mp_attn_fwd_taps(mp_ctx* ctx, const float* frames, int64_t n, int64_t h, int64_t w, float* out,
                     const mp_attn_taps* taps, void* stream);

/* tf.image.resize_images(x, [ho, wo]) with the TF1 defaults (BILINEAR, align_corners=False,
 * legacy source coordinates in = out * in_size / out_size), bit-identical to TF's float32 kernel:
 *   x [n, h, w, c] -> out [n, ho, wo, c], device pointers */
int mp_resize_bilinear(const float* x, int64_t n, int64_t h, int64_t w, int64_t c, int64_t ho, int64_t wo,
                       float* out, void* stream);

/* ---- host-side 3D CoM crop (no GPU; the pre-step of every regressor) -------------------------
 * MonkeyDetector(fx, fy, ux, uy, cube, d1, d2) (monkeydetector.py:31-63, tf_monkeydetector.py),
 * constructed in the reference as (365.456, 365.456, 256, 212, [800,800,1200], 200, 10000)
 * (train_cnn_networks_hgru.py:77). */
typedef struct {
  double fx, fy, ux, uy; /* focal lengths, principal point (pixels) */
  double cube[3];        /* crop volume (x, y, z) in mm */
  double min_depth;      /* d1: near plane, mm */
  double max_depth;      /* d2: far plane, mm (also the canvas fill of the crop) */
} mp_camera;

/* depth frame element type: float32 mm (the hGRU caller: image * 10000, train_cnn_networks_hgru.py:47)
 * or uint16 mm (Kinect PNG, sample_pipeline.py:21); numpy semantics differ and are kept: the CoM
 * depth sum is float32-pairwise vs exact, the near-plane clamp rounds vs truncates */
enum { MP_DEPTH_F32 = 0, MP_DEPTH_U16 = 1 };

/* MonkeyDetector.calculateCoM (monkeydetector.py:66-83): com = (mean col, mean row, sum(d)/count)
 * over pixels with min_depth <= d <= max_depth of a float32 [h][w] frame in mm; (0,0,0) if none */
int mp_center_of_mass(const mp_camera* cam, const void* depth, int depth_dtype, int64_t h, int64_t w,
                      double com[3]);

/* MonkeyDetector.cropArea3D(dpt, com, dsize=(dsize, dsize)) (monkeydetector.py:261-334):
 *   com     (u, v, d) in pixels / mm, or NULL to use mp_center_of_mass
 *   out     [dsize][dsize] float32 crop in mm, canvas filled with max_depth
 *   M       3x3 row-major crop transform (off * scale * trans), com_out: the CoM used
 *   info    optional {xstart, xend, ystart, yend, sz_w, sz_h, off_x, off_y} (integers of the crop) */
int mp_crop3d(const mp_camera* cam, const void* depth, int depth_dtype, int64_t h, int64_t w, const double* com,
              int64_t dsize, float* out, double M[9], double com_out[3], int32_t info[8]);

/* mp_crop3d with cropArea3D's other options (since 0.2):
 *   flags  MP_CROP_DOCOM: docom=True, the second refinement (monkeydetector.py:287-300) -- the CoM of
 *          the first crop (+ xstart / ystart), falling back to the crop's centre depth and then to
 *          300 mm when that CoM is (0,0,0), and a second crop around it; com_out is the refined CoM */
enum { MP_CROP_DOCOM = 1 };
int mp_crop3d_ex(const mp_camera* cam, const void* depth, int depth_dtype, int64_t h, int64_t w, const double* com,
                 int flags, int64_t dsize, float* out, double M[9], double com_out[3], int32_t info[8]);

/* prepare_data_test (train_cnn_networks_hgru.py:61-74) for n frames [n][h][w]: patches
 * [n][dsize][dsize][1] = crop / max_depth (the model input), Ms [n][9], coms_out [n][3];
 * coms [n][3] or NULL; frames are processed by up to nthreads host threads */
int mp_crop3d_batch(const mp_camera* cam, const void* frames, int depth_dtype, int64_t n, int64_t h, int64_t w,
                    const double* coms, int64_t dsize, float* patches, double* Ms, double* coms_out,
                    int nthreads);

/* prepare_data_test on the device (train_cnn_networks_hgru.py:61-74) with tr_res = the attention
 * output, for a batch of n frames in one launch (asynchronous; every pointer is device memory
 * except cam and com_scale, which are read on the host at the call):
 *   frames    [n][h][w] float32 as fed to the attention net; the crop sees frames * frame_scale
 *             (image_np * image_max_depth, line 67: frame_scale = 10000)
 *   com_norm  [n][3] float32 attention output; com = com_norm * com_scale in float64
 *             (com_scale: host double[3] = {image_orig_size[0], image_orig_size[1], image_max_depth},
 *             line 69)
 *   patches   [n][dsize][dsize][1] = cropArea3D(frame, com) / cam.max_depth
 *   Ms [n][9], coms_out [n][3] float64; status [n] int32: 0 ok, else the frame's crop failed
 *             (1 CoM depth zero / not finite, 2 empty crop, 3 degenerate bounds, 4 empty resize;
 *             that patch is all ones) -- the host mp_crop3d raises MP_ERR_ARG in those cases.
 * Integers (bounds, sizes, offsets, nearest-neighbour indices) are bit-exact with mp_crop3d. */
int mp_crop3d_dev(const mp_camera* cam, const float* frames, int64_t n, int64_t h, int64_t w, float frame_scale,
                  const float* com_norm, const double* com_scale, int64_t dsize, float* patches, double* Ms,
                  double* coms_out, int32_t* status, void* stream);

/* mp_crop3d_dev with flags (since 0.2): MP_CROP_DOCOM runs cropArea3D's docom refinement per frame on
 * the device (one block per frame: calculateCoM of the first crop with numpy's float32 pairwise
 * sum order, the allclose / isclose fallbacks, the second crop); coms_out then holds the refined
 * CoMs.  Bit-exact with mp_crop3d_ex(..., MP_CROP_DOCOM, ...). */
int mp_crop3d_dev_ex(const mp_camera* cam, const float* frames, int64_t n, int64_t h, int64_t w, float frame_scale,
                     const float* com_norm, const double* com_scale, int flags, int64_t dsize, float* patches,
                     double* Ms, double* coms_out, int32_t* status, void* stream);

/* ---- the detector path on the device (added after 0.3; mp_version() is unchanged) ------------
 * SURVEY config 5 with MonkeyDetector's own CoM: calculateCoM -> cropArea3D -> pose ->
 * getAbsoluteCoordinates for a batch without a host step.  All three calls are asynchronous on
 * `stream`, allocate nothing and synchronise nothing; every pointer except cam is device memory.
 *
 * mp_center_of_mass_dev: calculateCoM (monkeydetector.py:66-83) of n float32 frames [n][h][w]; the
 * detector sees frames * frame_scale (one float32 multiply: 1 for frames in mm, 10000 for frames
 * normalised by image_max_depth).  coms [n][3] float64 = mp_center_of_mass(MP_DEPTH_F32) of each
 * frame bit for bit: integer mask sums, and the depth sum in numpy 1.x's float32 pairwise order.
 * work: scratch of at least mp_center_of_mass_dev_work(n, h, w) bytes (8-byte aligned), reusable
 * by the next call on the same stream.  n <= 65535, h * w <= 2^30. */
size_t mp_center_of_mass_dev_work(int64_t n, int64_t h, int64_t w);
int mp_center_of_mass_dev(const mp_camera* cam, const float* frames, int64_t n, int64_t h, int64_t w,
                          float frame_scale, double* coms, void* work, size_t work_bytes, void* stream);

/* mp_crop3d_dev_ex around given CoMs: coms [n][3] float64 in device memory (e.g. the output of
 * mp_center_of_mass_dev) are used as they are, in place of com_norm * com_scale.  flags takes
 * MP_CROP_DOCOM.  patches, Ms, coms_out and status as mp_crop3d_dev_ex (a CoM of (0,0,0) gives
 * status 1 and an all-ones patch); coms_out must not alias coms. */
int mp_crop3d_dev_coms(const mp_camera* cam, const float* frames, int64_t n, int64_t h, int64_t w, float frame_scale,
                       const double* coms, int flags, int64_t dsize, float* patches, double* Ms, double* coms_out,
                       int32_t* status, void* stream);

/* The two calls above by frame element type (added after 0.3; mp_version() is unchanged).
 * MP_DEPTH_F32 forwards to them.  MP_DEPTH_U16: frames are uint16 millimetres [n][h][w] in device
 * memory (2-byte aligned; a camera's frames uploaded as they are, half the bytes), computed with
 * the uint16 semantics of the host functions and bit-identical to mp_center_of_mass(MP_DEPTH_U16) /
 * mp_crop3d_batch / mp_crop3d_ex(MP_DEPTH_U16): thresholds compared in float64, an exact integer
 * depth sum, a truncating near-plane clamp, and a docom refinement whose sums are all integers.
 * uint16 frames have no normalised form: frame_scale must be 1.0f.  That, a frames pointer at an
 * odd address and an unknown depth_dtype are MP_ERR_ARG (the work-size query returns 0); shape
 * limits, work-buffer rules, outputs and status codes are those of the float32 calls.  Every
 * argument is validated before the first GPU call. */
size_t mp_center_of_mass_dev_work_dt(int depth_dtype, int64_t n, int64_t h, int64_t w);
int mp_center_of_mass_dev_dt(const mp_camera* cam, const void* frames, int depth_dtype, int64_t n, int64_t h,
                             int64_t w, float frame_scale, double* coms, void* work, size_t work_bytes,
                             void* stream);
int mp_crop3d_dev_coms_dt(const mp_camera* cam, const void* frames, int depth_dtype, int64_t n, int64_t h, int64_t w,
                          float frame_scale, const double* coms, int flags, int64_t dsize, float* patches,
                          double* Ms, double* coms_out, int32_t* status, void* stream);

/* Recorded camera frames -> the attention net's input (added after 0.3; mp_version() is unchanged):
 * the preprocessing of eval_model_on_real_data (train_cnn_networks_hgru.py:388-392, 359) for n frames
 * in one asynchronous pass on `stream`; raw and out are device memory, nothing is allocated or
 * synchronised.
 *   raw         uint16 (MP_DEPTH_U16, the camera's millimetres) or float32 (MP_DEPTH_F32) frames,
 *               aligned to their element size (a uint16 frame may start at an address that is no
 *               multiple of 4)
 *   transposed  1: raw is [n][w][h], as the recordings are stored (np.transpose of each, line 388);
 *               0: raw is [n][h][w]
 *   gate        1: g = (v < lo || v > hi) ? fill : v in the frame's own dtype -- the reference's two
 *               masked assignments (390-391) for every fill.  uint16: integer compares; lo, hi and
 *               fill must be integers in [0, 65535] (MP_ERR_ARG).  float32: compared against
 *               (float)lo and (float)hi and filled with (float)fill; NaN stays NaN, +-inf is gated.
 *               0: g = v, and lo, hi, fill are ignored
 *   out         [n][h][w] float32 = (float)g / (float)max_depth, one correctly rounded IEEE float32
 *               division (not a multiply by a reciprocal): numpy's bits.  4-byte aligned; 16-byte
 *               alignment lets every row with w % 4 == 0 be stored as float4
 * The transposed form runs 64 x 64 tiles through LDS (reads along h, stores along w), for any h, w.
 * MP_ERR_ARG: a null or misaligned pointer, an unknown dtype, transposed or gate not 0 / 1,
 * (float)max_depth zero or NaN; MP_ERR_SHAPE: n, h or w <= 0, n > 65535, h * w > 2^30.  Every
 * argument is validated before the launch. */
int mp_real_frames_dev(const void* raw, int depth_dtype, int64_t n, int64_t h, int64_t w, int transposed, int gate,
                       double lo, double hi, double fill, double max_depth, float* out, void* stream);

/* getAbsoluteCoordinates (monkeydetector.py:356-360) of a pose output: pose [n][joints * 3] float32
 * normalised by cube_z / 2 (the regressors' output), coms [n][3] float64 (u, v, d).  Per joint:
 * xyz = pose * f32(cube_z / 2) + f32(uvdtoxyz(com)) in mm, uvd = xyztouvd(xyz) (a joint with z == 0
 * maps to (ux, uy, -z)); both [n][joints][3] float32, the bits of the host numpy code. */
int mp_abs_joints_dev(const mp_camera* cam, const float* pose, int64_t n, int64_t joints, const double* coms,
                      float* xyz, float* uvd, void* stream);

/* ---- the validation pass on the device (added after 0.3; mp_version() is unchanged) -----------
 * Labels, joint errors and metrics of a labelled batch (train_cnn_networks_hgru.py:160-173, 229-237;
 * pose_evaluation.py) without a host step.  Every call that takes `stream` is asynchronous on it,
 * allocates nothing and synchronises nothing; every pointer except cam and thresholds is device
 * memory.  joints <= 128 (numpy's pairwise sum is one leaf up to there), n <= 65535.
 *
 * mp_rel_labels_dev: the label half of prepare_data (train_cnn_networks_hgru.py:52-56): labels
 * [n][joints][3] float32 absolute xyz in mm, coms [n][3] float64 (the crop's coms_out) ->
 * rel [n][joints * 3] float32 = clip((label - f32(uvdtoxyz(com))) / f32(cube_z / 2), -1, 1); the
 * subtraction and division are float32, a NaN label stays NaN (numpy.clip).  f32(uvdtoxyz(com)) has
 * the bits mp_abs_joints_dev uses. */
int mp_rel_labels_dev(const mp_camera* cam, const float* labels, int64_t n, int64_t joints, const double* coms,
                      float* rel, void* stream);

/* tfMonkeyDetector.calculateCoMfrom3DJoints (tf_monkeydetector.py:66-71) and the driver's
 * normalisation (train_cnn_networks_hgru.py:166): labels [n][joints][3] float32 -> com [n][3]
 * float32.  The mean over the joints is a sequential float32 sum in joint order divided by
 * f32(joints); then xyztouvd in float32 with no z == 0 guard (inf / NaN propagate):
 * u = f32(ux) - (x / z) * f32(fx), v = f32(uy) + (y / z) * f32(fy), d = -z; then u, v, d are divided
 * by f32(scale_u), f32(scale_v), f32(scale_d) (pass 1, 1, 1 for the plain uvd). */
int mp_com_from_joints_dev(const mp_camera* cam, const float* labels, int64_t n, int64_t joints, double scale_u,
                           double scale_v, double scale_d, float* com, void* stream);

/* A streaming evaluator: a state in device memory that mp_eval_accumulate_dev updates per batch.
 *   state   mp_eval_state_bytes(joints, T) bytes, 8-byte aligned; T <= 1024 thresholds (0 if
 *           joints or T is out of range)
 *   mp_eval_reset_dev  zeroes the state and stores thresholds [T] float32, a HOST array read at
 *           the call
 *   mp_eval_accumulate_dev  labels, results [n][joints][3] float32, both multiplied by the float32
 *           `scale` first (1 for mm, f32(cube_z / 2) for normalised values).  Per joint
 *           d = sqrtf(((dx * dx) + (dy * dy)) + dz * dz); per frame, NaN-aware as numpy.nanmean /
 *           nanmax over the joints in numpy's float32 order: frame_mean, frame_max (NaN when every
 *           joint is NaN).  The state gains: frames, frames whose mean is not NaN, the float64 sum
 *           of frame_mean, the largest distance, per joint the float64 sum of distances and the
 *           non-NaN count, and per threshold the frames with frame_max <= t and with
 *           frame_mean <= t.  No floating-point atomics: the float64 sums run in frame order, so a
 *           sequence of calls leaves the same bytes whenever it is repeated, and the same sums
 *           however the frames are cut into batches.
 *           work: scratch of at least mp_eval_work_bytes(n, joints) bytes, 8-byte aligned.
 *           dist [n][joints], frame_mean [n], frame_max [n]: optional float32 outputs (NULL allowed).
 *           joints and T must be those of the reset; a state that was reset for others is left as
 *           it is and its summary is all NaN.
 *   mp_eval_summary_dev  out [mp_eval_summary_len(joints, T)] float64: frames, valid_frames,
 *           mean_error, max_error, joint_mean[joints], within_max[T], within_mean[T]; the two
 *           within arrays in percent of all frames (count / frames * 100).  With joints = 1 the
 *           mean_error is calc_com_error (train_cnn_networks_hgru.py:36-39). */
size_t mp_eval_state_bytes(int64_t joints, int64_t T);
size_t mp_eval_work_bytes(int64_t n, int64_t joints);
int mp_eval_reset_dev(void* state, int64_t joints, int64_t T, const float* thresholds, void* stream);
int mp_eval_accumulate_dev(void* state, const float* labels, const float* results, int64_t n, int64_t joints,
                           int64_t T, float scale, void* work, size_t work_bytes, float* dist, float* frame_mean,
                           float* frame_max, void* stream);
int64_t mp_eval_summary_len(int64_t joints, int64_t T);
int mp_eval_summary_dev(const void* state, int64_t joints, int64_t T, double* out, void* stream);

/* read a model property: "output_shape", "timesteps", "ssf", "finalized", "workspace_bytes",
 * "weight_bytes", "fft_loop" (hGRU contexts: 4 = the four-step FFT loop, 6 = the six-launch FFT
 * loop, 0 = a direct-convolution dtype, no FFT path), "channels" (the circuit's channel count k, from
 * p_r at mp_finalize_weights), "nhwc_loop" (1: finalized for the channel-general loop),
 * "nhwc_conv" (that loop's conv: 1 the FFT conv MP_CN_CONV_FFT, 2 MP_CN_CONV_FFT_TILED, 0 the direct conv),
 * "nhwc_fft_chunk" (windows -- images, up to 64 x 64 -- per chunk of the FFT conv at the context's k); graph contexts also "graph_kernels" (kernel launches per forward),
 * "graph_streams" (streams the schedule uses), "graph_buffers" (activation buffers after concat placement), "graph_fused_pools" (2x2 max pools
 * computed inside their conv's kernel: MP_GRAPH_FUSE / MP_GRAPH_FUSE_POOL), "graph_fused_1x1" (1x1
 * convs computed by a sibling's kernel) and "graph_path:<conv layer scope>" (the kernel the planned
 * conv launches, an MP_PATH_* word, below) -- as planned by the last forward; attention contexts
 * "attn_path:<aconv_2 .. aconv_5>" (the same word for the conv of that scope, from its launch arguments
 * at the last forward's batch; aconv_1 is the fused MP_PATH_CONV1_POOL_BN kernel) */
int mp_info(mp_ctx* ctx, const char* key, int64_t* value);

/* "graph_path:<scope>": which kernel family the planned conv of that scope launches, as decided by
 * the dispatch itself (the launcher switches on the same value).  One word:
 *   bits  0..7   family (MP_PATH_*)
 *   bit   8      the conv's 2x2 max pool is fused into this kernel
 *   bits 12..19  split-K count (1 = no split)
 *   bits 20..23  halo family: pixel rows of waves, WR (MP_HALO_*)
 *   bits 24..31  halo family: input channels per staged chunk, CH (16 or 32)
 *   bits 32..35  halo family: filter size KS (3 or 5)
 *   bits 36..39  pw / pwn: 32-channel input chunks, nch (1..6)
 *   bits 40..43  pwn: 32-channel output blocks one block owns, nb (2..6); f32 / x3 im2col: NB (1, 2, 4)
 * MP_PATH_SIBLING carries no other field: ask the sibling that leads the run for the kernel. */
enum {
  MP_PATH_F32_IM2COL = 1,      /* igemm_conv_kernel<NB>: exact fp32 (MP_DTYPE_F32, or K < 4)        */
  MP_PATH_X3 = 2,              /* igemm_x3_kernel<NB>: f16-split im2col, Cout <= 64                 */
  MP_PATH_X3W = 3,             /* igemm_x3w_kernel: wide im2col, Cout > 64                          */
  MP_PATH_X3W_SPLITK = 4,      /* igemm_x3w_kernel over K slices + igemm_split_reduce_kernel        */
  MP_PATH_PM = 5,              /* igemm_x3w_pm_kernel: position-major, padding taps skipped         */
  MP_PATH_PM_SPLITK = 6,       /* igemm_x3w_pm_kernel over Cin ranges + igemm_pm_reduce_kernel      */
  MP_PATH_HALO = 7,            /* igemm_x3h_kernel<KS, ., WR, CH>: halo tiles staged in LDS         */
  MP_PATH_PW = 8,              /* igemm_x3pw_kernel<., nch>: 1x1, K <= 192                          */
  MP_PATH_PWN = 9,             /* igemm_x3pwn_kernel<., nch, nb>: 1x1, one block per pixel tile     */
  MP_PATH_CONV1_POOL_BN = 10,  /* 1 -> 64 channels 3x3 + relu + 2x2 max pool, dense output          */
  MP_PATH_CONV1_POOL_ANY = 11, /* 1 -> C channels 3x3 + relu + 2x2 max pool into any output view    */
  MP_PATH_SIBLING = 12         /* a 1x1 conv computed by a sibling's kernel (concatenated weights)  */
};
enum {
  MP_HALO_TALL = 1,            /* Cout > 64 (default; MP_IGEMM_HALO_TALL=0 gives MP_HALO_WIDE)      */
  MP_HALO_WIDE = 2,            /* Cout > 64 under MP_IGEMM_HALO_TALL=0 only                         */
  MP_HALO_NARROW = 4,          /* Cout <= 64                                                        */
  MP_HALO_NARROW1 = 8          /* Cout <= 32, no fused pool                                         */
};
#define MP_PATH_FAMILY(v) ((int)((v) & 0xff))
#define MP_PATH_POOL(v) ((int)(((v) >> 8) & 1))
#define MP_PATH_SPLITS(v) ((int)(((v) >> 12) & 0xff))
#define MP_PATH_WR(v) ((int)(((v) >> 20) & 0xf))
#define MP_PATH_CH(v) ((int)(((v) >> 24) & 0xff))
#define MP_PATH_KS(v) ((int)(((v) >> 32) & 0xf))
#define MP_PATH_NCH(v) ((int)(((v) >> 36) & 0xf))
#define MP_PATH_NB(v) ((int)(((v) >> 40) & 0xf))

/* per-kernel device timing with HIP events recorded on the launch stream around every launch of
 * kernel class `name` ("conv15_a", "conv15_b", "fc1", "backbone"); enable, run, then read the
 * summed elapsed milliseconds and launch count (reading synchronises those events) */
int mp_profile_enable(mp_ctx* ctx, int enable);
int mp_profile_read(mp_ctx* ctx, const char* name, double* total_ms, int64_t* launches);

/* ---- layer-graph runtime (MP_MODEL_GRAPH) ---------------------------------------------------
 * The reference's regressors are TF1 graph builders: build() chains conv_layer / max_pool /
 * tf.concat / fc_layer calls.  A facade records the same calls as ops (tensor ids in SSA order:
 * id 0 = the [n, h, w, in_channels] input, every op defines `out`); the library then plans and runs
 * the graph natively:
 *   - tf.concat is free: a weighted union-find places every concatenated tensor as a channel
 *     range of one wide NHWC buffer per concat group, which its producers write in place;
 *   - relu / identity fold into their producer (conv_layer already applies relu; a relu after
 *     fc_layer becomes the FC epilogue);
 *   - kernels run as a dependency DAG over up to MP_GRAPH_STREAMS (env, default 8) HIP streams.
 * Replaces the graph-builder half of dense_hier_model_struct.build (train_dense_hier_networks.py:
 * 338-2382; helpers conv_layer 2431-2446, max_pool 2426-2429, avg_pool 2416-2419, max_pool_4
 * 2421-2424, fc_layer 2448-2455). */
enum {
  MP_OP_CONV = 1,     /* relu(conv2d(src, name/name_filters, stride, SAME) + name/name_biases) */
  MP_OP_MAXPOOL = 2,  /* ksize x ksize / ksize max pool, SAME (ksize 2 or 4)                     */
  MP_OP_AVGPOOL = 3,  /* 2x2 / 2 average pool, SAME (in-image count)                             */
  MP_OP_CONCAT = 4,   /* tf.concat(src[0..n_src), axis=-1)                                       */
  MP_OP_FC = 5,       /* reshape(src, [-1, K]) @ name/name_weights + name/name_biases             */
  MP_OP_RELU = 6,     /* tf.nn.relu                                                              */
  MP_OP_IDENTITY = 7  /* tf.identity                                                             */
};
#define MP_GRAPH_MAX_SRC 8
typedef struct {
  int32_t kind;                    /* MP_OP_* */
  int32_t out;                     /* tensor id defined by this op (> every id it reads) */
  int32_t n_src;
  int32_t src[MP_GRAPH_MAX_SRC];
  int32_t ksize, stride, cout;     /* conv: filter size, stride, out channels; pools: ksize */
  const char* name;                /* conv / fc: the layer's variable scope ("dense_1_conv_1_scale_1") */
} mp_graph_op;

/* install the graph of an MP_MODEL_GRAPH context (before mp_finalize_weights, which packs every
 * conv / fc layer it names); outputs: the tensor ids mp_graph_fwd writes, in order */
int mp_graph_set(mp_ctx* ctx, const mp_graph_op* ops, int n_ops, int in_channels, const int32_t* outputs,
                 int n_outputs);

/* run the graph on x [n, h, w, in_channels]; outs[i] = caller-owned device buffer holding output
 * tensor i densely ([n, cout] for an fc output, [n, H, W, C] otherwise) */
int mp_graph_fwd(mp_ctx* ctx, const float* x, int64_t n, int64_t h, int64_t w, float* const* outs, void* stream);

/* ---- joint overlays on the device (added after 0.3; mp_version() is unchanged) ---------------
 * The picture the reference's inference entries end with (plt.imshow(frame); plt.scatter(uvd);
 * save_result_image's labels / results / skeleton lines): n depth frames through a colour map with
 * joint markers and bones drawn on them, in one asynchronous pass on `stream`.  Nothing is allocated
 * or synchronised; every argument is validated before the launch.  The rule is
 * csrc/overlay_geom.hpp; in short:
 *   frames      [n][h][w] float32 (MP_DEPTH_F32) or uint16 (MP_DEPTH_U16), device memory aligned to
 *               the element size; n <= 65535, h, w <= 4096
 *   lo, hi      depth colour: x = (d - lo) / (hi - lo) in float32 (one IEEE division), index 0 if
 *               !(x >= 0) (also NaN), 255 if x >= 1, else (int)(x * 255 + 0.5); finite, hi != lo
 *               (lo > hi inverts the map)
 *   lut         [256][3] uint8 RGB in device memory, any alignment
 *   joints_uvd  [n][S][J][3] float32 in device memory (u, v read; d ignored), 1 <= S <= 4,
 *               0 <= J <= 128.  Centre = floor(u + 0.5), floor(v + 0.5); a joint whose centre is
 *               outside [-4096, 8191] (NaN, +-inf too) is not drawn and draws no bone
 *   bones       [nb][2] int32 indices into 0..J-1 in HOST memory (read at the call), 0 <= nb <= 256,
 *               shared by all sets and frames; NULL with nb = 0
 *   style       per set: marker colour and radius 0..15 (0: one pixel; covered iff dx^2 + dy^2 <= r^2),
 *               bone colour and thickness 1..15 (covered iff the pixel projects onto the segment and
 *               4 cross^2 <= th^2 |PQ|^2, in int64; the caps are the markers').  struct_size =
 *               sizeof(mp_overlay_style), checked
 *   out         [n][h][w][3] uint8 RGB in device memory at any byte address
 * A pixel takes the LAST primitive covering it in the order: for each set, its bones in list order,
 * then its joints in index order; else the depth colour.  No blending, text or anti-aliasing.
 * MP_ERR_SHAPE: n, h, w, S, J or nb out of range; MP_ERR_ARG: everything else. */
typedef struct {
  uint8_t marker_rgb[3];
  uint8_t radius;
  uint8_t bone_rgb[3];
  uint8_t thickness;
} mp_overlay_set_style;
typedef struct {
  uint64_t struct_size;          /* sizeof(mp_overlay_style) as the caller was compiled */
  mp_overlay_set_style sets[4];  /* the first S are read */
} mp_overlay_style;
int mp_overlay_dev(const void* frames, int depth_dtype, int64_t n, int64_t h, int64_t w, float lo, float hi,
                   const uint8_t* lut, const float* joints_uvd, int64_t S, int64_t J, const int32_t* bones, int64_t nb,
                   const mp_overlay_style* style, uint8_t* out, void* stream);

/* The uvd half of getRelativeCoordinates (monkeydetector.py:341-354) for a batch, i.e. joints in the
 * crop's pixel space (what save_result_image draws on the patch): joints_uvd [n][joints][3] float32,
 * Ms [n][9] float64 (the crops' transforms), device memory.  Per joint, in float64 and not fused:
 * t_i = (u * M_i0 + v * M_i1) + M_i2; out = (f32(t_0 / t_2), f32(t_1 / t_2), d).  Asynchronous. */
int mp_transform_joints_dev(const float* joints_uvd, const double* Ms, int64_t n, int64_t joints, float* out,
                            void* stream);

/* ---- HBM streaming probe (diagnostic; bench.py's practical roof) ----------------------------
 * The box's streaming HBM rates over `bytes`-sized buffers (>= 64 MiB; 2 GiB recommended):
 * read-only, write-only and copy (read + write bytes / time), each the best over grids of 1024 -
 * 8192 blocks of 256 threads, 1 / 4 / 8 16-byte accesses per thread in flight and default or
 * non-temporal policy (the chosen form is reported).  The ceiling the HBM-bound FFT-path kernels
 * are read against, next to the 8 TB/s spec figure.  Synchronous; not on any product path. */
typedef struct {
  double read_gbps, write_gbps, copy_gbps;
  int32_t read_grid, read_unroll, read_nt;
  int32_t write_grid, write_unroll, write_nt;
  int32_t copy_grid, copy_unroll, copy_nt;
} mp_hbm_rates;
int mp_hbm_probe(int device, int64_t bytes, mp_hbm_rates* out);

/* ---- TF1 checkpoint support (host only; monkey-pose_amd/tf_checkpoint.py) ----
 * CRC-32C (Castagnoli, reflected 0x82F63B78) of n bytes continuing from `init` (0 to start), as
 * tensor_bundle (BundleEntryProto.crc32c) and LevelDB-format table blocks store it before masking.
 * Replaces the checksum half of tf.train.NewCheckpointReader (train_cnn_networks_hgru.py:248-250,
 * 312-313: saver.restore). */
uint32_t mp_crc32c(uint32_t init, const void* data, size_t n);

/* ---- TFRecord ingestion (host only; monkey-pose_amd/data_loader.py) ----------
 * Replaces tf.TFRecordReader + tf.parse_single_example + tf.decode_raw (data_loader.py:10-26) and
 * tf.python_io.TFRecordWriter + encode_example (Datareader.py:13-27).  A reader memory-maps the
 * file and indexes its records once (length CRCs always checked, payload CRCs when verify != 0). */
typedef struct mp_tfrecord mp_tfrecord;
int mp_tfrecord_open(const char* path, int verify, mp_tfrecord** out, int64_t* n_records);
void mp_tfrecord_close(mp_tfrecord* r);
/* byte size of bytes feature `feature` (BytesList value[0], or a packed FloatList) of record rec */
int mp_tfrecord_feature_size(mp_tfrecord* r, int64_t rec, const char* feature, int64_t* bytes);
/* decode_raw gather: out[i] = the raw bytes of `feature` in record indices[i], each exactly
 * bytes_per_record (else MP_ERR_SHAPE), decoded by up to nthreads host threads */
int mp_tfrecord_read(mp_tfrecord* r, const int64_t* indices, int64_t count, const char* feature, void* out,
                     int64_t bytes_per_record, int nthreads);
/* write n_records tf.train.Example records {names[k]: bytes_feature(data[k] + i * bytes_per_record[k])}
 * (features in the given order), creating or (append != 0) extending the file */
int mp_tfrecord_write(const char* path, int64_t n_records, int n_features, const char* const* names,
                      const void* const* data, const int64_t* bytes_per_record, int append);

#ifdef __cplusplus
}
#endif

#endif /* MONKEYPOSE_H */
