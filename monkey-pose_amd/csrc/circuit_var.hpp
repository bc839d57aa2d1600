// The per-channel update rule of every ContextualCircuit variant the general loop runs
// (hgru_module.py:692-849), stated once for the epilogue kernels (k_circuit_var.hip) and for a host
// evaluator (mp_circuit_var_rule_host, the CPU test).  Everything after the two gate pre-activations
// O . i_r + i_b and I' . o_r + o_b is here; the 1x1 gate products and the association-field conv are
// the caller's.
//
//   g1   = sigmoid(O . i_r + i_b)                                     696-707
//   P1   = conv(A_in, p_r) + lateral_bias;  P1 = min(P1, 0) if rectify          714-722, 657
//   s    = nl(xi X - (beta r + nu) P1),  r = I (mely) or O (alternate, control) 758-804
//   I'   = g1 I + (1 - g1) s  (blend_in)  or  s
//   g2   = sigmoid(I' . o_r + o_b)                                    729-740
//   P2   = conv(B_in, p_r) + lateral_bias;  P2 = max(P2, 0) if rectify          746-754
//   e    = gamma P2;  s = nl(kappa (zeta I' + e) + omega (zeta I' e))  (mult)  or  nl(zeta I' + e)
//   O'   = g2 O + (1 - g2) s  (blend_out)  or  s;   O' *= rho[t] if adapt      769-849
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MP_CV_HD __host__ __device__
#else
#define MP_CV_HD
#endif

#include <cmath>
#include <cstdint>

namespace mpcv {

enum Nl { NL_TANH = 0, NL_RELU = 1, NL_SELU = 2, NL_LEAKY_RELU = 3, NL_HARD_TANH = 4, NL_COUNT = 5 };
enum Integration { INT_ALTERNATE = 0, INT_MELY = 1, INT_CONTROL = 2, INT_COUNT = 3 };

// one variant, passed to the kernels by value (wave-uniform)
struct CircuitVariant {
  uint8_t gru_gates;   // A_in = O g1 (else O)                                   709-711
  uint8_t out_gates;   // output_gru_gates: B_in = I' g2 (else I')               742-743
  uint8_t blend_in;    // I' = g1 I + (1 - g1) s: no gru_gates, alternate / mely 765, 802
  uint8_t blend_out;   // O' = g2 O + (1 - g2) s: mely, or alternate without output_gru_gates
  uint8_t rectify;     // rectify_weights is False                               721-722, 753-754
  uint8_t mult;        // multiplicative_excitation (alternate / control)        784-793, 808-819
  uint8_t adapt;       // adapation: O' *= rho[t]                                847-849
  uint8_t nl;          // Nl
  uint8_t integration; // Integration
};

// the four derived flags from the aux booleans
MP_CV_HD inline CircuitVariant make_variant(bool gru_gates, bool out_gates, bool rectify, bool mult, bool adapt,
                                            int nl, int integration) {
  CircuitVariant v{};
  v.gru_gates = gru_gates;
  v.out_gates = out_gates;
  v.blend_in = integration != INT_CONTROL && !gru_gates;
  v.blend_out = integration == INT_MELY || (integration == INT_ALTERNATE && !out_gates);
  v.rectify = rectify;
  v.mult = mult && integration != INT_MELY;
  v.adapt = adapt;
  v.nl = (uint8_t)nl;
  v.integration = (uint8_t)integration;
  return v;
}
// whether the previous I is read at all (its initial draw is then a live input)
MP_CV_HD inline bool reads_prev_i(const CircuitVariant& v) { return v.blend_in || v.integration == INT_MELY; }

MP_CV_HD inline float sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

// recurrent_nl by name (hgru_module.py:130-143); selu / leaky_relu with TensorFlow's constants
template <int NL>
MP_CV_HD inline float nl(float x) {
  if (NL == NL_TANH) return tanhf(x);
  if (NL == NL_RELU) return fmaxf(x, 0.f);
  if (NL == NL_SELU) return 1.0507009873554805f * (x > 0.f ? x : 1.6732632423543772f * expm1f(x));
  if (NL == NL_LEAKY_RELU) return x > 0.f ? x : 0.2f * x;
  return fmaxf(fminf(x, 1.f), 0.f);   // hard_tanh as the reference writes it (141)
}

// per-channel constants of the two halves (learned, or the constant the aux makes them: 404-497)
struct InConst {
  float lat, beta, nu, xi;
};
struct OutConst {
  float lat, gamma, kappa, omega, zeta;
};

// I' of one channel; p1: the conv result before lateral_bias, g1p: the gate pre-activation
template <int NL>
MP_CV_HD inline float rule_in(const CircuitVariant& v, float p1, float x, float o, float iprev, float g1p,
                              const InConst& c) {
  float P = p1 + c.lat;
  if (v.rectify) P = fminf(P, 0.f);
  const float r = v.integration == INT_MELY ? iprev : o;
  const float s = nl<NL>(c.xi * x - (c.beta * r + c.nu) * P);
  if (!v.blend_in) return s;
  const float g1 = sigmoid(g1p);
  return g1 * iprev + (1.f - g1) * s;
}

// O' of one channel; p2: the conv result before lateral_bias, g2p: the gate pre-activation
template <int NL>
MP_CV_HD inline float rule_out(const CircuitVariant& v, float p2, float ip, float o, float g2p, float rho,
                               const OutConst& c) {
  float P = p2 + c.lat;
  if (v.rectify) P = fmaxf(P, 0.f);
  const float e = c.gamma * P;
  const float zi = c.zeta * ip;
  const float s = v.mult ? nl<NL>(c.kappa * (zi + e) + c.omega * (zi * e)) : nl<NL>(zi + e);
  float on = s;
  if (v.blend_out) {
    const float g2 = sigmoid(g2p);
    on = g2 * o + (1.f - g2) * s;
  }
  if (v.adapt) on *= rho;
  return on;
}

// the same rules with the nonlinearity chosen at run time (host evaluator)
inline float rule_in_any(const CircuitVariant& v, float p1, float x, float o, float iprev, float g1p,
                         const InConst& c) {
  switch (v.nl) {
    case NL_TANH: return rule_in<NL_TANH>(v, p1, x, o, iprev, g1p, c);
    case NL_RELU: return rule_in<NL_RELU>(v, p1, x, o, iprev, g1p, c);
    case NL_SELU: return rule_in<NL_SELU>(v, p1, x, o, iprev, g1p, c);
    case NL_LEAKY_RELU: return rule_in<NL_LEAKY_RELU>(v, p1, x, o, iprev, g1p, c);
    default: return rule_in<NL_HARD_TANH>(v, p1, x, o, iprev, g1p, c);
  }
}
inline float rule_out_any(const CircuitVariant& v, float p2, float ip, float o, float g2p, float rho,
                          const OutConst& c) {
  switch (v.nl) {
    case NL_TANH: return rule_out<NL_TANH>(v, p2, ip, o, g2p, rho, c);
    case NL_RELU: return rule_out<NL_RELU>(v, p2, ip, o, g2p, rho, c);
    case NL_SELU: return rule_out<NL_SELU>(v, p2, ip, o, g2p, rho, c);
    case NL_LEAKY_RELU: return rule_out<NL_LEAKY_RELU>(v, p2, ip, o, g2p, rho, c);
    default: return rule_out<NL_HARD_TANH>(v, p2, ip, o, g2p, rho, c);
  }
}

}  // namespace mpcv
