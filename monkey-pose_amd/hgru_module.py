"""Drop-in for ``/root/reference/hgru_module.py``: ``ContextualCircuit(X, ...).build()``.

Runs the forward branches of ``circuit_input`` / ``circuit_output`` / ``input_integration`` /
``output_integration`` and their ``mely_*`` / ``*_control`` forms (``hgru_module.py:692-857``) for
the association-field eCRF with a full SSFxSSF conv (SSF_ext in {3, 5, 15}) and 1x1 gates: the
module's own defaults (``auxilliary_variables``, 9-51), ``gru_gates`` / ``output_gru_gates`` on or
off, ``multiplicative_excitation``, learned or constant ``beta`` / ``nu`` / ``gamma`` / ``zeta`` /
``xi``, the four lesions, ``rectify_weights=False``, ``adapation``, ``integration_type`` in
'alternate' / 'mely' / 'control', ``recurrent_nl`` in 'tanh' / 'relu' / 'selu' / 'leaky_relu' /
'hard_tanh', any ``hidden_init`` ('random', 'zeros', 'identity') and ``store_states``.

The configuration the pose model uses (``hgru_pose.py:20-39`` merged over the defaults) takes the
fused loop; every other one the general loop (conv -> P map -> epilogue kernel per half-step,
DESIGN.md 3e).  Options outside that family raise ``NotImplementedError`` naming the option rather
than silently computing something else.  Inference only.
"""
from __future__ import annotations

import math
from typing import Dict, Optional

import numpy as np

from . import _lib
from . import weights as W

# the effective aux of hgru_pose (hgru_pose.py:20-39 over hgru_module.py:9-51): the fused loop
POSE_AUX = {
    'recurrent_nl': 'tanh', 'rectify_weights': None, 'gate_filter': 1, 'xi': False,
    'zeta': False, 'gamma': True, 'beta': True, 'nu': True, 'batch_norm': False,
    'atrous_convolutions': False, 'output_gru_gates': False, 'association_field': True,
    'multiplicative_excitation': True, 'gru_gates': True, 'adapation': True,
    'dense_connections': False, 'integration_type': 'alternate',
    'lesion_beta': False, 'lesion_nu': False, 'lesion_omega': False, 'lesion_kappa': False,
    'dropout': None,
}
SUPPORTED_AUX = POSE_AUX
# keys with more than one implemented value
CHOICE_AUX = {'hidden_init': ('random', 'zeros', 'identity'), 'store_states': (False, True),
              'recurrent_nl': tuple(_lib.MP_NL), 'integration_type': tuple(_lib.MP_INT),
              'rectify_weights': (None, False)}
# boolean switches, every combination implemented (hgru_module.py:404-497, 692-849)
FLAG_AUX = ('gru_gates', 'output_gru_gates', 'multiplicative_excitation', 'adapation', 'beta', 'nu', 'gamma',
            'zeta', 'xi', 'lesion_beta', 'lesion_nu', 'lesion_kappa', 'lesion_omega')
# options with one implemented value; anything else raises NotImplementedError naming the key
FIXED_AUX = {'gate_filter': 1, 'association_field': True, 'batch_norm': False, 'dense_connections': False,
             'atrous_convolutions': False, 'dropout': None}
# keys that only affect training / initialisation, never the forward values
_IGNORED = {'symmetric_weights', 'symmetric_gate_weights', 'trainable', 'pre_batchnorm',
            'post_batchnorm', 'train', 'normal_initializer', 'gate_bias_init', 'dtype',
            'return_weights', 'lesions', 'tuning_nl', 'gate_nl', 'ecrf_nl', 'post_tuning_nl'}

_DEFAULTS = {  # auxilliary_variables() values for the keys checked above (hgru_module.py:13-51)
    'recurrent_nl': 'tanh', 'rectify_weights': None, 'gate_filter': 1, 'xi': False, 'zeta': False,
    'gamma': True, 'beta': True, 'nu': True, 'batch_norm': False, 'atrous_convolutions': False,
    'output_gru_gates': False, 'association_field': True, 'multiplicative_excitation': True,
    'gru_gates': False, 'adapation': False, 'dense_connections': False,
    'integration_type': 'alternate', 'hidden_init': 'random', 'lesion_beta': False,
    'lesion_nu': False, 'lesion_omega': False, 'lesion_kappa': False, 'dropout': None,
    'store_states': False,
}


def merged_aux(aux: Optional[dict] = None) -> dict:
    """``auxilliary_variables()`` with the caller's aux merged over it (hgru_module.py:81-85)."""
    merged = dict(_DEFAULTS)
    if aux is not None and isinstance(aux, dict):
        merged.update(aux)
    return merged


def validate_aux(merged: dict) -> None:
    """NotImplementedError, naming the option, for anything outside the implemented family."""
    nl = merged.get('recurrent_nl')
    if not isinstance(nl, str):
        raise NotImplementedError(f"recurrent_nl must be given by name {CHOICE_AUX['recurrent_nl']}, got {nl!r}")
    rw = merged.get('rectify_weights')
    if rw is not None and rw is not False:
        raise NotImplementedError(f"rectify_weights={rw!r}: the reference calls None(p_weights, 0) "
                                  "(p_convolution's rectification is None, hgru_module.py:619, 717)")
    for key, val in FIXED_AUX.items():
        got = merged.get(key)
        if (bool(got) != val) if isinstance(val, bool) else (got != val):
            raise NotImplementedError(f"aux {key}={got!r} is not implemented (only {key}={val!r})")
    for key, ok in CHOICE_AUX.items():
        if key != 'rectify_weights' and merged.get(key) not in ok:
            raise NotImplementedError(f"aux {key}={merged.get(key)!r} is not implemented (one of {ok})")
    unknown = set(merged) - set(FIXED_AUX) - set(CHOICE_AUX) - set(FLAG_AUX) - _IGNORED
    if unknown:
        raise NotImplementedError(f"unsupported aux keys: {sorted(unknown)}")


def is_pose_aux(merged: dict) -> bool:
    """the one configuration the fused loop computes"""
    for key, val in POSE_AUX.items():
        got = merged.get(key)
        if key in FLAG_AUX:
            if bool(got) != val:
                return False
        elif key == 'rectify_weights':
            if got is not None:
                return False
        elif got != val:
            return False
    return True


def variable_flags(merged: dict) -> Dict[str, bool]:
    """which optional variables ``prepare_tensors`` creates for this aux (hgru_module.py:404-497):
    the keyword arguments of ``weights.hgru_circuit_vars``"""
    mult = bool(merged['multiplicative_excitation'])
    return dict(beta=bool(merged['beta']) and not merged['lesion_beta'],
                nu=bool(merged['nu']) and not merged['lesion_nu'],
                zeta=bool(merged['zeta']), gamma=bool(merged['gamma']), xi=bool(merged['xi']),
                kappa=mult and not merged['lesion_kappa'], omega=mult and not merged['lesion_omega'],
                rho=bool(merged['adapation']))


def reads_previous_i(merged: dict) -> bool:
    """whether the initial I reaches the output: the forget gate on the input state
    (gru_gates off with 'alternate' / 'mely', hgru_module.py:765, 802) or mely's beta * I (762)"""
    it = merged['integration_type']
    return it == 'mely' or (it == 'alternate' and not merged['gru_gates'])


class ContextualCircuit(object):
    """``hgru_module.ContextualCircuit`` (hgru_module.py:54-128)."""

    def __getitem__(self, name):
        return getattr(self, name)

    def __contains__(self, name):
        return hasattr(self, name)

    def __init__(self, X, timesteps=1, SRF=1, SSN=9, SSF=29, strides=[1, 1, 1, 1],
                 padding='SAME', aux=None, train=True):
        self.X = X
        self.n, self.h, self.w, self.k = [int(x) for x in X.shape]
        self.timesteps = timesteps
        self.strides = strides
        self.padding = padding
        self.train = train
        merged = merged_aux(aux)
        validate_aux(merged)
        for key, val in merged.items():
            setattr(self, key, val)
        self.aux = merged
        self.SRF, self.SSN, self.SSF = SRF, SSN, SSF
        if isinstance(SSF, list):
            raise NotImplementedError("hierarchical (list) SSF is not implemented")
        self.SSF_ext = 2 * int(math.floor(SSF / 2.0)) + 1                # hgru_module.py:97
        if self.SSF_ext not in (3, 5, 15):
            raise NotImplementedError(f"SSF={SSF} (SSF_ext={self.SSF_ext}): the association-field conv is "
                                      "implemented for SSF_ext in (3, 5, 15)")
        if list(strides) != [1, 1, 1, 1] or padding != 'SAME':
            raise NotImplementedError(f"strides={list(strides)} padding={padding!r}: only strides [1,1,1,1] "
                                      "with SAME padding")
        self.p_shape = [self.SSF_ext, self.SSF_ext, self.k, self.k]
        self.i_shape = [self.gate_filter, self.gate_filter, self.k, self.k]
        self.o_shape = [self.gate_filter, self.gate_filter, self.k, self.k]
        self.bias_shape = [1, 1, 1, self.k]
        self.weights: Optional[Dict[str, np.ndarray]] = None
        self.weight_seed = 1234
        self.hidden_seed = 7        # hidden_init 'random': call c draws synth_hidden(seed=hidden_seed + c)
        self.hidden_seed_i = 1007   # ... and the initial I synth_hidden(seed=hidden_seed_i + c)
        self._calls = 0
        self.scope = "contextual_circuit"

    def variable_table(self):
        """the variables the reference creates for this aux (``weights.hgru_circuit_vars``)"""
        return W.hgru_circuit_vars(k=self.k, ssf=self.SSF_ext, gate_filter=self.gate_filter,
                                   timesteps=self.timesteps, scope=self.scope, **variable_flags(self.aux))

    def prepare_tensors(self, weights: Optional[Dict[str, np.ndarray]] = None,
                        seed: Optional[int] = None) -> Dict[str, np.ndarray]:
        """Variables of ``prepare_tensors`` (hgru_module.py:172-503) keyed
        ``contextual_circuit/<name>``; given values win, the rest are synthesised."""
        table = self.variable_table()
        given = {}
        for k_, v in (weights or self.weights or {}).items():
            given[k_.split("/")[-1]] = v
        s = self.weight_seed if seed is None else seed
        out = {}
        for v in table:
            short = v.name.split("/")[-1]
            out[v.name] = (np.asarray(given[short], np.float32) if short in given
                           else W.synth_value(v, s, self.timesteps))
        return out

    def build(self, weights: Optional[Dict[str, np.ndarray]] = None, h2_init=None,
              compute_dtype: str = 'auto', reference_stack_order: bool = False, h1_init=None,
              general_loop: bool = False, nhwc_loop: bool = False, nhwc_conv: str = 'direct'):
        """Run the circuit; returns ``(O, weights, activities)`` like the reference with
        ``return_weights=True`` (hgru_module.py:939-954).  ``compute_dtype``: 'auto' (the FFT
        path when the map allows), 'fp32_fft', 'fp32_split', 'fp32' or 'bf16' (see
        include/monkeypose.h and _lib.resolve_dtype; 'bf16' only for the pose aux's fused loop).

        hidden_init (875-892): 'random' -> O0 = ``h2_init`` if given, else a fresh xavier-uniform
        draw made on the device for every call, as the reference redraws it every sess.run (the
        draw of call c is ``weights.synth_hidden(shape, seed=self.hidden_seed + c)``, bit for bit);
        'zeros' -> zeros_like(X), 'identity' -> X.  The initial I is made the same way (``h1_init``,
        else the draw ``weights.synth_hidden(shape, seed=self.hidden_seed_i + c)``); it is read only
        where the aux reads the previous I (``reads_previous_i``).
        store_states (889-915): O is the per-step stack ``[n, T, h, w, k]`` (O_t after the rho
        gain, 909-912) and ``weights['store_O']`` / ``weights['store_I']`` hold the O_t / I_t
        stacks.  (The reference's TensorArrays trade places every step -- ``full`` takes
        ``(store_O, store_I)`` where the loop passes ``(store_I, store_O)``, 825 vs 897-908 -- so
        its stacked "O" alternates O_t and I_t; here each stack holds what its name says.
        ``reference_stack_order=True`` returns the reference's interleaved stacks instead, see
        ``reference_stacks``.)

        The pose aux runs the fused loop; any other aux, or ``general_loop=True``, the general loop,
        which also returns the final I as ``weights['I']``.

        The channel count is X's: k = 64 runs those loops, any other k in [4, 256] the channel-general
        loop ('fp32_split', which 'auto' then means, or 'fp32'; any map size), through
        the same two entry points.  ``nhwc_loop=True`` sends a 64-channel circuit there too.
        ``nhwc_conv='fft'`` runs that loop's association-field conv as an FFT conv (k % 4 == 0,
        'fp32_split', maps up to 64 x 64, conv inputs with h * w * max|v| / 64 inside f16 range; see
        _lib.resolve_nhwc_conv); 'direct', the default, is the implicit-GEMM conv.  'auto' never picks 'fft':
        at ssf 3 and 5 the direct conv is the faster one (README).
        ``nhwc_conv='fft_tiled'`` is that FFT conv on maps of any size (overlap-save over
        windows of at most 64 x 64, the other conditions of 'fft'; one window, and 'fft' bit for bit, up to
        64 x 64).  Its range bound is per window: conv inputs keep min(h, 64) * min(w, 64) * max|v| / 64
        inside f16 range, so tanh-bounded states use 64 of it at any map size.  'auto' never picks it."""
        import torch
        X = self.X
        if not isinstance(X, torch.Tensor) or not X.is_cuda:
            raise TypeError("X must be a CUDA (ROCm) torch tensor [n, h, w, k]")
        conv = _lib.resolve_nhwc_conv(nhwc_conv, compute_dtype, X.shape[1], X.shape[2], self.k, nhwc_loop)
        if general_loop or not is_pose_aux(self.aux):
            return self._build_general(weights, h2_init, h1_init, compute_dtype, reference_stack_order, nhwc_loop, conv)
        if h1_init is not None:
            raise ValueError("h1_init is not read by the hgru_pose aux (gru_gates ignore the previous I)")
        wts = self.prepare_tensors(weights)
        ctx = _lib.Context(_lib.MP_MODEL_HGRU_CIRCUIT, X.device.index or 0)
        for name, val in wts.items():
            ctx.set_weight(name, val)
        if nhwc_loop:
            ctx.set_nhwc_loop(True)
        if conv != _lib.MP_CN_CONV_DIRECT:
            ctx.set_nhwc_conv(conv)
        ctx.finalize(_lib.dtype_code(_lib.resolve_dtype(compute_dtype, X.shape[1], X.shape[2], self.k, nhwc_loop)))
        X = X.detach().float().contiguous()
        hidden = _lib.MP_HIDDEN[self.hidden_init]
        call = 0
        if self.hidden_init == 'random':
            if h2_init is None:
                hidden = _lib.MP_HIDDEN_RANDOM          # drawn on the device, per call
                call = self._calls
                self._calls += 1
            else:
                h2_init = h2_init.detach().float().contiguous()
                if h2_init.shape != X.shape:
                    raise ValueError("h2_init must have the shape of X")
        elif h2_init is not None:
            raise ValueError(f"h2_init is only used with hidden_init='random' (got {self.hidden_init!r})")
        O = torch.empty_like(X)
        sO = sI = None
        if self.store_states:
            sO = torch.empty((X.shape[0], self.timesteps) + tuple(X.shape[1:]), dtype=torch.float32,
                             device=X.device)
            sI = torch.empty_like(sO)
        ctx.circuit_fwd(X, h2_init, O, self.timesteps, _lib.current_stream(X.device), hidden, sO, sI,
                        rng_seed=self.hidden_seed, rng_call=call)
        torch.cuda.current_stream(X.device).synchronize()
        ctx.close()
        self.h2_init = h2_init
        weights_out = {k_.split("/")[-1]: v for k_, v in wts.items()}
        weights_out['p_t'] = weights_out['p_r']
        if self.store_states:
            if reference_stack_order:
                sO, sI = reference_stacks(sO, sI)
            weights_out['store_O'], weights_out['store_I'] = sO, sI
            return sO, weights_out, {}
        return O, weights_out, {}

    def _build_general(self, weights, h2_init, h1_init, compute_dtype, reference_stack_order, nhwc_loop=False,
                       nhwc_conv=_lib.MP_CN_CONV_DIRECT):
        """``build`` through the general loop (mp_hgru_circuit_fwd_var)."""
        import torch
        X = self.X.detach().float().contiguous()
        dtype = _lib.resolve_dtype(compute_dtype, X.shape[1], X.shape[2], self.k, nhwc_loop)
        if dtype == 'bf16':
            raise NotImplementedError("compute_dtype='bf16' runs the hgru_pose aux's fused loop only; the general "
                                      "loop runs 'fp32_fft', 'fp32_split' or 'fp32'")
        wts = self.prepare_tensors(weights)
        hidden = _lib.MP_HIDDEN[self.hidden_init]
        call = 0
        given = [h2_init, h1_init]
        if self.hidden_init == 'random':
            live_i = reads_previous_i(self.aux)
            if h2_init is None and h1_init is None:
                hidden = _lib.MP_HIDDEN_RANDOM          # both drawn on the device, per call
                call = self._calls
                self._calls += 1
            elif h2_init is None or (live_i and h1_init is None):
                raise ValueError("give both h2_init and h1_init, or neither (then both are drawn)")
            for j, t in enumerate(given):
                if t is not None:
                    given[j] = t.detach().float().contiguous()
                    if given[j].shape != X.shape:
                        raise ValueError("h2_init / h1_init must have the shape of X")
        elif h2_init is not None or h1_init is not None:
            raise ValueError(f"h2_init / h1_init are only used with hidden_init='random' (got {self.hidden_init!r})")
        variant = _lib.circuit_variant(self.aux, self.hidden_seed, self.hidden_seed_i, call)
        ctx = _lib.Context(_lib.MP_MODEL_HGRU_CIRCUIT, X.device.index or 0)
        ctx.set_circuit_variant(variant)
        if nhwc_loop:
            ctx.set_nhwc_loop(True)
        if nhwc_conv != _lib.MP_CN_CONV_DIRECT:
            ctx.set_nhwc_conv(nhwc_conv)
        for name, val in wts.items():
            ctx.set_weight(name, val)
        ctx.finalize(_lib.dtype_code(dtype))
        O = torch.empty_like(X)
        I = torch.empty_like(X)
        sO = sI = None
        if self.store_states:
            sO = torch.empty((X.shape[0], self.timesteps) + tuple(X.shape[1:]), dtype=torch.float32,
                             device=X.device)
            sI = torch.empty_like(sO)
        ctx.circuit_fwd_var(X, given[0], given[1], O, I, self.timesteps, _lib.current_stream(X.device), variant,
                            hidden, sO, sI)
        torch.cuda.current_stream(X.device).synchronize()
        ctx.close()
        self.h2_init, self.h1_init = given
        weights_out = {k_.split("/")[-1]: v for k_, v in wts.items()}
        weights_out['p_t'] = weights_out['p_r']
        weights_out['I'] = I
        if self.store_states:
            if reference_stack_order:
                sO, sI = reference_stacks(sO, sI)
            weights_out['store_O'], weights_out['store_I'] = sO, sI
            return sO, weights_out, {}
        return O, weights_out, {}


def reference_stacks(states_O, states_I):
    """The reference's own ``store_states`` stacks from the per-step O_t / I_t stacks [n, T, ...].

    ``full(self, i0, O, I, store_O=None, store_I=None)`` (hgru_module.py:825) is called by
    ``tf.while_loop`` with the loop variables ``[i0, O, I, store_I, store_O]`` (897-908) and returns
    them in its own parameter order (857), so the two TensorArrays trade places every step: after
    T steps the array returned as ``store_O`` (912-914) holds O_t where T-1-t is even and I_t
    elsewhere, and ``store_I`` the complement (pinned symbolically, tests/test_hgru_structure.py).
    Returns (O_ref, I_ref) with the reference's layout, for callers that relied on it."""
    import torch
    T = states_O.shape[1]
    pick = torch.tensor([(T - 1 - t) % 2 == 0 for t in range(T)], device=states_O.device)
    pick = pick.view((1, T) + (1,) * (states_O.dim() - 2))
    return torch.where(pick, states_O, states_I), torch.where(pick, states_I, states_O)
