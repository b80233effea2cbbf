"""Base class of the HIP-backed backbones and the autograd bridge to libopendpd_hip.so.

The reference backbones are nn.Modules composed of ATen ops with the duck type
`forward(x:(B,T,2), h_0) -> (B,T,2)` (models.py:150-160).  A NativeBackbone keeps the same
parameters (same names, shapes and registration order, so `state_dict()` is interchangeable with
the reference's) but stores them as views into ONE contiguous fp32 buffer — the `params` pointer
of the C ABI — and runs forward/backward as hand-written HIP kernels.
"""
import ctypes as C
import math

import torch
import torch.nn as nn

from .. import _lib


class RnnParams(nn.Module):
    """Parameter holder with torch.nn.GRU / nn.LSTM's names and construction-time RNG consumption
    (uniform(-1/sqrt(H), 1/sqrt(H)) over weight_ih_l0, weight_hh_l0, bias_ih_l0, bias_hh_l0 in that
    order), so that `reset_parameters()` afterwards sees the same generator state as the reference."""

    def __init__(self, input_size, hidden_size, gates, num_layers=1):
        super().__init__()
        self.input_size, self.hidden_size, self.gates, self.num_layers = input_size, hidden_size, gates, num_layers
        G = gates * hidden_size
        self.weight_ih_l0 = nn.Parameter(torch.empty(G, input_size))
        self.weight_hh_l0 = nn.Parameter(torch.empty(G, hidden_size))
        self.bias_ih_l0 = nn.Parameter(torch.empty(G))
        self.bias_hh_l0 = nn.Parameter(torch.empty(G))
        for layer in range(1, num_layers):      # torch.nn.RNNBase registers (and initialises) layer after layer; a layer's input is the one below's state
            setattr(self, f"weight_ih_l{layer}", nn.Parameter(torch.empty(G, hidden_size)))
            setattr(self, f"weight_hh_l{layer}", nn.Parameter(torch.empty(G, hidden_size)))
            setattr(self, f"bias_ih_l{layer}", nn.Parameter(torch.empty(G)))
            setattr(self, f"bias_hh_l{layer}", nn.Parameter(torch.empty(G)))
        stdv = 1.0 / math.sqrt(hidden_size) if hidden_size > 0 else 0
        for w in self.parameters():
            nn.init.uniform_(w, -stdv, stdv)


def init_gatewise(rnn, hidden_size, xavier_suffix="weight_ih_l0"):
    """Initialisation rule shared by the reference's recurrent backbones (e.g. gru.py:27-37):
    biases 0; every H-row gate block of a weight orthogonal; gate blocks of the input weight
    re-drawn xavier-uniform.  Same call order => same RNG consumption."""
    for name, p in rnn.named_parameters():
        n_gates = p.shape[0] // hidden_size
        if "bias" in name:
            nn.init.constant_(p, 0)
        if "weight" in name:
            for g in range(n_gates):
                nn.init.orthogonal_(p[g * hidden_size:(g + 1) * hidden_size, :])
        if xavier_suffix in name:
            for g in range(n_gates):
                nn.init.xavier_uniform_(p[g * hidden_size:(g + 1) * hidden_size, :])


def init_linear(lin, weight="xavier"):
    for name, p in lin.named_parameters():
        if "weight" in name:
            if weight == "xavier":
                nn.init.xavier_uniform_(p)
            elif weight == "kaiming":
                nn.init.kaiming_uniform_(p)
            elif weight == "orthogonal":
                nn.init.orthogonal_(p)
        if "bias" in name:
            nn.init.constant_(p, 0)


class _BackboneFn(torch.autograd.Function):
    """y = backbone(x) through odpd_backbone_fwd / odpd_backbone_bwd — or, given an initial state h_0 (1, B, H), through
    odpd_backbone_fwd_state / odpd_backbone_bwd_state (ODPD_FLAG_INIT_STATE: the lane-per-unit kernels of gru_wide.hip / lstm_wide.hip),
    whose backward also returns dL/dh_0 in h_0's dtype and shape.

    The forward states its kernel selection as ONE descriptor (NativeBackbone.call_desc) and the backward sizes and launches with that same
    object.  The kernel-selection knobs (odpd_set_tuning) choose the kernel, and with it the checkpoint layout, at each of the two calls, and
    the checkpoint carries no record of the layout it was written in.  So the backward refuses to run when odpd_tuning_generation moved since
    its forward wrote the checkpoints.  The rule is deliberately conservative: any movement refuses, also a knob set and then set back."""

    @staticmethod
    def forward(ctx, x, h_0, mod, grad_mode, *params):
        from ..train_funcs import ckpt_buffer
        lib = _lib.load()
        if not x.is_cuda:
            raise RuntimeError("opendpd_amd backbones run on a HIP device only (no CPU fallback)")
        x = x.contiguous().float()
        B, T = x.shape[0], x.shape[1]
        h0 = None if h_0 is None else h_0.detach().reshape(B, mod.hidden_size).float().contiguous()      # the kernels run in fp32
        flat = mod.flat_params()
        # (needs_input_grad looks at requires_grad only: under torch.no_grad() — net_eval, run_dpd — nothing will call backward, so no
        # checkpoints are asked for and the kernels may take their inference path)
        need_grad = grad_mode and any(ctx.needs_input_grad)      # (autograd switches grad mode off inside forward: the caller passes it)
        # delta backbones: dL/dx lives in the 16-sequences-per-wave kernels only; the flag routes forward, checkpoint sizing and backward of
        # THIS call to them (include/opendpd_hip.h: ODPD_FLAG_NEED_DX)
        d = ctx.desc = mod.call_desc(need_dx=ctx.needs_input_grad[0], init_state=h0 is not None)
        ctx.generation = None
        y = torch.empty_like(x)
        ckpt = None
        if need_grad:
            ctx.generation = int(lib.odpd_tuning_generation())      # (before the size query: the layout is the one of this generation)
            ckpt = ckpt_buffer(d, B, T, x.device)
        if h0 is None:
            rc = lib.odpd_backbone_fwd(_lib.stream_ptr(), C.byref(d), B, T, _lib.ptr(flat), _lib.ptr(x), _lib.ptr(y), _lib.ptr(ckpt),
                                       _lib.ptr(mod._stats_buffer(x.device)))
            _lib.check(rc, f"odpd_backbone_fwd[{mod.backbone_name}]")
        else:
            rc = lib.odpd_backbone_fwd_state(_lib.stream_ptr(), C.byref(d), B, T, _lib.ptr(flat), _lib.ptr(x), _lib.ptr(h0), _lib.ptr(y),
                                             _lib.ptr(ckpt))
            _lib.check(rc, f"odpd_backbone_fwd_state[{mod.backbone_name}]")
            ctx.h0_dtype, ctx.h0_shape = h_0.dtype, h_0.shape
        ctx.mod = mod
        ctx.save_for_backward(x, ckpt if ckpt is not None else x.new_empty(0), flat, *(() if h0 is None else (h0,)))
        return y

    @staticmethod
    def backward(ctx, dy):
        from ..train_funcs import partials_buffer
        lib = _lib.load()
        mod, d = ctx.mod, ctx.desc
        x, ckpt, flat, *h0 = ctx.saved_tensors
        B, T = x.shape[0], x.shape[1]
        if ctx.generation is not None and int(lib.odpd_tuning_generation()) != ctx.generation:
            raise RuntimeError(f"{mod.backbone_name}: the kernel-selection knobs (odpd_set_tuning) changed between forward and backward; "
                               "the checkpoints of the forward may be laid out for another kernel, so no gradients were written. "
                               "Run the forward again under the current knobs.")
        need_dx, need_dh0 = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        need_w = any(ctx.needs_input_grad[4:])
        if not (need_w or need_dx or need_dh0):
            return (None,) * len(ctx.needs_input_grad)
        dy = dy.contiguous().float()
        P = mod.n_flat
        partials = dx = dh0 = None
        if need_w or (need_dx and mod.dx_needs_flag):      # the delta kernels compute the weight gradients in every backward launch
            partials = partials_buffer(d, (B,), T, 0, P, x.device)
        if need_dx:
            dx = torch.empty_like(x)
        ck = _lib.ptr(ckpt) if ckpt.numel() else None
        if not h0:
            rc = lib.odpd_backbone_bwd(_lib.stream_ptr(), C.byref(d), B, T, _lib.ptr(flat), _lib.ptr(x), _lib.ptr(dy), ck, _lib.ptr(partials),
                                       _lib.ptr(dx))
            _lib.check(rc, f"odpd_backbone_bwd[{mod.backbone_name}]")
        else:
            if need_dh0:
                dh0 = torch.empty_like(h0[0])
            rc = lib.odpd_backbone_bwd_state(_lib.stream_ptr(), C.byref(d), B, T, _lib.ptr(flat), _lib.ptr(x), _lib.ptr(h0[0]), _lib.ptr(dy), ck,
                                             _lib.ptr(partials), _lib.ptr(dx), _lib.ptr(dh0))
            _lib.check(rc, f"odpd_backbone_bwd_state[{mod.backbone_name}]")
            if dh0 is not None:
                dh0 = dh0.view(ctx.h0_shape).to(ctx.h0_dtype)
        gparams = (None,) * (len(ctx.needs_input_grad) - 4)
        if need_w:
            grad = torch.empty(P + _lib.LOSS_COLS, dtype=torch.float32, device=x.device)
            rc = lib.odpd_reduce_partials(_lib.stream_ptr(), partials.shape[0], P, _lib.ptr(partials), _lib.ptr(grad), 0)
            _lib.check(rc, "odpd_reduce_partials")
            gparams = tuple(grad[o:o + n].view(shape) if need else None
                            for (o, n, shape), need in zip(mod._slices, ctx.needs_input_grad[4:]))
        return (dx, dh0, None, None) + gparams


# how the reference's backbone treats the h_0 argument of CoreModel.forward (models.py:150-160), per NativeBackbone subclass:
#   "state"    the initial state of the recurrence (gru.py:45, dgru.py:70, qgru.py, qgru_amp1.py; lstm.py:46: h and c)
#   "ignored"  never read, or set to None / zeros (deltagru, deltajanet, deltagru_tcnskip, vdlstm, apnrru, mcldnn, gmp, tcnn, rvtdcnn, neuraltx)
#   "refused"  an initial state the kernels do not take (pgjanet, bojanet, dvrjanet, quantised models)
H0_STATE, H0_IGNORED, H0_REFUSED = "state", "ignored", "refused"


class NativeBackbone(nn.Module):
    """nn.Module whose parameters are views into one flat fp32 buffer consumed by the HIP kernels."""

    backbone_name = None
    native = True
    dx_needs_flag = False      # True for the delta backbones (ODPD_FLAG_NEED_DX)
    initial_state = H0_REFUSED

    mode_selects_kernel = False      # True where train() / eval() of the module selects a kernel (ODPD_FLAG_EVAL: the quantised models)

    def _finalize(self, hidden_size, thx=0.0, thh=0.0, bits_w=0, bits_a=0, flags=0):
        """Call at the end of __init__ once every parameter holder is registered.  The arguments are the structural fields of the
        model's odpd_model_t (`flags`: ODPD_FLAG_TWO_LAYERS, ODPD_FLAG_QUANT_CELL), fixed from here on."""
        self._desc_fields = (_lib.BACKBONE_IDS[self.backbone_name], int(hidden_size), float(thx), float(thh), int(bits_w), int(bits_a))
        self._desc_flags = int(flags)
        self._call_descs = {}
        self._slices = []
        off = 0
        for p in self.parameters():
            self._slices.append((off, p.numel(), tuple(p.shape)))
            off += p.numel()
        self.n_flat = off
        self._flat = None
        self._stats = None
        self._sentinels = None

    # -- flat parameter buffer ---------------------------------------------------------------
    def _reflatten(self):
        ps = list(self.parameters())
        dev = ps[0].device
        with torch.no_grad():
            flat = torch.cat([p.detach().reshape(-1).float() for p in ps]).contiguous().to(dev)
            for p, (o, n, shape) in zip(ps, self._slices):
                p.data = flat[o:o + n].view(shape)
        self._flat = flat
        # first and last parameter stand guard for the whole buffer on the per-step fast path
        self._sentinels = ((ps[0], 0), (ps[-1], 4 * self._slices[-1][0]))

    def flat_params(self, full_check=False):
        """The contiguous parameter buffer (re-built if a parameter was re-pointed, e.g. by .to() — `_apply` drops it;
        the per-call check looks at the first and last parameter only, `full_check` at every one)."""
        f = self._flat
        ok = f is not None
        if ok:
            base = f.data_ptr()
            if full_check:
                for p, (o, n, _) in zip(self.parameters(), self._slices):
                    if p.data_ptr() != base + 4 * o or p.device != f.device:
                        ok = False
                        break
            else:
                for p, off in self._sentinels:
                    if p.data_ptr() != base + off:
                        ok = False
                        break
        if not ok:
            self._reflatten()
        return self._flat

    def _apply(self, fn, *args, **kwargs):
        out = super()._apply(fn, *args, **kwargs)
        self._flat = None
        return out

    # -- descriptors -------------------------------------------------------------------------
    def _mode_flag(self):
        return _lib.FLAG_EVAL if self.mode_selects_kernel and not self.training else 0

    def _make_desc(self, call_flags):
        """The one place that builds this model's odpd_model_t: the structural fields plus the flags of one call."""
        return _lib.ModelDesc(*self._desc_fields, self._desc_flags | call_flags)

    @property
    def desc(self):
        """A fresh odpd_model_t of the module as it stands (structural flags; ODPD_FLAG_EVAL where the mode selects a kernel and the module is
        in eval()): the caller's own copy, for a raw call into the library — editing it never reaches the module."""
        return self._make_desc(self._mode_flag())

    def call_desc(self, need_dx=False, init_state=False):
        """The odpd_model_t of ONE call: the per-call kernel selections ODPD_FLAG_NEED_DX (honoured where dx_needs_flag) and
        ODPD_FLAG_INIT_STATE on top of `desc`.  Cached per selection and shared between callers: read-only."""
        flags = (self._mode_flag() | (_lib.FLAG_NEED_DX if need_dx and self.dx_needs_flag else 0)
                 | (_lib.FLAG_INIT_STATE if init_state else 0))
        d = self._call_descs.get(flags)
        if d is None:
            d = self._call_descs[flags] = self._make_desc(flags)
        return d

    def _stats_buffer(self, device):
        return None

    def forward(self, x, h_0=None):
        return _BackboneFn.apply(x, None, self, torch.is_grad_enabled(), *self.parameters())

    def state_refusal(self):
        """None when this model can start from a given state on the kernels (forward_state), else the reason it cannot."""
        if self._desc_fields[4] > 0 and self.backbone_name != "dvrjanet":      # (bits_w; dvrjanet: it carries num_dvr_units)
            return f"quantised '{self.backbone_name}'"
        if self.initial_state != H0_STATE:
            return f"'{self.backbone_name}'"
        if self._desc_flags & _lib.FLAG_TWO_LAYERS:
            return f"two-layer '{self.backbone_name}'"
        return None

    def forward_state(self, x, h_0):
        """y = backbone(x) from the initial state h_0 (1, B, H); h_0 may require grad (the state route, ODPD_FLAG_INIT_STATE)."""
        return _BackboneFn.apply(x, h_0, self, torch.is_grad_enabled(), *self.parameters())
