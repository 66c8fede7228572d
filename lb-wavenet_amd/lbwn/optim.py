"""tf.train.AdamOptimizer drop-in (train.py:178, :186) over lbwn's flat buffers."""
import ctypes
import math

import torch

from . import _lib

EMA_SUFFIX = '/ExponentialMovingAverage'   # tf.train.ExponentialMovingAverage's shadow variable name
SKIPS_KEY = 'Adam/nonfinite_skips'


class AdamOptimizer:
    """TF1 Adam: lr_t = lr·√(1-β2^t)/(1-β1^t); m = β1m+(1-β1)g; v = β2v+(1-β2)g²;
    θ -= lr_t·m/(√v+ε).  g = Σxent-grad/n_valid + l2_factor·θ (non-BIAS), applied by ONE
    kernel (lbwn_adam_tf1) that also advances GLOBAL_STEP / VALID_SAMPLES.  The step's plan
    status word goes with it: a step whose chain hand-off timed out is skipped on the device
    and recorded in the cumulative status (WaveNetTrain.check_status), with no host sync.

    The options past ``epsilon`` all run on the device inside the step (lbwn_adam_ex; include/lbwn.h
    has the definitions): ``clip_norm`` clips by tf.global_norm, ``skip_nonfinite`` (implied by clipping)
    leaves a step with a NaN/Inf gradient norm unapplied and counts it, ``ema_decay`` keeps
    tf.train.ExponentialMovingAverage shadows of every variable (``ema_num_updates``: the
    min(decay, (1+t)/(10+t)) ramp), ``warmup_steps`` / ``decay_steps`` / ``decay_rate`` /
    ``decay_staircase`` schedule the learning rate from Adam's own step count, and ``log_norm`` makes
    the norm available (grad_info) without clipping.  With all of them neutral, apply() is the
    lbwn_adam_tf1 call it always was."""

    def __init__(self, learning_rate=0.001, beta1=0.9, beta2=0.999, epsilon=1e-8, clip_norm=None,
                 skip_nonfinite=False, ema_decay=None, ema_num_updates=True, warmup_steps=0, decay_steps=0,
                 decay_rate=1.0, decay_staircase=False, log_norm=False):
        self.lr, self.b1, self.b2, self.eps = float(learning_rate), float(beta1), float(beta2), float(epsilon)
        self.clip_norm = 0.0 if clip_norm is None else float(clip_norm)
        if not (math.isfinite(self.clip_norm) and self.clip_norm >= 0.0):
            raise ValueError('clip_norm must be None or 0 (off), or finite and > 0, got %r' % (clip_norm,))
        self.ema_decay = 0.0 if ema_decay is None else float(ema_decay)
        if not (0.0 <= self.ema_decay < 1.0):
            raise ValueError('ema_decay must be None (off) or in (0, 1), got %r' % (ema_decay,))
        self.warmup_steps, self.decay_steps = int(warmup_steps), int(decay_steps)
        if self.warmup_steps < 0:
            raise ValueError('warmup_steps must be >= 0, got %r' % (warmup_steps,))
        if self.decay_steps < 0:
            raise ValueError('decay_steps must be >= 0, got %r' % (decay_steps,))
        self.decay_rate = float(decay_rate)
        if self.decay_steps > 0 and not (0.0 < self.decay_rate <= 1.0):
            raise ValueError('decay_rate must be in (0, 1] when decay_steps > 0, got %r' % (decay_rate,))
        self.skip_nonfinite = bool(skip_nonfinite)
        self.ema_num_updates = bool(ema_num_updates)
        self.decay_staircase = bool(decay_staircase)
        self.log_norm = bool(log_norm)
        self._slots = {}
        self._ex = {}

    # ---- which call ---------------------------------------------------------------------------
    @property
    def norm_pass(self):
        """Whether the step computes the gradient's global norm (a launch of its own)."""
        return self.clip_norm > 0.0 or self.skip_nonfinite or self.log_norm

    @property
    def extended(self):
        """False when every option is neutral: apply() is then the plain lbwn_adam_tf1 call."""
        return self.norm_pass or self.ema_decay > 0.0 or self.warmup_steps > 0 or self.decay_steps > 0

    def slots(self, net):
        key = id(net)
        if key not in self._slots:
            self._slots[key] = (torch.zeros_like(net.flat), torch.zeros_like(net.flat))
        return self._slots[key]

    def ex_slots(self, net):
        """The net's buffers of the extended step: 'ema' (the shadow, a clone of net.flat at creation,
        None with EMA off), 'ws' and 'info' (None without the norm pass) and 'skips' (int64 [1])."""
        key = id(net)
        if key not in self._ex:
            dev = net.flat.device
            lib = getattr(net, 'lib', None) or _lib.load()
            n_ws = int(lib.lbwn_adam_ex_ws_floats(net.layout.n_total))
            self._ex[key] = dict(
                ema=net.flat.detach().clone() if self.ema_decay > 0.0 else None,
                ws=torch.zeros(max(n_ws, 4), dtype=torch.float32, device=dev) if self.norm_pass else None,
                info=torch.zeros(4, dtype=torch.float32, device=dev) if self.norm_pass else None,
                skips=torch.zeros(1, dtype=torch.int64, device=dev))
        return self._ex[key]

    def apply_gradients(self, grads_and_vars, stream=None):
        net = grads_and_vars.net
        self.apply(net, stream)

    def apply(self, net, stream=None):
        m, v = self.slots(net)
        if not self.extended:
            _lib.check(net.lib.lbwn_adam_tf1(net.flat.data_ptr(), net.grad_flat.data_ptr(), m.data_ptr(),
                                             v.data_ptr(), net.layout.n_weights, net.layout.n_total, self.lr,
                                             self.b1, self.b2, self.eps, net.l2_factor, net.stats.data_ptr(),
                                             net.counters.data_ptr(), net.status_ptr(), _lib.stream_ptr(stream)))
        else:
            ex = self.ex_slots(net)
            a = _lib.AdamExArgs(
                params=net.flat.data_ptr(), grads=net.grad_flat.data_ptr(), m=m.data_ptr(), v=v.data_ptr(),
                n_weights=net.layout.n_weights, n_total=net.layout.n_total, lr=self.lr, beta1=self.b1,
                beta2=self.b2, eps=self.eps, l2_factor=net.l2_factor, stats=net.stats.data_ptr(),
                counters=net.counters.data_ptr(), step_status=net.status_ptr(), clip_norm=self.clip_norm,
                skip_nonfinite=int(self.skip_nonfinite), ema_decay=self.ema_decay,
                ema_num_updates=int(self.ema_num_updates), ema=_lib.ptr(ex['ema']),
                lr_warmup_steps=self.warmup_steps, lr_decay_steps=self.decay_steps, lr_decay_rate=self.decay_rate,
                lr_decay_staircase=int(self.decay_staircase), ws=_lib.ptr(ex['ws']), info=_lib.ptr(ex['info']),
                nonfinite_skips=ex['skips'].data_ptr())
            _lib.check(net.lib.lbwn_adam_ex(ctypes.byref(a), _lib.stream_ptr(stream)))
        net.global_step_host += 1

    # ---- readouts -----------------------------------------------------------------------------
    def grad_info(self, net):
        """The device fp32[4] the last step wrote: the norm before clipping, the scale applied, 1 if the
        step was skipped as non-finite, the scheduled learning rate.  No synchronisation."""
        info = self.ex_slots(net)['info']
        if info is None:
            raise ValueError('grad_info needs clip_norm, skip_nonfinite or log_norm: the norm is not computed')
        return info

    def nonfinite_skips(self, net):
        """How many steps were left unapplied for a non-finite gradient norm (synchronises)."""
        return int(self.ex_slots(net)['skips'].item())

    def ema_tensors(self, net):
        """{variable name: view of its shadow}, the layout's names."""
        ema = self.ex_slots(net)['ema']
        if ema is None:
            raise ValueError('ema_tensors needs ema_decay: there are no shadows')
        return net.layout.views(ema)

    # ---- checkpoint state: TF's slot names (<var>/Adam = m, <var>/Adam_1 = v) ----------------
    def state_tensors(self, net):
        m, v = self.slots(net)
        out = {}
        for name, t in net.layout.views(m).items():
            out[name + '/Adam'] = t
        for name, t in net.layout.views(v).items():
            out[name + '/Adam_1'] = t
        out['Adam/step'] = net.counters[2:3]
        if self.ema_decay > 0.0:       # only when enabled: the default key set stays what it was
            for name, t in self.ema_tensors(net).items():
                out[name + EMA_SUFFIX] = t
        if self.ema_decay > 0.0 or self.norm_pass:
            out[SKIPS_KEY] = self.ex_slots(net)['skips']
        return out

    def load_state_tensors(self, net, loaded):
        """Restore the slots if the checkpoint has them (reference checkpoints do not:
        tmodel.py:330 saves only the model variables, so Adam restarts from zero).  With EMA on, the
        shadows come from the checkpoint, or, if it has none, from the loaded parameters."""
        m, v = self.slots(net)
        with torch.no_grad():
            if self.extended:
                ex = self.ex_slots(net)
                if ex['ema'] is not None:
                    for name, t in net.layout.views(ex['ema']).items():
                        t.copy_(loaded[name + EMA_SUFFIX] if name + EMA_SUFFIX in loaded else net.vars[name])
                if SKIPS_KEY in loaded:
                    ex['skips'].copy_(loaded[SKIPS_KEY].reshape(1))
                else:
                    ex['skips'].zero_()
            if 'Adam/step' not in loaded:
                m.zero_()
                v.zero_()
                net.counters[2:3].zero_()
                return False
            for name, t in net.layout.views(m).items():
                t.copy_(loaded[name + '/Adam'])
            for name, t in net.layout.views(v).items():
                t.copy_(loaded[name + '/Adam_1'])
            net.counters[2:3].copy_(loaded['Adam/step'])
        return True
