"""WaveNetTrain — drop-in for tmodel.WaveNetTrain (tmodel.py:6-358) on MI355X.

Same constructor arguments and methods as the reference; the TF graph is replaced by an
lbwn plan (liblbwn.so) that runs the whole forward/loss/backward as a fixed sequence of
HIP launches on the current torch stream.  The reference's TF-eager flow (train.py:219-222)

    grads_and_vars, loss = net.build(wav_input, mel_input, id_mask)
    optimizer.apply_gradients(grads_and_vars)

is reproduced literally (lbwn.optim.AdamOptimizer).
"""
import contextlib
import ctypes
import sys
from collections import OrderedDict

import numpy as np
import torch

from . import _lib
from .ckpt import Checkpoint
from .arch import ParamLayout, layer_iter, n_layers, recep_field_sz, save_layout, xavier_limit


def _i32(x, dev):
    if isinstance(x, torch.Tensor):
        return x.to(device=dev, dtype=torch.int32).contiguous()
    return torch.as_tensor(np.asarray(x), dtype=torch.int32, device=dev).contiguous()


class GradsAndVars(list):
    """list of (grad view, serial name) like TF's compute_gradients output; carries the
    flat buffers so the optimizer applies one fused update."""

    def __init__(self, net, pairs):
        super().__init__(pairs)
        self.net = net


class WaveNetTrain:
    def __init__(self, n_blocks, n_block_layers, n_quant, n_res, n_dil, n_skip, n_post, n_gc_embed,
                 n_gc_category, n_lc_in, n_lc_out, lc_upsample, use_bias, wav_input_type, batch_sz,
                 l2_factor, add_summary=False, n_keep_checkpoints=10, ckpt_path=None, resume_step=0,
                 n_valid_total=0, sess=None, print_interval=10, device='cuda', seed=0):
        self.arch = dict(n_blocks=n_blocks, n_block_layers=n_block_layers, n_quant=n_quant, n_res=n_res,
                         n_dil=n_dil, n_skip=n_skip, n_post=n_post, n_gc_embed=n_gc_embed,
                         n_gc_category=n_gc_category, n_lc_in=n_lc_in, n_lc_out=n_lc_out,
                         lc_upsample=list(lc_upsample), use_bias=bool(use_bias), wav_input_type=wav_input_type)
        for k, v in self.arch.items():
            setattr(self, k, v)
        self.batch_sz = batch_sz
        self.l2_factor = float(l2_factor)
        self.add_summary = add_summary
        self.n_keep_checkpoints = n_keep_checkpoints
        self.ckpt_path = ckpt_path
        self.resume_step = resume_step
        self.n_valid_total = n_valid_total
        self.print_interval = print_interval
        self.dp = None      # lbwn.dist.DPContext when training data-parallel (set by train.py)
        self.device = torch.device(device)
        self.lib = _lib.load()
        self.layout = ParamLayout(self.arch)
        self.save_index, n_save = save_layout(self.arch, batch_sz)
        dev = self.device
        self.flat = torch.zeros(self.layout.n_total, dtype=torch.float32, device=dev)
        self.grad_flat = torch.zeros_like(self.flat)
        self.save_flat = torch.zeros(n_save, dtype=torch.float32, device=dev)
        self.stats = torch.zeros(4, dtype=torch.float32, device=dev)
        self.counters = torch.zeros(4, dtype=torch.int64, device=dev)   # GLOBAL_STEP, VALID_SAMPLES, adam t-1, status
        self.vars = self.layout.views(self.flat)
        self.grads = self.layout.views(self.grad_flat)
        self.save_vars = OrderedDict((n, self.save_flat[o:o + int(np.prod(s))].view(*s))
                                     for n, (o, s) in self.save_index.items())
        self._arch_c = self._make_arch_struct()
        self._params_c = self._make_params_struct(self.flat)
        self._grads_c = self._make_params_struct(self.grad_flat)
        self._plans = {}
        self._ws = None
        self._last = None
        self._sp_cache = None
        self._dmel = {}     # slice length -> the dmel buffer of forward(want_dmel=True)
        self.dmel = None
        self._stats_ex = None   # allocated by the first forward with distillation or label smoothing
        self.stats_ex = None
        self._local_nv = None
        self._teacher = None
        self.init_vars(seed)
        # host mirror of GLOBAL_STEP: counts the optimizer calls (attempted steps) so the print
        # cadence needs no sync; re-read from counters[0] by check_status, since a step skipped
        # on the device (chain timeout) does not advance GLOBAL_STEP
        self.global_step_host = 0
        # checkpoint surface (ckpt.py:13-81; the saveables are self.vars, tmodel.py:330)
        self.ckpt = Checkpoint(ckpt_path, n_keep_checkpoints, resume_step)
        self.ckpt.add_saveable_objects(self.state_tensors())

    # ---- reference API -------------------------------------------------------------------
    def get_recep_field_sz(self):
        return recep_field_sz(self.arch)

    def has_global_cond(self):
        return self.n_gc_embed > 0

    def use_lc_input(self):
        return self.n_lc_out > 0

    def init_vars(self, seed=0, bias_scale=0.0):
        """Xavier-uniform weights (arch.py:63), zero biases (arch.py:64), Xavier SAVE
        (tmodel.py:123-124 passes no initializer)."""
        g = torch.Generator(device='cpu').manual_seed(seed)
        with torch.no_grad():
            for name, e in self.layout.entries.items():
                if e.is_bias:
                    if bias_scale:
                        v = (torch.rand(e.shape, generator=g) * 2 - 1) * bias_scale
                    else:
                        v = torch.zeros(e.shape)
                else:
                    lim = xavier_limit(e.shape)
                    v = (torch.rand(e.shape, generator=g) * 2 - 1) * lim
                self.vars[name].copy_(v)
            for name, t in self.save_vars.items():
                lim = xavier_limit(list(t.shape))
                t.copy_((torch.rand(t.shape, generator=g) * 2 - 1) * lim)
        self.counters.zero_()

    def build(self, wav_input, lc_input, id_mask):
        """Forward + loss + backward of one slice (tmodel.py:292-340).  Returns
        (grads_and_vars, loss) with loss a 0-d device tensor (total = mean xent + l2)."""
        self.forward(wav_input, lc_input, id_mask, backward=True)
        gv = GradsAndVars(self, [(self.grads[n], n) for n in self.layout.names()])
        return gv, self.total_loss()

    # ---- engine ------------------------------------------------------------------------------
    def _make_arch_struct(self):
        a = _lib.Arch()
        for k in ('n_blocks', 'n_block_layers', 'n_quant', 'n_res', 'n_dil', 'n_skip', 'n_post',
                  'n_gc_embed', 'n_gc_category', 'n_lc_in', 'n_lc_out'):
            setattr(a, k, int(self.arch[k]))
        ups = self.arch['lc_upsample'] if self.arch['n_lc_out'] > 0 else []
        a.n_lc_upsample = len(ups)
        for i, s in enumerate(ups):
            a.lc_upsample[i] = int(s)
        a.use_bias = int(self.arch['use_bias'])
        return a

    def _make_params_struct(self, flat):
        P = _lib.Params()
        base = flat.data_ptr()
        kb = self.layout.kind_base
        for field in ('pre', 'pre_b', 'sig', 'sig_b', 'gate', 'gate_b', 'res', 'res_b', 'skip', 'skip_b',
                      'gc_embed', 'gc_sig', 'gc_gate', 'lc_sig', 'lc_gate', 'post1', 'post1_b', 'post2',
                      'post2_b'):
            setattr(P, field, base + 4 * kb[field] if field in kb else None)
        for i in range(8):
            k = 'lc_up%d' % i
            P.lc_up[i] = base + 4 * kb[k] if k in kb else None
        return P

    def _plan(self, T):
        if T not in self._plans:
            h = ctypes.c_void_p()
            _lib.check(self.lib.lbwn_plan_create(ctypes.byref(self._arch_c), self.batch_sz, T, ctypes.byref(h)))
            nbytes = self.lib.lbwn_plan_workspace_bytes(h)
            self._plans[T] = (h, nbytes)
        h, nbytes = self._plans[T]
        if self._ws is None or self._ws.numel() < nbytes:
            # zeroed once, at allocation: the padding rows that plan_tensor reports but no launch writes
            # (e.g. "dz" in whole 32-row blocks) are then defined, not whatever the allocator handed back
            self._ws = torch.zeros(nbytes, dtype=torch.uint8, device=self.device)
        return h

    def plan_tensor(self, T, name):
        """fp32 view of a named plan workspace tensor (debug/parity)."""
        h = self._plan(T)
        off, nb = _lib.c_size_t(), _lib.c_size_t()
        _lib.check(self.lib.lbwn_plan_tensor(h, name.encode(), ctypes.byref(off), ctypes.byref(nb)))
        return self._ws[off.value:off.value + nb.value].view(torch.float32)

    def plan_info(self, T, key):
        """A dispatch fact of the plan (lbwn_plan_info: 'up_fused', 'split_dlcx', 'dlc_parts', ...)."""
        v = _lib.c_int64()
        _lib.check(self.lib.lbwn_plan_info(self._plan(T), key.encode(), ctypes.byref(v)))
        return v.value

    def workspace_bytes(self, T):
        self._plan(T)
        return self._plans[T][1]

    def logits_view(self, T):
        """Torch view [B·T, n_quant] of the plan's "logits" at slice length T: the raw logits after
        ``eval_slice``, the dlogits after ``forward``.  A view of the workspace: valid until the plan's
        next call on it."""
        return self.plan_tensor(T, 'logits').view(self.batch_sz * T, self.n_quant)

    def forward(self, wav_input, lc_input, id_mask, backward=True, stream=None, want_dmel=False,
                teacher_logits=None, distill_alpha=0.0, distill_temp=1.0, label_smoothing=0.0):
        """Run the plan on one slice; wav_input int [B,T] mu-law codes (raw floats are
        mu_encode'd first when wav_input_type == 'raw', tmodel.py:58-62).  want_dmel: the backward
        goes through lbwn_train_backward_ex and leaves in ``self.dmel`` the gradient of Σ masked xent
        (a raw sum, like grad_flat) with respect to lc_input, a device tensor [B, T/hop, n_lc_in]: one
        buffer per slice length, valid until the next forward.

        Distillation and label smoothing (lbwn_train_forward_ex): ``teacher_logits`` is a
        device fp32 tensor [B·T, >= n_quant] or [B, T, n_quant] whose row stride becomes ld_teacher
        (it must not be this net's own workspace), ``distill_alpha`` the weight of the soft term,
        ``distill_temp`` its temperature, ``label_smoothing`` ε.  stats[0] is then Σ of the objective,
        and ``self.stats_ex`` a device fp32[4]: (Σ plain xent, Σ KL, 0, 0), rank-local under data
        parallelism.  With distill_alpha == 0 and label_smoothing == 0 the call is
        lbwn_train_forward's and ``self.stats_ex`` is None: stats[0] is the plain xent."""
        dev = self.device
        alpha, temp, eps = float(distill_alpha), float(distill_temp), float(label_smoothing)
        if not 0.0 <= alpha <= 1.0:
            raise ValueError('distill_alpha %r outside [0, 1]' % (distill_alpha,))
        if not (np.isfinite(temp) and temp > 0.0):
            raise ValueError('distill_temp %r must be finite and > 0' % (distill_temp,))
        if not 0.0 <= eps < 1.0:
            raise ValueError('label_smoothing %r outside [0, 1)' % (label_smoothing,))
        if alpha > 0.0 and teacher_logits is None:
            raise ValueError('distill_alpha > 0 needs teacher_logits')
        if want_dmel and not self.use_lc_input():
            raise ValueError('want_dmel: this arch has no local conditioning (n_lc_out == 0)')
        if want_dmel and not backward:
            raise ValueError('want_dmel needs backward=True: dmel is an output of the backward')
        if self.wav_input_type == 'raw':
            from .ops import mu_encode
            wav_input = mu_encode(torch.as_tensor(wav_input, dtype=torch.float32, device=dev), self.n_quant)
        q = _i32(wav_input, dev)
        ids = _i32(id_mask, dev)
        B, T = q.shape
        if B != self.batch_sz:
            raise ValueError('batch %d != batch_sz %d' % (B, self.batch_sz))
        mel = None
        if self.use_lc_input():
            mel = torch.as_tensor(lc_input, dtype=torch.float32, device=dev).contiguous()
        h = self._plan(T)
        sp = _lib.stream_ptr(stream)
        self._last = (q, ids, mel)   # keep inputs alive until the stream consumed them
        self._teacher = None
        if alpha == 0.0 and eps == 0.0:
            self.stats_ex = None
            _lib.check(self.lib.lbwn_train_forward(h, ctypes.byref(self._params_c), self._ws.data_ptr(), q.data_ptr(),
                                                   ids.data_ptr(), _lib.ptr(mel), self.save_flat.data_ptr(),
                                                   self.stats.data_ptr(), sp))
        else:
            tl, ld = None, 0
            if alpha > 0.0:
                tl = teacher_logits
                if not (isinstance(tl, torch.Tensor) and tl.dtype == torch.float32 and tl.device == self.flat.device):
                    raise ValueError('teacher_logits must be an fp32 tensor on the model device')
                if tl.dim() == 3:
                    if tuple(tl.shape) != (B, T, self.n_quant) or not tl.is_contiguous():
                        raise ValueError('teacher_logits [B, T, Q] must be contiguous %s, got %s'
                                         % ((B, T, self.n_quant), tuple(tl.shape)))
                    tl = tl.view(B * T, self.n_quant)
                if tl.dim() != 2 or tl.shape[0] != B * T or tl.shape[1] < self.n_quant or tl.stride(1) != 1:
                    raise ValueError('teacher_logits must be [B·T, >= n_quant] with unit column stride, got %s'
                                     % (tuple(tl.shape),))
                ld = tl.stride(0)
            if self._stats_ex is None:
                self._stats_ex = torch.zeros(4, dtype=torch.float32, device=dev)
            self.stats_ex = self._stats_ex
            self._teacher = tl          # kept alive with the inputs; None: label smoothing alone
            a = _lib.ForwardArgs(wav_q=q.data_ptr(), ids=ids.data_ptr(), mel=_lib.ptr(mel),
                                 save=self.save_flat.data_ptr(), stats=self.stats.data_ptr(),
                                 stats_ex=self.stats_ex.data_ptr(), teacher_logits=_lib.ptr(tl), ld_teacher=ld,
                                 distill_alpha=alpha, distill_temp=temp, label_smoothing=eps)
            _lib.check(self.lib.lbwn_train_forward_ex(h, ctypes.byref(self._params_c), self._ws.data_ptr(),
                                                      ctypes.byref(a), sp))
            # this rank's own count beside its own stats_ex (stats[1] is summed over ranks later)
            self._local_nv = None
            if self.dp is not None and self.dp.enabled:
                with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
                    self._local_nv = self.stats[1].clone()
        self.dmel = None
        if backward and want_dmel:
            shape = (B, T // int(np.prod(self.lc_upsample)), self.n_lc_in)
            if tuple(mel.shape) != shape:
                raise ValueError('want_dmel: lc_input must be %s, got %s' % (shape, tuple(mel.shape)))
            if T not in self._dmel:
                self._dmel[T] = torch.empty(shape, dtype=torch.float32, device=dev)
            self.dmel = self._dmel[T]
            a = _lib.BackwardArgs(wav_q=q.data_ptr(), ids=ids.data_ptr(), mel=mel.data_ptr(),
                                  dmel=self.dmel.data_ptr())
            _lib.check(self.lib.lbwn_train_backward_ex(h, ctypes.byref(self._params_c), ctypes.byref(self._grads_c),
                                                       self._ws.data_ptr(), ctypes.byref(a), sp))
        elif backward:
            _lib.check(self.lib.lbwn_train_backward(h, ctypes.byref(self._params_c), ctypes.byref(self._grads_c),
                                                    self._ws.data_ptr(), q.data_ptr(), ids.data_ptr(),
                                                    _lib.ptr(mel), sp))
        return self.stats

    # ---- held-out evaluation (lbwn_train_eval) ---------------------------------
    def eval_state(self, n_bins=None):
        """The buffers one evaluation owns: a zero SAVE (its own D-sep state, never the training
        run's), acc double[4], by_voice double[n_bins][2] when ``n_bins`` is given, the status word,
        and the scratch, sized per slice length on first use."""
        dev = self.device
        return dict(save=torch.zeros_like(self.save_flat), acc=torch.zeros(4, dtype=torch.float64, device=dev),
                    by_voice=(torch.zeros(int(n_bins), 2, dtype=torch.float64, device=dev)
                              if n_bins is not None else None),
                    n_bins=int(n_bins) if n_bins is not None else 0,
                    status=torch.zeros(1, dtype=torch.int32, device=dev), scratch=None, keep=[])

    def eval_slice(self, state, wav_input, lc_input, id_mask, flat=None, nll=None, stream=None):
        """One lbwn_train_eval on a slice: adds to ``state`` (acc, by_voice, status) and advances its
        SAVE.  ``nll``: an fp32 [B, >= T] device tensor to receive the per-position values.  No
        synchronisation; the training run's save_flat, stats and counters are not touched."""
        dev = self.device
        if self.wav_input_type == 'raw':
            from .ops import mu_encode
            wav_input = mu_encode(torch.as_tensor(wav_input, dtype=torch.float32, device=dev), self.n_quant)
        q = _i32(wav_input, dev)
        ids = _i32(id_mask, dev)
        B, T = q.shape
        if B != self.batch_sz:
            raise ValueError('batch %d != batch_sz %d' % (B, self.batch_sz))
        mel = None
        if self.use_lc_input():
            mel = torch.as_tensor(lc_input, dtype=torch.float32, device=dev).contiguous()
        h = self._plan(T)
        need = self.lib.lbwn_train_eval_scratch_bytes(h, state['n_bins'])
        if state['scratch'] is None or state['scratch'].numel() < need:
            state['scratch'] = torch.empty(need, dtype=torch.uint8, device=dev)
        params = self._params_c if flat is None else self._make_params_struct(flat)
        a = _lib.EvalArgs(wav_q=q.data_ptr(), ids=ids.data_ptr(), mel=_lib.ptr(mel), save=state['save'].data_ptr(),
                          acc=state['acc'].data_ptr(), nll=_lib.ptr(nll), ld_nll=nll.stride(0) if nll is not None else 0,
                          by_voice=_lib.ptr(state['by_voice']), n_bins=state['n_bins'],
                          status=state['status'].data_ptr(), scratch=state['scratch'].data_ptr())
        state['keep'].append((q, ids, mel))   # inputs stay alive until the evaluation's synchronisation
        _lib.check(self.lib.lbwn_train_eval(h, ctypes.byref(params), self._ws.data_ptr(), ctypes.byref(a),
                                            _lib.stream_ptr(stream)))

    def evaluate(self, batches, state=None, flat=None, want_nll=False):
        """Held-out loss over an iterator of ``(cnt, wav, mel, ids)`` (lbwn.data.eval_batches): one
        lbwn_train_eval per slice through one state, one synchronisation at the end.  ``flat``
        selects another parameter buffer of the layout (the optimizer's EMA shadow); a ``state``
        made with ``eval_state(n_bins)`` adds the per-voice split.  A state accumulates: the result
        covers everything evaluated into it since eval_state().  Under data parallelism each rank
        evaluates its rows of the same global deal and the sums are all-reduced once, into copies (the
        state keeps the rank's own sums, so it stays reusable).  Returns
        nll (mean, nats), bits (nll / ln 2), top1 (share with argmax == target), avg_diff (mean
        |argmax - target|), n (scored positions), by_voice ([n_bins, 2]: sum, count) when the state has
        bins, and with ``want_nll`` nll_rows (one fp32 [B, T] device tensor per slice).  Raises on a
        nonzero status word."""
        state = state if state is not None else self.eval_state()
        if flat is not None and (flat.numel() != self.flat.numel() or flat.dtype != torch.float32
                                 or flat.device != self.flat.device):
            raise ValueError('flat must be an fp32 buffer of the parameter layout on the model device')
        rows = []
        for _, wav, mel, ids in batches:
            out = None
            if want_nll:
                out = torch.zeros(np.shape(wav)[0], np.shape(wav)[1], dtype=torch.float32, device=self.device)
                rows.append(out)
            self.eval_slice(state, wav, mel, ids, flat=flat, nll=out)
        acc, by_voice, status = state['acc'], state['by_voice'], state['status']
        if self.dp is not None and self.dp.enabled:
            # the global sums go into copies: the state keeps this rank's own, so it can be evaluated into again
            acc, status = acc.clone(), status.clone()
            by_voice = by_voice.clone() if by_voice is not None else None
            self.dp.reduce_eval(acc, by_voice, status)
        if self.device.type == 'cuda':
            torch.cuda.synchronize(self.device)
        state['keep'].clear()
        st = int(status.item())
        if st:
            raise RuntimeError('lbwn: chain hand-off timed out during evaluation (status word %#x)' % st)
        s, n, d, hit = acc.tolist()
        mean = s / n if n else 0.0
        res = dict(nll=mean, bits=mean / float(np.log(2.0)), top1=hit / n if n else 0.0,
                   avg_diff=d / n if n else 0.0, n=int(n))
        if by_voice is not None:
            res['by_voice'] = by_voice.cpu().numpy()
        if want_nll:
            res['nll_rows'] = rows
        return res

    def status_word(self, T=None):
        """int32 view of the plan's per-step status word (zeroed at each forward; the chains
        OR their timeout codes in: bit 0 forward chain, bit 1 backward chain)."""
        T = T if T is not None else self._last[0].shape[1]
        return self.plan_tensor(T, 'status')[:1].view(torch.int32)

    def status_ptr(self):
        """Device pointer of the last step's status word (None before any step)."""
        if self._last is None:
            return None
        key = (self._last[0].shape[1], self._ws.data_ptr())
        if self._sp_cache is None or self._sp_cache[0] != key:
            self._sp_cache = (key, self.status_word().data_ptr())
        return self._sp_cache[1]

    def wait_point(self, point, stream):
        """Make a torch stream wait for a point of the last backward (lbwn_plan_stream_wait);
        False if the plan has no such point."""
        if self._last is None:
            return False
        waited = ctypes.c_int(0)
        _lib.check(self.lib.lbwn_plan_stream_wait(self._plan(self._last[0].shape[1]), point.encode(),
                                                  stream.cuda_stream, ctypes.byref(waited)))
        return bool(waited.value)

    def status(self, T=None):
        """Cumulative status (synchronises): every applied step's status word is ORed into
        counters[3] by the optimizer kernel (which skips a failed step's update on the
        device), plus the current step's word for a step not yet applied.  0 = ok; bit 0 = a
        forward-chain hand-off timed out, bit 1 = a backward-chain one."""
        return int(self.counters[3].item()) | int(self.status_word(T).item())

    def check_status(self, T=None):
        st = self.status(T)
        self.global_step_host = int(self.counters[0].item())
        if st:
            raise RuntimeError('lbwn: chain hand-off timed out (status word %#x): the failed steps were '
                               'not applied' % st)

    def l2_loss(self):
        """tmodel.py:250-261: Σ_{trainable, non-BIAS} Σv²/2 (the weight region of the flat buffer)."""
        w = self.flat[:self.layout.n_weights]
        return 0.5 * torch.dot(w, w)

    def total_loss(self):
        nv = self.stats[1]
        mean = torch.where(nv > 0, self.stats[0] / torch.clamp(nv, min=1.0), torch.zeros_like(nv))
        return mean + self.l2_factor * self.l2_loss()

    def progress_line(self):
        """tmodel.py:263-267 columns: step, total, mean xent, l2, avg_diff, n_valid,
        n_valid_cumul, n_valid_total, %."""
        st = self.stats.tolist()
        cnt = self.counters.tolist()
        nv = int(st[1])
        mean = st[0] / nv if nv else 0.0
        l2 = float(self.l2_loss())
        total = mean + self.l2_factor * l2
        B, T = self._last[0].shape
        world = self.dp.world if self.dp is not None else 1     # stats[2] is summed over ranks
        avg_diff = int(st[2]) // (world * B * (T - 1))
        pct = cnt[1] * 100.0 / self.n_valid_total if self.n_valid_total else 0.0
        line = ('{:5d}\t{:8.4f}\t{:8.4f}\t{:7.2f}\t{:5.0f}\t{:5.0f}\t{:10d}\t{:14d}\t{:5.2f}'.format(
            cnt[0], total, mean, l2, avg_diff, nv, cnt[1], int(self.n_valid_total), pct))
        if self.stats_ex is not None and self._teacher is not None:
            # distilling: total and mean above are the objective; the plain xent and the KL follow
            # (this rank's own sums over this rank's own count: stats_ex is not reduced)
            ex = self.stats_ex.tolist()
            nloc = int(self._local_nv.item()) if self._local_nv is not None else nv
            line += '\t{:8.4f}\t{:8.4f}'.format(ex[0] / nloc if nloc else 0.0, ex[1] / nloc if nloc else 0.0)
        return line

    def maybe_print(self, file=None):
        """The in-graph progress print (tmodel.py:272-281): every print_interval steps,
        BEFORE the counters advance.  Uses the host mirror of GLOBAL_STEP, so steps that do
        not print never synchronise with the device."""
        if self.print_interval and self.global_step_host % self.print_interval == 0:
            print(self.progress_line(), file=file or sys.stderr)

    # ---- checkpoints (ckpt.py:53-81) --------------------------------------------------------
    def save(self, step, optimizer=None, more=None):
        """Write '<ckpt_path>-<step>.safetensors'; with ``optimizer`` its Adam slots too, and the
        tensors of ``more`` (e.g. Distiller.state_tensors()) as they are.
        Data-parallel: a collective (every rank calls it).  The weights are replicated, but
        SAVE is per stream, so the ranks' rows are gathered and rank 0 writes the SAVE of
        the GLOBAL batch [world·B, d, Cr] -- the same file a single process over world·B
        streams writes; the other ranks return None."""
        if self.device.type == 'cuda':
            torch.cuda.synchronize(self.device)
        extra = dict(optimizer.state_tensors(self)) if optimizer is not None else {}
        if more:
            extra.update(more)
        if self.dp is not None and self.dp.enabled:
            extra.update(self._gather_save())
            if self.dp.rank != 0:
                return None
        return self.ckpt.save(step, extra)

    def _gather_save(self):
        import torch.distributed as dist
        parts = [torch.empty_like(self.save_flat) for _ in range(self.dp.world)]
        dist.all_gather(parts, self.save_flat)
        return OrderedDict((n, torch.cat([p[o:o + int(np.prod(s))].view(*s) for p in parts], 0))
                           for n, (o, s) in self.save_index.items())

    def restore(self, optimizer=None):
        """Load '<ckpt_path>-<resume_step>' into the live buffers (ckpt.py:63-81).  Under
        data parallelism each rank takes its own rows of the global-batch SAVE."""
        select = None
        if self.dp is not None and self.dp.enabled:
            rows = self.dp.rows(self.batch_sz)
            select = lambda name, t: t[rows] if name in self.save_vars else t   # noqa: E731
        loaded = self.ckpt.restore(select)
        if optimizer is not None:
            optimizer.load_state_tensors(self, loaded)
        self.global_step_host = int(self.counters[0])
        return loaded

    # ---- state dicts (checkpoint surface, names as arch.py:142) ----------------------------
    def state_tensors(self):
        out = OrderedDict(self.vars)
        out.update(self.save_vars)
        out['GLOBAL_STEP'] = self.counters[0:1]
        out['VALID_SAMPLES'] = self.counters[1:2]
        return out
