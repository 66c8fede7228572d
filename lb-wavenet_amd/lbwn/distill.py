"""Knowledge distillation: a student WaveNetTrain trained against a teacher's distribution
(lbwn_train_forward_ex).

The teacher is a second WaveNetTrain of the same batch size with a workspace of its own.  Per slice
its forward runs as a held-out evaluation (lbwn_train_eval) and leaves the raw logits in its plan's
"logits"; the student's head reads them from there while it overwrites its own logits with the
gradient of

    (1-α)·hard + α·τ²·KL(softmax(u/τ) ‖ softmax(l/τ)).

Both calls are enqueued on one stream and nothing synchronises with the host.  The teacher keeps an
evaluation state of its own, SAVE included, so its lookback chains across consecutive slices exactly
as the student's does; that SAVE travels in checkpoints under ``TEACHER/<save var name>``.

Data parallelism reduces nothing new: the gradients and stats[:3] travel as they do without a
teacher, and stats_ex (plain xent, KL) stays rank-local.
"""
import sys
from collections import OrderedDict

import numpy as np
import torch

from .arch import mel_hop_sz, recep_field_sz

TEACHER_PREFIX = 'TEACHER/'


def check_pair(student_arch, teacher_arch, student_batch=None, teacher_batch=None):
    """Raise ValueError unless a net of ``teacher_arch`` can teach one of ``student_arch`` on the same
    (wav, lc, ids) slices."""
    s, t = student_arch, teacher_arch
    if s['n_quant'] != t['n_quant']:
        raise ValueError('distill: n_quant differs (student %d, teacher %d): the two distributions must be over '
                         'the same codes' % (s['n_quant'], t['n_quant']))
    if s['n_lc_out'] > 0 or t['n_lc_out'] > 0:
        if s['n_lc_in'] != t['n_lc_in']:
            raise ValueError('distill: n_lc_in differs (student %d, teacher %d): both nets read the same mel input'
                             % (s['n_lc_in'], t['n_lc_in']))
        hs, ht = mel_hop_sz(s), mel_hop_sz(t)
        if hs != ht:
            raise ValueError('distill: the mel hop differs (student %d, teacher %d): both nets read the same mel '
                             'input' % (hs, ht))
    if t['n_gc_embed'] > 0 and s['n_gc_embed'] > 0 and t['n_gc_category'] < s['n_gc_category']:
        raise ValueError('distill: the teacher has n_gc_category %d, fewer than the student\'s %d: a voice id the '
                         'student takes would index past the teacher\'s table' % (t['n_gc_category'],
                                                                                 s['n_gc_category']))
    if student_batch is not None and student_batch != teacher_batch:
        raise ValueError('distill: batch_sz differs (student %s, teacher %s)' % (student_batch, teacher_batch))


class Distiller:
    """``Distiller(student, teacher, alpha, temp)``: ``step(wav, lc, ids)`` is the student's
    ``forward`` with the teacher's logits of the same slice as soft targets."""

    def __init__(self, student, teacher, alpha=0.5, temp=1.0, label_smoothing=0.0, teacher_flat=None):
        check_pair(student.arch, teacher.arch, student.batch_sz, teacher.batch_sz)
        alpha, temp, eps = float(alpha), float(temp), float(label_smoothing)
        if not 0.0 <= alpha <= 1.0:
            raise ValueError('distill: alpha %r outside [0, 1]' % (alpha,))
        if not (np.isfinite(temp) and temp > 0.0):
            raise ValueError('distill: temp %r must be finite and > 0' % (temp,))
        if not 0.0 <= eps < 1.0:
            raise ValueError('distill: label_smoothing %r outside [0, 1)' % (eps,))
        if student is teacher:
            raise ValueError('distill: the teacher must be a net of its own (its logits may not lie in the '
                             'student\'s workspace)')
        self.student, self.teacher = student, teacher
        self.alpha, self.temp, self.label_smoothing = alpha, temp, eps
        self.teacher_flat = teacher_flat      # None: the teacher's own weights; else e.g. its EMA shadow
        self.state = teacher.eval_state()     # the teacher's own SAVE (zeros), acc, status
        self.teacher_save_vars = OrderedDict(
            (n, self.state['save'][o:o + int(np.prod(s))].view(*s)) for n, (o, s) in teacher.save_index.items())

    def recep_field_sz(self):
        """The larger of the two receptive fields: the dataset's invalid-window mask then covers both."""
        return max(recep_field_sz(self.student.arch), recep_field_sz(self.teacher.arch))

    def step(self, wav_input, lc_input, id_mask, backward=True, stream=None, want_dmel=False):
        """The teacher's forward of the slice, then the student's forward (and backward) against it, on
        one stream with no host synchronisation.  Returns the student's stats; ``student.stats_ex`` holds
        (Σ plain xent, Σ KL, 0, 0)."""
        t, s = self.teacher, self.student
        t.eval_slice(self.state, wav_input, lc_input if t.use_lc_input() else None, id_mask,
                     flat=self.teacher_flat, stream=stream)
        # one slice's inputs are enough to keep alive: the stream orders the next call behind this one
        del self.state['keep'][:-1]
        T = int(np.shape(wav_input)[1])
        return s.forward(wav_input, lc_input if s.use_lc_input() else None, id_mask, backward=backward,
                         stream=stream, want_dmel=want_dmel, teacher_logits=t.logits_view(T),
                         distill_alpha=self.alpha, distill_temp=self.temp, label_smoothing=self.label_smoothing)

    def teacher_status(self):
        """The teacher's accumulated chain status word (synchronises); 0 = ok."""
        return int(self.state['status'].item())

    # ---- checkpoints -------------------------------------------------------------------------
    def state_tensors(self):
        """The teacher's SAVE under ``TEACHER/<save var name>``.  Data-parallel: a collective; the
        ranks' rows are gathered into the SAVE of the global batch, as WaveNetTrain.save does."""
        dp = getattr(self.student, 'dp', None)
        if dp is not None and dp.enabled:
            import torch.distributed as dist
            parts = [torch.empty_like(self.state['save']) for _ in range(dp.world)]
            dist.all_gather(parts, self.state['save'])
            return OrderedDict((TEACHER_PREFIX + n, torch.cat([p[o:o + int(np.prod(s))].view(*s) for p in parts], 0))
                               for n, (o, s) in self.teacher.save_index.items())
        return OrderedDict((TEACHER_PREFIX + n, v) for n, v in self.teacher_save_vars.items())

    def load_state_tensors(self, loaded, log=None):
        """Restore the teacher's SAVE from a checkpoint's tensors.  A checkpoint without the keys (one
        written without a teacher) loads zeros and prints one warning; returns whether it had them."""
        keys = [TEACHER_PREFIX + n for n in self.teacher_save_vars]
        have = [k in loaded for k in keys]
        with torch.no_grad():
            if not all(have):
                print('Warning: the checkpoint has no {}* state ({} of {} keys): the teacher\'s lookback starts '
                      'from zeros'.format(TEACHER_PREFIX, sum(have), len(keys)), file=log or sys.stderr)
                self.state['save'].zero_()
                return False
            dp = getattr(self.student, 'dp', None)
            rows = dp.rows(self.teacher.batch_sz) if dp is not None and dp.enabled else slice(None)
            for k, dst in zip(keys, self.teacher_save_vars.values()):
                src = loaded[k][rows]
                if tuple(src.shape) != tuple(dst.shape):
                    raise ValueError('checkpoint: %s has shape %s, the teacher expects %s'
                                     % (k, tuple(src.shape), tuple(dst.shape)))
                dst.copy_(src.to(dst.dtype))
        return True
