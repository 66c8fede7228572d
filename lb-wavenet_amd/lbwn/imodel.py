"""WaveNetGen — drop-in for imodel.WaveNetGen (imodel.py:7-303) on MI355X.

Same constructor arguments as the reference (imodel.py:9-23: n_blocks, n_block_layers,
n_quant, n_res, n_dil, n_skip, n_post1, n_gc_embed, n_gc_category, use_bias, batch_sz,
chunk_sz, teacher_vec).  The TF while_loop becomes lbwn_gen_run: the whole step is HIP
kernels with device-resident state, optionally captured as a hipGraph of ``chunk_sz``
steps and replayed.  The reference's generation path does not run as shipped;
this class implements its stated intent (tests.py:1: tmodel and imodel are equivalent
functions), adding PRE_BIAS to the input embedding by default (``pre_bias=False``
reproduces imodel.py:75-77 literally).

Local conditioning (keyword-only ``n_lc_in, n_lc_out, lc_upsample``; the reference's generator
has no LC path): ``init_buffers`` / ``run`` take ``mel`` [B, n_frames, n_lc_in] (or [n_frames,
n_lc_in], shared by every stream).  Generation step i is training position i-1, so it is
conditioned on row max(i-1, 0) of the upsampled mel; n_frames·hop rows cover n_frames·hop + 1 steps.

Prompt prefill: ``prefill(codes)`` advances every stream by n known inputs in one parallel pass
(lbwn_gen_prefill) instead of n steps; ``run(gen_sz, prefill=True)`` primes with the teacher vector
that way.  On an LC arch the prefilled steps are conditioned on the loaded mel like any other step
(``init_buffers(mel=...)`` first, or ``run(gen_sz, mel=..., prefill=True)``).  The default teacher
path is unchanged.

Scoring: ``score(codes)`` is the same parallel pass with the head run over every position
(lbwn_gen_score): it returns log p(codes[b, j] | history) as float32 [batch_sz, n], advances the state
as ``prefill(codes)`` does and leaves the last scored step's ``logits()``.

Sampling (keyword-only ``temperature=1.0, top_k=0, top_p=1.0``, or ``set_sampling`` later): the draw of
every step is filtered as lbwn_gen_set_sampling defines -- top_k keeps the codes whose logit is >= the
k-th largest (ties kept, 0 = off, >= n_quant = off), the kept codes get e = exp((l - max l) / T), top_p
then keeps the shortest descending-e prefix with mass >= p·Σe (ties with its last member kept), and the
inverse-CDF draw runs over the surviving e in code order.  ``top_k=1`` is greedy decoding; the neutral
(1, 0, 1) is the unfiltered draw, bit for bit.  "logits" stays raw.

State (lbwn_gen_state_save / _load): ``save_state()`` returns a ``GenState`` -- the rings, the
pending codes and the step of every stream, stream-major, so it loads into a plan of another batch size;
``load_state(state, streams)`` gives stream b the record ``streams[b]``; ``fork(src)`` is both at once.
``run(gen_sz, prefill='fanout')`` prefills the teacher once per distinct voice id in a private generator
and loads that state into every stream of the voice.

Sessions (lbwn_gen_begin): ``begin(slots, mels, gc_ids, keys)`` restarts single streams between
two ``step`` calls -- zero rings, the stream's own mel, voice id, draw key and step origin -- while the others
continue; ``take(slot, n)`` is a session's first n samples of "wav".  ``vocode(mels)`` turns a list of mels of
different lengths into one wav each, recycling a stream as soon as its utterance is covered (the schedule of
``plan_sessions``); with the default keys (the utterance indices) the result does not depend on batch_sz or
on the schedule.

Ring plans (keyword-only ``ring_steps=R``; lbwn_gen_plan_create_ex): "samples" / "wav" hold the last
R local steps of every stream and "lc" a ring of ceil(R/hop)·hop rows, so the workspace does not grow with the
run.  ``extend(slots, mels)`` feeds a live session more frames, ``collect(slot, i0, n)`` copies local steps out
of the rings, ``take`` returns a collected copy; ``vocode`` runs the schedule of ``plan_ring`` and
``vocode_iter(iterable)`` yields (index, wav) as utterances finish, endlessly if the iterable is.  Prefill,
score and a teacher vector are refused on a ring plan.
"""
import ctypes
import math
import sys

import numpy as np
import torch

from . import _lib
from .arch import ParamLayout, mel_hop_sz, normalize_arch


STATE_MAGIC = 0x5453424c      # "LBST" (include/lbwn.h, lbwn_gen_state_save)
STATE_VERSION = 1
STATE_HEADER = 256
STATE_DIMS = ('n_blocks', 'n_block_layers', 'n_res', 'n_quant')


def state_record_bytes(n_blocks, n_block_layers, n_res):
    """Bytes of one stream's record: the pending code (16 bytes) and its rings, rounded up to 16."""
    return (16 + 4 * n_blocks * (2 ** n_block_layers - 1) * n_res + 15) // 16 * 16


def parse_state_header(raw):
    """The 256 header bytes (uint8 array) of a snapshot -> dict(n_streams, n_blocks, n_block_layers, n_res,
    n_quant, record_bytes, step); ValueError when they are not a version-1 header."""
    raw = np.ascontiguousarray(np.asarray(raw, np.uint8).reshape(-1)[:STATE_HEADER])
    if raw.size < STATE_HEADER:
        raise ValueError('state: %d bytes are shorter than the %d-byte header' % (raw.size, STATE_HEADER))
    w = raw[:32].view('<i4')
    if int(w[0]) != STATE_MAGIC:
        raise ValueError('state: bad magic 0x%08x (want 0x%08x)' % (int(w[0]) & 0xffffffff, STATE_MAGIC))
    if int(w[1]) != STATE_VERSION:
        raise ValueError('state: layout version %d, this build reads %d' % (int(w[1]), STATE_VERSION))
    h = dict(zip(('n_streams',) + STATE_DIMS + ('record_bytes',), (int(v) for v in w[2:8])))
    h['step'] = int(raw[32:40].view('<i8')[0])
    if h['n_streams'] < 1 or h['record_bytes'] != state_record_bytes(h['n_blocks'], h['n_block_layers'], h['n_res']):
        raise ValueError('state: inconsistent header %r' % (h,))
    return h


def plan_sessions(lengths, batch_sz, chunk):
    """The schedule ``WaveNetGen.vocode`` runs: utterances of ``lengths[u]`` steps dealt to ``batch_sz``
    slots first in, first out, a slot taking the next utterance at the first chunk boundary after its
    own is covered.  Returns (rounds, total): each round is (steps to run, [(slot, utterance), ...] to
    begin before them), total the sum of the steps -- what the plan's max_steps must hold.  While
    utterances wait a round runs a whole ``chunk``; once none waits, min(chunk, the longest remainder).
    Pure host arithmetic."""
    lens = [int(n) for n in lengths]
    if isinstance(batch_sz, bool) or not isinstance(batch_sz, (int, np.integer)) or batch_sz < 1:
        raise ValueError('plan_sessions: batch_sz must be an integer >= 1, got %r' % (batch_sz,))
    if isinstance(chunk, bool) or not isinstance(chunk, (int, np.integer)) or chunk < 1:
        raise ValueError('plan_sessions: chunk must be an integer >= 1, got %r' % (chunk,))
    for u, n in enumerate(lens):
        if n < 1:
            raise ValueError('plan_sessions: lengths[%d] = %d must be >= 1' % (u, n))
    left = [0] * int(batch_sz)      # steps each slot's session still needs
    rounds, total, nxt = [], 0, 0
    while True:
        begins = []
        for slot in range(int(batch_sz)):
            if left[slot] <= 0 and nxt < len(lens):
                begins.append((slot, nxt))
                left[slot] = lens[nxt]
                nxt += 1
        need = max(left)
        if need <= 0:
            break
        steps = int(chunk) if nxt < len(lens) else min(int(chunk), need)
        rounds.append((steps, begins))
        total += steps
        left = [r - steps for r in left]
    return rounds, total


def _check_ring_args(batch_sz, chunk, ring_steps, hop):
    for name, v in (('batch_sz', batch_sz), ('chunk', chunk), ('ring_steps', ring_steps), ('hop', hop)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1:
            raise ValueError('plan_ring: %s must be an integer >= 1, got %r' % (name, v))
    if chunk > ring_steps:
        raise ValueError('plan_ring: chunk = %d exceeds ring_steps = %d (a round would overwrite its own samples '
                         'before they are collected)' % (chunk, ring_steps))


def ring_rounds(lengths, batch_sz, chunk, ring_steps, hop):
    """``plan_ring``'s rounds as a generator over an iterator of lengths, which is read one utterance ahead of
    the slots (to know whether any waits, as ``plan_sessions`` does): an endless iterator gives an endless
    schedule."""
    _check_ring_args(batch_sz, chunk, ring_steps, hop)
    B, chunk, R, hop = int(batch_sz), int(chunk), int(ring_steps), int(hop)
    Rlc = -(-R // hop) * hop
    it = iter(lengths)
    state = {'u': 0}

    def pull():
        try:
            n = int(next(it))
        except StopIteration:
            return None
        if n < 1:
            raise ValueError('plan_ring: lengths[%d] = %d must be >= 1' % (state['u'], n))
        return n

    ahead = pull()
    # per slot: the utterance, its length, frames, local steps run, rows fed, samples collected
    sess = [None] * B
    left = [0] * B
    while True:
        begins = []
        for slot in range(B):
            if left[slot] <= 0 and ahead is not None:
                n, u = ahead, state['u']
                state['u'] += 1
                ahead = pull()
                nf = min(-(-n // hop), Rlc // hop)
                sess[slot] = dict(u=u, len=n, frames=-(-n // hop), i=0, rows=nf * hop)
                begins.append((slot, u, nf))
                left[slot] = n
        need = max(left)
        if need <= 0:
            return
        todo = chunk if ahead is not None else min(chunk, need)
        left = [r - todo for r in left]
        while todo > 0:
            # feed every live session what its ring takes: the rows behind the one its next step reads are free
            extends, can = [], todo
            for slot, s in enumerate(sess):
                if s is None or s['i'] >= s['len']:
                    continue       # no session, or past its end: the clamp is the rule there
                full = s['frames'] * hop
                rows = min(full, (max(s['i'] - 1, 0) // hop) * hop + Rlc)
                if rows > s['rows']:
                    extends.append((slot, s['u'], s['rows'] // hop, (rows - s['rows']) // hop))
                    s['rows'] = rows
                if s['rows'] < full:          # local step j reads row j - 1: steps up to j = rows may run
                    can = min(can, s['rows'] - s['i'] + 1)
            steps = min(can, R)
            collects = []
            for slot, s in enumerate(sess):
                if s is None:
                    continue
                lo, hi = min(s['i'], s['len']), min(s['i'] + steps, s['len'])
                s['i'] += steps
                if hi > lo:
                    collects.append((slot, s['u'], lo, hi - lo))
            yield steps, begins, extends, collects
            begins = []
            todo -= steps


def plan_ring(lengths, batch_sz, chunk, ring_steps, hop):
    """``plan_sessions`` for a ring plan of ``ring_steps`` = R columns and Rlc = ceil(R/hop)·hop rows per stream:
    the same deal of utterances to slots at the same chunk boundaries and the same total, each round with
    what a ring needs around it.  Returns (rounds, total); a round is (steps, begins, extends, collects):
      begins   [(slot, utterance, n_frames)]        begin with the utterance's first n_frames frames
      extends  [(slot, utterance, f0, n_frames)]    then extend with its frames [f0, f0 + n_frames)
      collects [(slot, utterance, i0, n)]           after the steps, collect its local steps [i0, i0 + n)
    A round of ``plan_sessions`` is cut into several where a session's rows run out before the round ends (an
    utterance longer than the ring is begun with what fits and extended round by round; only the first
    piece carries the begins).  Guaranteed: no round runs more than R steps; no session ever holds more than
    Rlc rows beyond the one its next step reads; no step runs before its mel row is fed, except past an
    utterance's end, where the last row is repeated (the per-session clamp); every sample of every
    utterance is collected exactly once, in order, right after the round that drew it.  ValueError naming
    the argument for what cannot be scheduled (chunk > ring_steps).  Pure host arithmetic."""
    rounds = list(ring_rounds([int(n) for n in lengths], batch_sz, chunk, ring_steps, hop))
    return rounds, sum(r[0] for r in rounds)


class GenState:
    """A snapshot written by lbwn_gen_state_save: ``blob`` is the uint8 tensor in the documented layout
    (256-byte header, then n_streams stream-major records), ``dims`` the arch dimensions it belongs to."""

    def __init__(self, blob, n_streams, n_blocks, n_block_layers, n_res, n_quant):
        self.blob = blob
        self.n_streams = int(n_streams)
        self.dims = dict(n_blocks=int(n_blocks), n_block_layers=int(n_block_layers), n_res=int(n_res),
                         n_quant=int(n_quant))
        self.record_bytes = state_record_bytes(self.dims['n_blocks'], self.dims['n_block_layers'], self.dims['n_res'])
        want = STATE_HEADER + self.n_streams * self.record_bytes
        if blob.dtype != torch.uint8 or blob.dim() != 1 or blob.numel() != want:
            raise ValueError('state: blob must be uint8 [%d], got %s %s' % (want, blob.dtype, tuple(blob.shape)))

    def header(self):
        """The parsed header (one device synchronisation)."""
        return parse_state_header(self.blob[:STATE_HEADER].cpu().numpy())

    def step(self):
        """The step the snapshot was taken at (one device synchronisation)."""
        return self.header()['step']

    def save(self, path):
        """Write the blob with np.save (a .npy of uint8; numpy appends '.npy' to a path without it)."""
        np.save(path, self.blob.cpu().numpy(), allow_pickle=False)

    @classmethod
    def load(cls, path, device='cuda'):
        """Read a snapshot written by ``save`` (no pickle); the header says whose it is."""
        a = np.load(path, allow_pickle=False)
        if a.dtype != np.uint8 or a.ndim != 1:
            raise ValueError('state file %s: expected a 1-D uint8 array, got %s %s' % (path, a.dtype, a.shape))
        h = parse_state_header(a)
        if a.size != STATE_HEADER + h['n_streams'] * h['record_bytes']:
            raise ValueError('state file %s: %d bytes, the header says %d' % (
                path, a.size, STATE_HEADER + h['n_streams'] * h['record_bytes']))
        return cls(torch.from_numpy(a).to(device), h['n_streams'], *(h[k] for k in STATE_DIMS))


class WaveNetGen:
    def __init__(self, n_blocks, n_block_layers, n_quant, n_res, n_dil, n_skip, n_post1, n_gc_embed,
                 n_gc_category, use_bias, batch_sz, chunk_sz, teacher_vec=None, *, pre_bias=True, seed=0,
                 device='cuda', graph=True, n_lc_in=0, n_lc_out=0, lc_upsample=(), temperature=1.0, top_k=0,
                 top_p=1.0, ring_steps=0):
        if isinstance(ring_steps, bool) or not isinstance(ring_steps, (int, np.integer)) or ring_steps < 0:
            raise ValueError('ring_steps must be an integer >= 0, got %r' % (ring_steps,))
        self.ring_steps = int(ring_steps)     # > 0: a ring plan (lbwn_gen_plan_create_ex); max_steps is then R
        self.sampling = self._check_sampling(temperature, top_k, top_p)
        self.arch = normalize_arch(dict(n_blocks=n_blocks, n_block_layers=n_block_layers, n_quant=n_quant,
                                        n_res=n_res, n_dil=n_dil, n_skip=n_skip, n_post=n_post1,
                                        n_gc_embed=n_gc_embed, n_gc_category=n_gc_category, use_bias=use_bias,
                                        n_lc_in=n_lc_in if n_lc_out else 0, n_lc_out=n_lc_out,
                                        lc_upsample=list(lc_upsample) if n_lc_out else []))
        self.hop = mel_hop_sz(self.arch) if self.arch['n_lc_out'] > 0 else 0
        self.batch_sz = batch_sz
        self.chunk_sz = chunk_sz
        self.pre_bias = bool(pre_bias)
        self.seed = int(seed)
        self.device = torch.device(device)
        self.use_graph = graph
        self.lib = _lib.load()
        self.layout = ParamLayout(self.arch)
        self.flat = torch.zeros(self.layout.n_total, dtype=torch.float32, device=self.device)
        self.vars = self.layout.views(self.flat)
        self.teacher_vec = teacher_vec
        self.teacher_mu = None
        if teacher_vec is not None:
            from .ops import mu_encode
            self.teacher_mu = mu_encode(torch.as_tensor(np.asarray(teacher_vec), dtype=torch.float32,
                                                        device=self.device), n_quant)   # imodel.py:46
            print('Teacher vec is {} samples long.'.format(len(teacher_vec)), file=sys.stderr)
        self._plan = None
        self._ws = None
        self._graph = None
        self._graph_mode = None   # (session mode, steps) the captured chunk was captured with
        self._mel = None      # the mel loaded by the last init_buffers (None: none since lbwn_gen_start)
        self._started = False   # init_buffers (lbwn_gen_start) ran on the current plan
        self._state_keep = None   # the snapshot and map of the last load_state: its launch reads them in stream order
        self._fan = None        # (n_voices, n), the private generator of the last fan-out prefill
        self.teacher_logp = None   # [batch_sz, n] of the last init_buffers(prefill='score')
        self._score_scratch = None   # (plan, uint8 tensor): lbwn_gen_score's scratch, allocated once per plan
        self._reset_sessions()

    def _reset_sessions(self):
        """Host mirror of what lbwn_gen_start resets: no session mode, the step 0, no stream has a base."""
        self._sess_mode = False          # a begin since the last lbwn_gen_start
        self._hstep = 0                  # the device step counter, tracked on the host (None: unknown)
        self._base = [None] * self.batch_sz   # each slot's step origin
        self._sess_mels = {}             # slot -> the device mel its upsample launches read
        self._rows = [0] * self.batch_sz      # each slot's rows given by begin and extend (the plan's mirror)

    # ---- parameters -------------------------------------------------------------------------
    def load_params(self, src, ema=False):
        """src: WaveNetTrain, {serial name: tensor/array}, or a flat tensor of this layout.  With
        ``ema`` (a {name: tensor} source only) every variable is taken from its averaged shadow,
        '<name>/ExponentialMovingAverage' (lbwn.optim.AdamOptimizer(ema_decay=...) saves them); a
        ValueError names the first one the source lacks."""
        with torch.no_grad():
            if hasattr(src, 'vars'):
                src = src.vars
            if isinstance(src, torch.Tensor):
                if ema:
                    raise ValueError('ema: a flat tensor holds no shadows; pass the checkpoint\'s {name: tensor}')
                self.flat.copy_(src)
                return
            sfx = '/ExponentialMovingAverage' if ema else ''
            for name in self.vars:
                if ema and name + sfx not in src:
                    raise ValueError('ema: the checkpoint has no %s (was it trained with ema_decay?)' % (name + sfx))
            for name, v in self.vars.items():
                t = src[name + sfx]
                v.copy_(torch.as_tensor(np.asarray(t) if not isinstance(t, torch.Tensor) else t,
                                        dtype=torch.float32))

    def restore(self, path, ema=False):
        from .ckpt import load_tensors
        self.load_params(load_tensors(path), ema=ema)

    # ---- graph ------------------------------------------------------------------------------
    def build_graph(self, max_steps):
        """Allocate the generation plan for up to max_steps samples (imodel.py:279-303)."""
        a = _lib.Arch()
        for k in ('n_blocks', 'n_block_layers', 'n_quant', 'n_res', 'n_dil', 'n_skip', 'n_post',
                  'n_gc_embed', 'n_gc_category', 'n_lc_in', 'n_lc_out'):
            setattr(a, k, int(self.arch[k]))
        ups = self.arch['lc_upsample'] if self.arch['n_lc_out'] > 0 else []
        if len(ups) > 8:
            raise ValueError('lc_upsample has %d stages, at most 8 are supported' % len(ups))
        a.n_lc_upsample = len(ups)
        for i, s in enumerate(ups):
            a.lc_upsample[i] = int(s)
        a.use_bias = int(self.arch['use_bias'])
        self._arch_c = a
        h = ctypes.c_void_p()
        n_teach = 0 if self.teacher_mu is None else self.teacher_mu.numel()
        if self.ring_steps:
            # a ring plan: "samples" / "wav" hold ring_steps columns whatever the run's length (max_steps, the
            # column count of samples() and of the wav view, is the ring's)
            args = _lib.GenPlanArgs(batch_sz=self.batch_sz, max_steps=1, max_teacher=int(n_teach),
                                    ring_steps=self.ring_steps)
            _lib.check(self.lib.lbwn_gen_plan_create_ex(ctypes.byref(a), ctypes.byref(args), ctypes.byref(h)))
            max_steps = self.ring_steps
        else:
            _lib.check(self.lib.lbwn_gen_plan_create(ctypes.byref(a), self.batch_sz, int(max_steps), int(n_teach),
                                                     ctypes.byref(h)))
        self._plan = h
        self.max_steps = int(max_steps)
        nbytes = self.lib.lbwn_gen_workspace_bytes(h)
        self._ws = torch.zeros(nbytes, dtype=torch.uint8, device=self.device)
        P = _lib.Params()
        base = self.flat.data_ptr()
        for field, off in self.layout.kind_base.items():
            if field.startswith('lc_up'):
                P.lc_up[int(field[5:])] = base + 4 * off
            else:
                setattr(P, field, base + 4 * off)
        self._params_c = P
        self._graph = None
        self._started = False
        self._reset_sessions()
        self._apply_sampling()
        return self

    # ---- sampling ---------------------------------------------------------------------------
    @staticmethod
    def _check_sampling(temperature, top_k, top_p):
        """(float T, int k, float p) or ValueError naming the argument.  No library call."""
        try:
            T, p = float(temperature), float(top_p)
        except (TypeError, ValueError):
            raise ValueError('temperature and top_p must be numbers, got %r and %r' % (temperature, top_p))
        if not (math.isfinite(T) and T > 0):
            raise ValueError('temperature must be finite and > 0, got %r' % (temperature,))
        if isinstance(top_k, bool) or not isinstance(top_k, (int, np.integer)) or top_k < 0:
            raise ValueError('top_k must be an integer >= 0, got %r' % (top_k,))
        if not (0 < p <= 1):
            raise ValueError('top_p must be in (0, 1], got %r' % (top_p,))
        return T, int(top_k), p

    def _apply_sampling(self):
        T, k, p = self.sampling
        _lib.check(self.lib.lbwn_gen_set_sampling(self._plan, T, k, p))

    def set_sampling(self, temperature=None, top_k=None, top_p=None):
        """Change the draw's filters (None keeps the current value) for the steps run from now on.
        The plan reads them at launch, so a captured graph holds the old ones: it is dropped and the
        next ``step`` captures again."""
        T, k, p = self.sampling
        self.sampling = self._check_sampling(T if temperature is None else temperature,
                                             k if top_k is None else top_k, p if top_p is None else top_p)
        if self._plan is not None:
            self._apply_sampling()
        self._graph = None
        return self

    @property
    def persistent(self):
        """True when the plan runs each gen_run as one persistent launch (stream groups of <= 16,
        B <= 80 on 256 CUs)."""
        return bool(self._plan is not None and self.lib.lbwn_gen_is_persistent(self._plan))

    def tensor(self, name, dtype=torch.float32):
        off, nb = _lib.c_size_t(), _lib.c_size_t()
        _lib.check(self.lib.lbwn_gen_tensor(self._plan, name.encode(), ctypes.byref(off), ctypes.byref(nb)))
        return self._ws[off.value:off.value + nb.value].view(dtype)

    def _check_mel(self, mel, gen_sz=None):
        """mel as a float32 [B, n_frames, n_lc_in] array/tensor (None for archs without LC);
        ValueError on a missing mel, a shape mismatch or a mel too short for gen_sz steps."""
        if self.arch['n_lc_out'] == 0:
            if mel is not None:
                raise ValueError('mel given, but the arch has no local conditioning')
            return None
        if mel is None:
            raise ValueError('LC arch: mel [batch_sz, n_frames, n_lc_in] required')
        if not isinstance(mel, torch.Tensor):
            mel = np.asarray(mel, np.float32)
        Li = self.arch['n_lc_in']
        shp = tuple(mel.shape)
        if len(shp) == 2:
            shp = (self.batch_sz,) + shp
            mel = mel[None].expand(*shp) if isinstance(mel, torch.Tensor) else np.broadcast_to(mel[None], shp)
        if len(shp) != 3 or shp[0] != self.batch_sz or shp[2] != Li or shp[1] < 1:
            raise ValueError('mel has shape %s, expected [%d, n_frames, %d] or [n_frames, %d]'
                             % (tuple(mel.shape), self.batch_sz, Li, Li))
        if gen_sz is not None and gen_sz > shp[1] * self.hop + 1:
            raise ValueError('gen_sz %d needs more than the %d mel frames given (%d rows cover %d steps)'
                             % (gen_sz, shp[1], shp[1] * self.hop, shp[1] * self.hop + 1))
        return mel

    def _check_codes(self, codes, mel_coming=False):
        """Prompt codes as an integer [batch_sz, n] or [n] (shared by every stream) array/tensor;
        ValueError on an LC arch with no mel loaded (and none being loaded by the same
        init_buffers call: mel_coming), a float dtype, a shape mismatch or n < 1.  No library call."""
        if self.arch['n_lc_out'] > 0 and self._mel is None and not mel_coming:
            raise ValueError('prefill: local conditioning is not supported before a mel is loaded '
                             '(init_buffers(mel=...) first)')
        if not isinstance(codes, torch.Tensor):
            codes = np.asarray(codes)
            if codes.dtype.kind not in 'iu':
                raise ValueError('prefill: codes must be integers, got dtype %s' % codes.dtype)
        elif codes.dtype not in (torch.int32, torch.int64, torch.int16, torch.int8, torch.uint8):
            raise ValueError('prefill: codes must be integers, got dtype %s' % codes.dtype)
        shp = tuple(codes.shape)
        if len(shp) not in (1, 2) or (len(shp) == 2 and shp[0] != self.batch_sz):
            raise ValueError('prefill: codes have shape %s, expected [n] or [%d, n]' % (shp, self.batch_sz))
        if shp[-1] < 1:
            raise ValueError('prefill: n must be >= 1')
        return codes

    def prefill(self, codes):
        """Advance every stream by the n known inputs ``codes`` (int [n], shared, or [batch_sz, n]) in
        parallel over the n positions (lbwn_gen_prefill): the state n teacher-forced steps leave,
        with the prompt itself as samples / wav of those steps.  On the current stream."""
        codes = self._check_codes(codes)
        if self._plan is None:
            raise RuntimeError('prefill: no plan (build_graph and init_buffers first)')
        if not isinstance(codes, torch.Tensor):
            codes = torch.from_numpy(np.ascontiguousarray(codes).astype(np.int32))
        # kept until the next prefill: the launches read it in stream order
        self._prefill_codes = codes.to(device=self.device, dtype=torch.int32).contiguous()
        n = int(codes.shape[-1])
        _lib.check(self.lib.lbwn_gen_prefill(self._plan, ctypes.byref(self._params_c), self._ws.data_ptr(),
                                             self._prefill_codes.data_ptr(), n if codes.dim() == 2 else 0, n,
                                             _lib.stream_ptr()))
        if self._hstep is not None:
            self._hstep += n
        return n

    def score(self, codes):
        """log p(code | history) of the known waveform ``codes`` (int [n], shared, or [batch_sz, n]) under
        the model, natural log, as a float32 [batch_sz, n] tensor on the device (lbwn_gen_score): entry
        [b, j] is the log-probability of codes[b, j] at the step it is fed in.  The state advances exactly as
        ``prefill(codes)`` advances it, and ``logits()`` holds the last scored step's.  To score without
        advancing: ``s = save_state(); score(codes); load_state(s)``.  On the current stream."""
        codes = self._check_codes(codes)
        if self._plan is None:
            raise RuntimeError('score: no plan (build_graph and init_buffers first)')
        if not isinstance(codes, torch.Tensor):
            codes = torch.from_numpy(np.ascontiguousarray(codes).astype(np.int32))
        # kept until the next call: the launches read it in stream order
        self._prefill_codes = codes.to(device=self.device, dtype=torch.int32).contiguous()
        n = int(codes.shape[-1])
        if self._score_scratch is None or self._score_scratch[0] is not self._plan:   # once per plan
            nb = self.lib.lbwn_gen_score_scratch_bytes(self._plan)
            self._score_scratch = (self._plan, torch.empty(nb, dtype=torch.uint8, device=self.device))
        logp = torch.empty(self.batch_sz, n, dtype=torch.float32, device=self.device)
        _lib.check(self.lib.lbwn_gen_score(self._plan, ctypes.byref(self._params_c), self._ws.data_ptr(),
                                           self._prefill_codes.data_ptr(), n if codes.dim() == 2 else 0, n,
                                           logp.data_ptr(), n, self._score_scratch[1].data_ptr(), _lib.stream_ptr()))
        if self._hstep is not None:
            self._hstep += n
        return logp

    # ---- state ------------------------------------------------------------------------------
    def _state_dims(self):
        return {k: int(self.arch[k]) for k in STATE_DIMS}

    def _check_map(self, streams, n_src, what):
        """``streams`` as a list of batch_sz ints in [0, n_src) (None: identity, n_src == batch_sz);
        ValueError otherwise.  No library call."""
        if streams is None:
            if n_src != self.batch_sz:
                raise ValueError('%s: streams=None (identity) needs a state of batch_sz = %d streams, got %d'
                                 % (what, self.batch_sz, n_src))
            return None
        try:
            m = list(streams)
        except TypeError:
            raise ValueError('%s: streams must be a list of %d stream indices, got %r' % (what, self.batch_sz, streams))
        if len(m) != self.batch_sz:
            raise ValueError('%s: streams has %d entries, batch_sz is %d' % (what, len(m), self.batch_sz))
        for b, s in enumerate(m):
            if isinstance(s, bool) or not isinstance(s, (int, np.integer)) or not 0 <= s < n_src:
                raise ValueError('%s: streams[%d] = %r is not an integer in [0, %d)' % (what, b, s, n_src))
        return [int(s) for s in m]

    def save_state(self):
        """The state of the run as a ``GenState`` (lbwn_gen_state_save, on the current stream): every
        stream's rings and pending code and the step.  "samples" / "wav" are not part of it."""
        if self._plan is None:
            raise ValueError('save_state: no plan (build_graph and init_buffers first)')
        nb = self.lib.lbwn_gen_state_bytes(self._plan, self.batch_sz)
        blob = torch.empty(nb, dtype=torch.uint8, device=self.device)
        _lib.check(self.lib.lbwn_gen_state_save(self._plan, self._ws.data_ptr(), blob.data_ptr(), _lib.stream_ptr()))
        return GenState(blob, self.batch_sz, **self._state_dims())

    def load_state(self, state, streams=None):
        """Stream b continues from record ``streams[b]`` of ``state`` (None: record b) at the state's step
        (lbwn_gen_state_load, on the current stream; after init_buffers, which supplies everything that is
        not state).  Draws stay keyed by the destination stream, so streams loaded from one record continue
        differently.  A captured graph stays valid.  A snapshot the device refuses sets status 6
        (``check_status``)."""
        if self._plan is None:
            raise ValueError('load_state: no plan (build_graph and init_buffers first)')
        if not isinstance(state, GenState):
            raise ValueError('load_state: state must be a GenState, got %s' % type(state).__name__)
        if state.dims != self._state_dims():
            raise ValueError('load_state: the state belongs to another arch (%r, this plan has %r)'
                             % (state.dims, self._state_dims()))
        m = self._check_map(streams, state.n_streams, 'load_state')
        if not self._started:
            raise RuntimeError('load_state: init_buffers first (it supplies the images, GC projections and seed)')
        blob = state.blob.to(self.device)
        mt = None if m is None else torch.tensor(m, dtype=torch.int32, device=self.device)
        self._state_keep = (blob, mt)
        _lib.check(self.lib.lbwn_gen_state_load(self._plan, self._ws.data_ptr(), blob.data_ptr(), state.n_streams,
                                                _lib.ptr(mt), _lib.stream_ptr()))
        self._hstep = None        # the snapshot's step: read from the device when a begin needs it
        return self

    def fork(self, src):
        """Continue several streams from one: an int sends every stream to the state of stream ``src``, a
        list [batch_sz] is a gather (stream b continues from stream src[b]).  save_state + load_state."""
        if self._plan is None:
            raise ValueError('fork: no plan (build_graph and init_buffers first)')
        if not isinstance(src, bool) and isinstance(src, (int, np.integer)):
            src = [src] * self.batch_sz
        m = self._check_map(src, self.batch_sz, 'fork')
        if m is None:
            raise ValueError('fork: src must be a stream index or a list of batch_sz indices')
        return self.load_state(self.save_state(), m)

    def _check_prefill(self, prefill, mel):
        """prefill is False, True, 'fanout' or 'score'; a fan-out takes a shared (2-D) mel only.  ValueError
        otherwise."""
        if prefill not in (False, True, 'fanout', 'score'):
            raise ValueError("prefill must be False, True, 'fanout' or 'score', got %r" % (prefill,))
        if prefill == 'fanout' and mel is not None and len(tuple(mel.shape)) != 2:
            raise ValueError("prefill='fanout' takes a shared mel [n_frames, n_lc_in] only, got shape %s"
                             % (tuple(mel.shape),))

    def _fanout(self, gc_ids, mel):
        """Prefill the teacher once per distinct voice in a private generator of that many streams (sharing
        this one's parameters) and return (its state, the map stream -> record, n)."""
        n = min(int(self.teacher_mu.numel()), self.max_steps)
        if self.arch['n_gc_embed'] > 0:
            ids = np.asarray(gc_ids, np.int32).reshape(-1)
            voices, smap = np.unique(ids, return_inverse=True)
        else:
            voices, smap = None, np.zeros(self.batch_sz, np.int64)
        nv = 1 if voices is None else len(voices)
        if self._fan is None or self._fan[0] != (nv, n):
            a = self.arch
            sub = WaveNetGen(a['n_blocks'], a['n_block_layers'], a['n_quant'], a['n_res'], a['n_dil'], a['n_skip'],
                             a['n_post'], a['n_gc_embed'], a['n_gc_category'], a['use_bias'], nv, self.chunk_sz, None,
                             pre_bias=self.pre_bias, seed=self.seed, device=self.device, graph=False,
                             n_lc_in=a['n_lc_in'], n_lc_out=a['n_lc_out'],
                             lc_upsample=a['lc_upsample'] if a['n_lc_out'] > 0 else ())
            sub.flat = self.flat          # the same parameters, not a copy
            sub.vars = self.vars
            sub.build_graph(n)
            self._fan = ((nv, n), sub)
        sub = self._fan[1]
        sub.init_buffers(None if voices is None else voices, mel)
        sub.prefill(self.teacher_mu.reshape(-1)[:n])
        return sub.save_state(), [int(v) for v in smap.reshape(-1)], n

    def init_buffers(self, gc_ids=None, mel=None, prefill=False):
        """imodel.init_buffers: zero the lookback/loop buffers, load teacher + GC ids (+ the mel of
        an LC arch, upsampled once).  ``prefill=True`` with a teacher: start without the teacher
        vector and prefill its µ-law codes instead (at most max_steps of them); returns the number
        of steps already taken that way (0 otherwise); on an LC arch the prefilled steps are
        conditioned on the mel this call loads.  ``prefill='fanout'``: the same result for a teacher
        shared by the streams, but the prompt is prefilled once per distinct voice id of ``gc_ids`` (once on
        an arch without GC) and that state loaded into every stream of the voice; mel absent or 2-D.
        ``prefill='score'``: as True through ``score``; the teacher's log-probabilities [batch_sz, n] are kept
        in ``teacher_logp``."""
        self._check_prefill(prefill, mel)
        if prefill and self.teacher_mu is not None:
            self._check_codes(self.teacher_mu, mel_coming=mel is not None)
        mel_shared = mel
        mel = self._check_mel(mel)
        if mel is not None:   # frames past the plan's ceil(max_steps / hop) condition no step
            mel = mel[:, :-(-self.max_steps // self.hop)]
        self._gc = None
        if self.arch['n_gc_embed'] > 0:
            if gc_ids is None:
                raise ValueError('GC arch: gc_ids [batch_sz] required (generate.py:94)')
            ids = np.asarray(gc_ids, np.int32).reshape(-1)
            if ids.size != self.batch_sz:
                raise ValueError('gc_ids has %d entries, batch_sz is %d' % (ids.size, self.batch_sz))
            self._gc = torch.as_tensor(ids, device=self.device)
        t = None if prefill else self.teacher_mu
        _lib.check(self.lib.lbwn_gen_start(self._plan, ctypes.byref(self._params_c), self._ws.data_ptr(),
                                           _lib.ptr(self._gc), _lib.ptr(t), 0 if t is None else t.numel(),
                                           self.seed, int(self.pre_bias), _lib.stream_ptr()))
        self._mel = None      # lbwn_gen_start clears the loaded mel
        self._reset_sessions()
        if mel is not None:
            if not isinstance(mel, torch.Tensor):
                mel = torch.from_numpy(np.array(mel, np.float32))   # a writable copy (a broadcast view is not)
            self._mel = mel.to(device=self.device, dtype=torch.float32).contiguous()
            _lib.check(self.lib.lbwn_gen_set_mel(self._plan, ctypes.byref(self._params_c), self._ws.data_ptr(),
                                                 self._mel.data_ptr(), self._mel.shape[1], _lib.stream_ptr()))
        self._started = True
        if prefill == 'fanout' and self.teacher_mu is not None:
            state, smap, n = self._fanout(gc_ids, mel_shared)
            self.load_state(state, smap)
            # the outputs of the prefilled steps, as lbwn_gen_prefill leaves them: the prompt and its decode
            from .ops import mu_decode
            q = self.teacher_mu.reshape(-1)[:n].to(torch.int32).clamp(0, self.arch['n_quant'] - 1)
            self.samples()[:, :n] = q
            self.tensor('wav').view(self.batch_sz, self.max_steps)[:, :n] = mu_decode(q, self.arch['n_quant'])
            return n
        if prefill == 'score' and self.teacher_mu is not None:
            self.teacher_logp = self.score(self.teacher_mu.reshape(-1)[:self.max_steps])
            return int(self.teacher_logp.shape[1])
        if prefill and self.teacher_mu is not None:
            return self.prefill(self.teacher_mu.reshape(-1)[:self.max_steps])
        return 0

    def _launch(self, n):
        _lib.check(self.lib.lbwn_gen_run(self._plan, ctypes.byref(self._params_c), self._ws.data_ptr(), n,
                                         _lib.stream_ptr()))

    def step(self, n_steps):
        """Advance every stream by n_steps samples (graph replay of chunk_sz-step chunks)."""
        chunk = self.chunk_sz
        done = 0
        # a captured chunk is bound to what its capture baked in: the number of steps, and whether the draw
        # and the LC projection take the session words (session mode) or not (the dense path).  A later
        # lbwn_gen_start or begin that changes the mode makes it draw from the wrong table: capture again.
        if self._graph is not None and self._graph_mode != (self._sess_mode, chunk):
            self._graph = None
        if self.use_graph and n_steps >= chunk:
            if self._graph is None:
                self._graph_mode = (self._sess_mode, chunk)
                s = torch.cuda.Stream()
                s.wait_stream(torch.cuda.current_stream())
                g = torch.cuda.CUDAGraph()
                with torch.cuda.stream(s):
                    with torch.cuda.graph(g, stream=s):
                        self._launch(chunk)
                torch.cuda.current_stream().wait_stream(s)
                self._graph = g
                done += chunk           # capture does not execute; replay below covers it
                self._graph.replay()
            while n_steps - done >= chunk:
                self._graph.replay()
                done += chunk
        if n_steps - done > 0:
            self._launch(n_steps - done)
        if self._hstep is not None:
            self._hstep += int(n_steps)

    def run(self, gen_sz, gc_ids=None, mel=None, prefill=False):
        """The reference's sess.run(wave_ops) (generate.py:110): generate gen_sz steps from a
        fresh state; the returned waveform holds whole chunks only (imodel.py:256-258).  LC archs:
        mel must cover the run, gen_sz <= n_frames·hop + 1.  ``prefill=True``: the teacher's steps
        are prefilled in parallel instead of stepped (the same continuation up to fp32 rounding;
        the waveform then starts with the µ-law-quantised teacher, not the model's ignored draws).
        ``prefill='fanout'``: as True, the prompt prefilled once per distinct voice id (``init_buffers``).
        ``prefill='score'``: as True, and ``teacher_logp`` holds the teacher's log-probabilities."""
        self._check_prefill(prefill, mel)
        if self.ring_steps and gen_sz > self.ring_steps:
            raise ValueError('run: gen_sz %d exceeds ring_steps %d (a ring plan returns its last ring_steps samples '
                             'through collect)' % (gen_sz, self.ring_steps))
        mel_in = mel
        mel = self._check_mel(mel, int(gen_sz))
        if self._plan is None or self.max_steps < gen_sz:
            self.build_graph(gen_sz)
        done = self.init_buffers(gc_ids, mel_in if prefill == 'fanout' else mel, prefill=prefill)
        self.step(max(int(gen_sz) - done, 0))
        self.check_status()
        n_out = (int(gen_sz) // self.chunk_sz) * self.chunk_sz
        wav = self.tensor('wav').view(self.batch_sz, self.max_steps)[:, :n_out]
        return int(gen_sz), wav, int(gen_sz) % self.chunk_sz

    def check_status(self):
        """Raise if a skip helper's granule poll timed out (status 5): the step's skip sum, and
        every draw after it, would be wrong; or if the device refused a load_state (status 6: the
        snapshot's header or the stream map does not fit the plan; nothing was loaded)."""
        s = int(self.tensor('status', torch.int32).item())
        if s == 6:
            raise RuntimeError('generation status 6: load_state refused the snapshot or the stream map')
        if s == 7:
            raise RuntimeError('generation status 7: the device refused the range of an extend or a collect')
        if s != 0:
            raise RuntimeError('generation status %d: a skip-helper hand-off timed out' % s)

    def samples(self):
        return self.tensor('samples', torch.int32).view(self.batch_sz, self.max_steps)

    def logits(self):
        return self.tensor('logits').view(self.batch_sz, self.arch['n_quant'])

    # ---- sessions ---------------------------------------------------------------------------
    def init_sessions(self):
        """lbwn_gen_start for a run whose streams all get their voice and mel from ``begin``: no teacher,
        voice id 0 everywhere until a session says otherwise, no dense mel."""
        if self._plan is None:
            raise RuntimeError('init_sessions: no plan (build_graph first)')
        self._gc = None
        if self.arch['n_gc_embed'] > 0:
            self._gc = torch.zeros(self.batch_sz, dtype=torch.int32, device=self.device)
        _lib.check(self.lib.lbwn_gen_start(self._plan, ctypes.byref(self._params_c), self._ws.data_ptr(),
                                           _lib.ptr(self._gc), None, 0, self.seed, int(self.pre_bias),
                                           _lib.stream_ptr()))
        self._mel = None
        self._reset_sessions()
        self._started = True
        return self

    def _check_begin(self, slots, mels, gc_ids, keys):
        """(slots, mels, gc_ids, keys) as lists of equal length, validated; ValueError naming the argument.
        No library call."""
        try:
            slots = list(slots)
        except TypeError:
            raise ValueError('begin: slots must be a list of stream indices, got %r' % (slots,))
        n = len(slots)
        if not 1 <= n <= self.batch_sz:
            raise ValueError('begin: %d slots given, expected 1..batch_sz = %d' % (n, self.batch_sz))
        for i, b in enumerate(slots):
            if isinstance(b, bool) or not isinstance(b, (int, np.integer)) or not 0 <= b < self.batch_sz:
                raise ValueError('begin: slots[%d] = %r is not an integer in [0, %d)' % (i, b, self.batch_sz))
        if len(set(int(b) for b in slots)) != n:
            raise ValueError('begin: slots %r lists a stream twice' % (slots,))
        keys = list(slots) if keys is None else list(keys)
        if len(keys) != n:
            raise ValueError('begin: keys has %d entries for %d slots' % (len(keys), n))
        for i, k in enumerate(keys):
            if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 0 <= k < 2 ** 31:
                raise ValueError('begin: keys[%d] = %r is not an integer in [0, 2^31)' % (i, k))
        if self.arch['n_gc_embed'] > 0:
            if gc_ids is None:
                raise ValueError('begin: GC arch, gc_ids (one voice id per slot) required')
            gc_ids = list(gc_ids)
            if len(gc_ids) != n:
                raise ValueError('begin: gc_ids has %d entries for %d slots' % (len(gc_ids), n))
            for i, v in enumerate(gc_ids):
                if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or \
                        not 0 <= v <= self.arch['n_gc_category']:
                    raise ValueError('begin: gc_ids[%d] = %r is not a voice id in [0, %d]'
                                     % (i, v, self.arch['n_gc_category']))
        else:
            gc_ids = [0] * n
        if self.arch['n_lc_out'] == 0:
            if mels is not None:
                raise ValueError('begin: mels given, but the arch has no local conditioning')
            mels = [None] * n
        else:
            if mels is None:
                raise ValueError('begin: LC arch, mels (one [n_frames, n_lc_in] per slot) required')
            mels = list(mels)
            if len(mels) != n:
                raise ValueError('begin: mels has %d entries for %d slots' % (len(mels), n))
            mels = [self._as_mel(m, 'begin: mels[%d]' % i) for i, m in enumerate(mels)]
        return [int(b) for b in slots], mels, [int(v) for v in gc_ids], [int(k) for k in keys]

    def _as_mel(self, m, what):
        """One utterance's mel as a tensor or float32 array [n_frames, n_lc_in] (a nested list is converted);
        ValueError naming ``what`` otherwise."""
        if not isinstance(m, torch.Tensor):
            try:
                m = np.asarray(m, np.float32)
            except (TypeError, ValueError):
                raise ValueError('%s is not an array of numbers [n_frames, %d]' % (what, self.arch['n_lc_in']))
        shp = tuple(m.shape)
        if len(shp) != 2 or shp[1] != self.arch['n_lc_in'] or shp[0] < 1:
            raise ValueError('%s has shape %s, expected [n_frames, %d]' % (what, shp, self.arch['n_lc_in']))
        return m

    def begin(self, slots, mels=None, gc_ids=None, keys=None):
        """Begin a new utterance in the streams ``slots`` at the current step while the others continue
        (lbwn_gen_begin, on the current stream): each gets zero rings, its mel ``mels[i]`` [n_frames,
        n_lc_in] (LC archs), its voice ``gc_ids[i]`` (GC archs) and the draw key ``keys[i]`` (default: the
        slot), and counts its steps from here.  After init_buffers without a mel or teacher, or
        init_sessions; an LC plan runs again once every stream has begun a session.  A captured chunk is
        bound to the mode of its capture: one captured before the first begin is dropped (it draws without
        the session words), one captured in session mode stays valid across later begins and is dropped by
        ``step`` once init_buffers / init_sessions has left session mode."""
        slots, mels, gc_ids, keys = self._check_begin(slots, mels, gc_ids, keys)
        if self._plan is None or not self._started:
            raise RuntimeError('begin: no run (build_graph, then init_sessions or init_buffers)')
        if self._hstep is None:       # after a load_state: the snapshot's step
            self._hstep = int(self.tensor('step', torch.int64).item())
        arr = (_lib.GenSession * len(slots))()
        keep = {}
        for i, b in enumerate(slots):
            arr[i].slot, arr[i].gc_id, arr[i].key = b, gc_ids[i], keys[i]
            if mels[i] is not None:
                m = mels[i]
                if not isinstance(m, torch.Tensor):
                    m = torch.from_numpy(np.ascontiguousarray(m, np.float32))
                keep[b] = m.to(device=self.device, dtype=torch.float32).contiguous()
                arr[i].mel, arr[i].n_frames = keep[b].data_ptr(), keep[b].shape[0]
        _lib.check(self.lib.lbwn_gen_begin(self._plan, ctypes.byref(self._params_c), self._ws.data_ptr(), arr,
                                           len(slots), ctypes.sizeof(_lib.GenSession), _lib.stream_ptr()))
        self._sess_mels.update(keep)     # read by the upsample launches in stream order
        if not self._sess_mode:
            self._graph = None
            self._sess_mode = True
        for i, b in enumerate(slots):
            self._base[b] = self._hstep
            self._rows[b] = 0 if mels[i] is None else int(mels[i].shape[0]) * self.hop
        return self

    def _local_step(self, slot):
        """The local steps stream ``slot`` has run, from the host's step mirror (read from the device once after
        a load_state)."""
        if self._hstep is None:
            self._hstep = int(self.tensor('step', torch.int64).item())
        return self._hstep - (self._base[slot] or 0)

    @property
    def lc_ring_rows(self):
        """Rows of one stream's region of "lc": Rlc = ceil(R/hop)·hop on a ring plan, the reserved rows else."""
        return -(-self.max_steps // self.hop) * self.hop if self.hop else 0

    def extend(self, slots, mels):
        """Append more mel frames to the live sessions of ``slots`` (lbwn_gen_extend, on the current stream):
        ``mels[i]`` [n_frames, n_lc_in] are the frames after those the stream already has.  What the device
        guards is refused here first, from the host's step mirror: on a ring plan a session may hold at most
        Rlc rows beyond the one its next step reads, elsewhere at most the reserved rows; ValueError."""
        if self.arch['n_lc_out'] == 0:
            raise ValueError('extend: the arch has no local conditioning (no mel to extend)')
        try:
            slots, mels = list(slots), list(mels)
        except TypeError:
            raise ValueError('extend: slots and mels must be lists, got %r and %r' % (slots, mels))
        n = len(slots)
        if not 1 <= n <= self.batch_sz:
            raise ValueError('extend: %d slots given, expected 1..batch_sz = %d' % (n, self.batch_sz))
        if len(mels) != n:
            raise ValueError('extend: mels has %d entries for %d slots' % (len(mels), n))
        for i, b in enumerate(slots):
            if isinstance(b, bool) or not isinstance(b, (int, np.integer)) or not 0 <= b < self.batch_sz:
                raise ValueError('extend: slots[%d] = %r is not an integer in [0, %d)' % (i, b, self.batch_sz))
            if self._plan is None or self._base[b] is None:
                raise ValueError('extend: slots[%d] = %d has begun no session' % (i, b))
        if len(set(int(b) for b in slots)) != n:
            raise ValueError('extend: slots %r lists a stream twice' % (slots,))
        mels = [self._as_mel(m, 'extend: mels[%d]' % i) for i, m in enumerate(mels)]
        cap = self.lc_ring_rows
        for i, b in enumerate(slots):
            add, rows = int(mels[i].shape[0]) * self.hop, self._rows[b]
            read = min(max(self._local_step(b) - 1, 0), rows) if self.ring_steps else 0
            if rows + add - read > cap:
                raise ValueError('extend: mels[%d] brings %d rows to the %d of stream %d, %d of them read: more than '
                                 'the %d its region holds' % (i, add, rows, b, read, cap))
        arr = (_lib.GenExtendEntry * n)()
        keep = []
        for i, b in enumerate(slots):
            m = mels[i]
            if not isinstance(m, torch.Tensor):
                m = torch.from_numpy(np.ascontiguousarray(m, np.float32))
            m = m.to(device=self.device, dtype=torch.float32).contiguous()
            if m.data_ptr() % 16:
                m = m.clone()
            keep.append(m)
            arr[i].slot, arr[i].mel, arr[i].n_frames = int(b), m.data_ptr(), m.shape[0]
        _lib.check(self.lib.lbwn_gen_extend(self._plan, ctypes.byref(self._params_c), self._ws.data_ptr(), arr, n,
                                            ctypes.sizeof(_lib.GenExtendEntry), _lib.stream_ptr()))
        for i, b in enumerate(slots):
            self._rows[b] += int(keep[i].shape[0]) * self.hop
            self._sess_mels[(int(b), 'ext')] = keep[i]     # read by the upsample launches in stream order
        return self

    def collect(self, slot, i0, n):
        """Local steps [i0, i0 + n) of stream ``slot`` as dense copies (wav float32 [n], samples int32 [n]) on
        the device (lbwn_gen_collect, on the current stream).  The steps must have run and, on a ring plan,
        lie within the last ring_steps of them; ValueError otherwise (the device guards the same)."""
        if self._plan is None or isinstance(slot, bool) or not isinstance(slot, (int, np.integer)) or \
                not 0 <= slot < self.batch_sz:
            raise ValueError('collect: slot %r is not a stream of a built plan' % (slot,))
        if isinstance(i0, bool) or not isinstance(i0, (int, np.integer)) or i0 < 0:
            raise ValueError('collect: i0 must be an integer >= 0, got %r' % (i0,))
        if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or n < 0:
            raise ValueError('collect: n must be an integer >= 0, got %r' % (n,))
        e = self._local_step(slot)
        if i0 + n > e:
            raise ValueError('collect: steps [%d, %d) of stream %d: only %d have run' % (i0, i0 + n, slot, e))
        if self.ring_steps and i0 < e - self.ring_steps:
            raise ValueError('collect: i0 = %d of stream %d is overwritten: %d steps have run and the ring holds '
                             'the last %d' % (i0, slot, e, self.ring_steps))
        if not self.ring_steps and (self._base[slot] or 0) + i0 + n > self.max_steps:
            raise ValueError('collect: steps [%d, %d) of stream %d lie past max_steps %d' % (i0, i0 + n, slot,
                                                                                            self.max_steps))
        wav = torch.empty(int(n), dtype=torch.float32, device=self.device)
        smp = torch.empty(int(n), dtype=torch.int32, device=self.device)
        if n:
            _lib.check(self.lib.lbwn_gen_collect(self._plan, self._ws.data_ptr(), int(slot), int(i0), int(n),
                                                 wav.data_ptr(), smp.data_ptr(), _lib.stream_ptr()))
        return wav, smp

    def take(self, slot, n):
        """The first n samples of the session stream ``slot`` carries: "wav" columns base .. base + n - 1
        (a view; the steps must have run).  On a ring plan a collected copy (they must still be in the ring)."""
        if self._plan is None or not 0 <= slot < self.batch_sz or self._base[slot] is None:
            raise ValueError('take: stream %r has begun no session' % (slot,))
        if self.ring_steps:
            return self.collect(slot, 0, n)[0]
        b0 = self._base[slot]
        if n < 0 or b0 + n > self.max_steps:
            raise ValueError('take: %d samples from step %d exceed max_steps %d' % (n, b0, self.max_steps))
        return self.tensor('wav').view(self.batch_sz, self.max_steps)[slot, b0:b0 + n]

    def vocode(self, mels, gc_ids=None, keys=None, chunk=None):
        """One wav per mel: ``mels`` is a list of [n_frames_u, n_lc_in] arrays of any lengths; utterance u
        gets n_frames_u·hop samples, voice ``gc_ids[u]`` (GC archs) and draw key ``keys[u]`` (default u, so
        the wavs do not depend on batch_sz or on the schedule).  Runs ``plan_sessions(lengths, batch_sz,
        chunk)`` (chunk defaults to chunk_sz and holds for this call only): a stream takes the next utterance
        at the first chunk boundary after its own is covered.  Returns the wavs, float32 tensors on the device, in input order."""
        if self.arch['n_lc_out'] == 0:
            raise ValueError('vocode: the arch has no local conditioning (nothing to vocode from)')
        mels = list(mels)
        if not mels:
            return []
        chunk = self.chunk_sz if chunk is None else int(chunk)
        n_utt = len(mels)
        keys = list(range(n_utt)) if keys is None else list(keys)
        if len(keys) != n_utt:
            raise ValueError('vocode: keys has %d entries for %d mels' % (len(keys), n_utt))
        if self.arch['n_gc_embed'] > 0:
            if gc_ids is None or len(list(gc_ids)) != n_utt:
                raise ValueError('vocode: GC arch, gc_ids (one voice id per mel) required')
            gc_ids = [int(v) for v in gc_ids]
        mels = [self._as_mel(m, 'vocode: mels[%d]' % u) for u, m in enumerate(mels)]
        if self.ring_steps:       # one continuous ring schedule (plan_ring), whatever the list's length
            out = [None] * n_utt
            for u, wav in self.vocode_iter(mels, gc_ids, keys, chunk):
                out[u] = wav
            return out
        lengths = [int(m.shape[0]) * self.hop for m in mels]
        rounds, total = plan_sessions(lengths, self.batch_sz, chunk)
        if self._plan is None or self.max_steps < total:
            self.build_graph(total)
        keep_chunk = self.chunk_sz       # ``chunk`` holds for this call only (step re-captures on a change)
        self.chunk_sz = chunk
        try:
            return self._vocode_rounds(mels, gc_ids, keys, lengths, rounds)
        finally:
            self.chunk_sz = keep_chunk

    def vocode_iter(self, mels, gc_ids=None, keys=None, chunk=None, samples=False):
        """``vocode`` on a ring plan (``ring_steps`` > 0) as a generator over any iterable of mels: yields
        (index, wav) as utterances finish, in the order they finish ((index, wav, µ-law codes) with
        ``samples=True``).  ``gc_ids`` / ``keys`` are iterables
        parallel to ``mels`` (keys default to the indices).  The schedule is ``ring_rounds``: an utterance
        longer than the ring is begun with what fits and extended round by round, every round's samples are
        collected right after it.  At most batch_sz utterances are in flight, plus the one read ahead, so an
        endless iterable runs endlessly in the plan's fixed workspace."""
        if self.arch['n_lc_out'] == 0:
            raise ValueError('vocode_iter: the arch has no local conditioning (nothing to vocode from)')
        if not self.ring_steps:
            raise ValueError('vocode_iter: needs a ring plan (WaveNetGen(..., ring_steps=R))')
        chunk = self.chunk_sz if chunk is None else int(chunk)
        _check_ring_args(self.batch_sz, chunk, self.ring_steps, self.hop)
        gc = self.arch['n_gc_embed'] > 0
        if gc and gc_ids is None:
            raise ValueError('vocode_iter: GC arch, gc_ids (one voice id per mel) required')
        git = iter(gc_ids) if gc else None
        kit = iter(keys) if keys is not None else None
        live = {}                      # utterance -> dict(mel on the device, voice, key, length, parts)

        def lengths():
            for u, m in enumerate(mels):
                m = self._as_mel(m, 'vocode: mels[%d]' % u)
                if not isinstance(m, torch.Tensor):
                    m = torch.from_numpy(np.ascontiguousarray(m, np.float32))
                m = m.to(device=self.device, dtype=torch.float32).contiguous()
                try:
                    live[u] = dict(mel=m, gc=int(next(git)) if gc else 0, key=int(next(kit)) if kit else u,
                                   len=int(m.shape[0]) * self.hop, parts=[])
                except StopIteration:
                    raise ValueError('vocode: gc_ids / keys are shorter than mels (at utterance %d)' % u)
                yield live[u]['len']

        if self._plan is None:
            self.build_graph(self.ring_steps)
        keep_chunk = self.chunk_sz       # ``chunk`` holds for this call only (step re-captures on a change)
        self.chunk_sz = chunk
        try:
            self.init_sessions()
            idle = np.zeros((1, self.arch['n_lc_in']), np.float32)   # streams no utterance has reached yet
            first = True
            for steps, begins, extends, collects in ring_rounds(lengths(), self.batch_sz, chunk, self.ring_steps,
                                                                self.hop):
                slots = [s for s, _, _ in begins]
                ms = [live[u]['mel'][:nf] for _, u, nf in begins]
                ks = [live[u]['key'] for _, u, _ in begins]
                gs = [live[u]['gc'] for _, u, _ in begins] if gc else None
                if first:
                    first = False
                    for s in range(self.batch_sz):
                        if s not in slots:
                            slots.append(s)
                            ms.append(idle)
                            ks.append(0)
                            if gc:
                                gs.append(0)
                if slots:
                    self.begin(slots, ms, gs, ks)
                if extends:
                    self.extend([s for s, _, _, _ in extends], [live[u]['mel'][f0:f0 + nf] for _, u, f0, nf in extends])
                self.step(steps)
                done = []
                for s, u, i0, n in collects:
                    live[u]['parts'].append(self.collect(s, i0, n))
                    if i0 + n == live[u]['len']:
                        done.append((u, live.pop(u)['parts']))
                if done:
                    self.check_status()       # one synchronisation per round that finishes an utterance
                for u, parts in done:
                    out = tuple(torch.cat([p[k] for p in parts]) for k in ((0, 1) if samples else (0,)))
                    yield (u,) + out
        finally:
            self.chunk_sz = keep_chunk

    def _vocode_rounds(self, mels, gc_ids, keys, lengths, rounds):
        """vocode's schedule on the built plan: one lbwn_gen_start, then per round its begins and its steps."""
        n_utt = len(mels)
        self.init_sessions()
        where = [None] * n_utt           # (slot, base) of every utterance
        idle = np.zeros((1, self.arch['n_lc_in']), np.float32)   # streams no utterance ever reaches
        for r, (steps, begins) in enumerate(rounds):
            slots = [s for s, _ in begins]
            ms = [mels[u] for _, u in begins]
            ks = [int(keys[u]) for _, u in begins]
            gs = [gc_ids[u] for _, u in begins] if gc_ids is not None else None
            if r == 0:
                for s in range(len(begins), self.batch_sz):
                    slots.append(s)
                    ms.append(idle)
                    ks.append(0)
                    if gs is not None:
                        gs.append(0)
            if slots:
                self.begin(slots, ms, gs, ks)
            for s, u in begins:
                where[u] = (s, self._base[s])
            self.step(steps)
        self.check_status()
        wav = self.tensor('wav').view(self.batch_sz, self.max_steps)
        return [wav[s, b0:b0 + lengths[u]].clone() for u, (s, b0) in enumerate(where)]
