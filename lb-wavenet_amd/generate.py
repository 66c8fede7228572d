"""generate.py drop-in (generate.py:1-120 of the reference) on MI355X.

Same flags and positionals (ARCH_FILE CHECKPOINT_PREFIX OUTPUT_WAV_DIR).  The checkpoint is
a '<prefix>.safetensors' written by this build's train.py (reference serial names).  The TF
while_loop becomes WaveNetGen's device-resident generation (hipGraph-replayed chunks);
librosa (absent here) is replaced by scipy.io.wavfile for reading the teacher wav and
writing 'gen.i<k>.wav' (float32).  The reference hard-codes gc_ids = [5, 6]
(generate.py:94); --gc-ids overrides, and the list is cycled over the batch.  Archs with local
conditioning (the reference's generator has none) take their mel from --mel-npy, or compute it on the
device from a wav with --mel-from-wav (lbwn.mel.MelSpectrogram: n_fft 1024, Slaney, power 2, ln floor 1e-5
unless --mel-config names the mel_config.json that make_mels.py wrote).
--teacher-prefill (build extension, off by default) runs the teacher's steps as one parallel prefill;
the written wav then starts with the µ-law-quantised teacher instead of the draws the model made, and
ignored, during those steps.  With --mel-npy the prefilled steps are conditioned on the mel like the
sequential ones (upsampled row i-1 for step i).
--temperature / --top-k / --top-p (build extensions, defaults 1 / 0 / 1 = the plain softmax draw) filter
every step's draw: keep the top-k logits (ties kept), e = exp((l - max) / T), then the shortest
descending prefix with mass >= top-p; --top-k 1 is greedy decoding.
--prefill-fanout (build extension; implies the prefill path, needs --teacher-wav) prefills the teacher
once per distinct voice id and copies that state to every stream of the voice (WaveNetGen.run(...,
prefill='fanout')); with --mel-npy only the shared [frames, n_lc_in] shape.
--score-teacher (build extension; needs --teacher-wav, not with --prefill-fanout) handles the teacher as
--teacher-prefill does, but through WaveNetGen.score: it prints, per stream, the codes scored, the mean
-log p(code | history) in nats and the bits per sample to stderr, then generation continues as under
--teacher-prefill.  --score-npy PATH saves the [batch, n] float32 log-probabilities.
--ema (build extension) loads every variable from its exponential moving average in the checkpoint
(train.py --ema-decay); a checkpoint without them is an error.
--mel-list LIST (build extension, LC archs only) vocodes a list: every line is "vid<TAB>mel.npy[<TAB>name]",
and OUTPUT_WAV_DIR/<name>.wav gets frames x hop samples for every line (WaveNetGen.vocode: a stream of the
batch takes the next utterance as soon as its own is covered; the draw key is the line's position, so a wav
does not depend on --batch-size).  A list whose outputs, upsampled mels and upsample scratch would exceed
--mel-list-budget-mb on the device is vocoded in consecutive groups.
"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)


def get_args(argv=None):
    p = argparse.ArgumentParser(description='WaveNet')
    p.add_argument('--teacher-wav', '-w', type=str,
                   help='Provide a preliminary teacher-forcing vector to prime the generation')
    p.add_argument('--teacher-prefill', action='store_true',
                   help='(build extension) run the teacher\'s steps as one parallel prefill instead of '
                        'one step at a time; the written wav then starts with the mu-law-quantised teacher '
                        '(without it: with the draws the model made, and ignored, during those steps)')
    p.add_argument('--prefill-fanout', action='store_true',
                   help='(build extension) prefill the teacher once per distinct voice id and fan the state '
                        'out to the batch (implies the prefill path; needs --teacher-wav; --mel-npy must be '
                        'the shared [frames, n_lc_in] shape)')
    p.add_argument('--score-teacher', action='store_true',
                   help='(build extension) as --teacher-prefill, and print per stream the mean -log p of the '
                        'teacher\'s codes under the model (nats, and bits per sample) to stderr; needs '
                        '--teacher-wav, not with --prefill-fanout')
    p.add_argument('--score-npy', type=str, default=None, metavar='PATH',
                   help='(build extension) with --score-teacher: save the [batch, n] float32 log-probabilities')
    p.add_argument('--teacher-start', '-ts', type=float, help='Number of seconds to parse from <teacher_wav>')
    p.add_argument('--teacher-duration', '-td', type=float, help='Number of seconds to parse from <teacher_wav>')
    p.add_argument('--gen-seconds', '-g', type=float, default=5, help='Number of additional seconds to generate')
    p.add_argument('--sample-rate', '-s', type=int, default=16000,
                   help='Number of samples per second for parsed .wav files')
    p.add_argument('--chunk-size', '-c', type=int, default=1000,
                   help='Number of timesteps to generate between internal buffer shifts')
    p.add_argument('--batch-size', '-b', type=int, default=10, help='Number of .wav files to generate simultaneously')
    p.add_argument('--gc-ids', type=str, default='5,6', help='(build extension) voice ids, cycled over the batch')
    p.add_argument('--seed', type=int, default=0, help='(build extension) sampling seed')
    p.add_argument('--mel-npy', type=str, default=None, metavar='PATH',
                   help='(build extension) local conditioning for LC archs: a .npy of [frames, n_lc_in] '
                        '(shared by the batch) or [batch, frames, n_lc_in].  Upsampled mel row i-1 conditions '
                        'step i, counted from the start of the teacher (step 0 uses row 0), so it must hold '
                        'at least (steps - 1) / hop frames for the gen_seconds + teacher seconds requested')
    p.add_argument('--mel-from-wav', type=str, default=None, metavar='PATH',
                   help='(build extension) local conditioning for LC archs computed on the device from this wav '
                        '(read like --teacher-wav; --teacher-start / --teacher-duration apply when PATH is also '
                        'the --teacher-wav); used as the shared [frames, n_lc_in] mel; not with --mel-npy')
    p.add_argument('--mel-config', type=str, default=None, metavar='JSON',
                   help='(build extension) with --mel-from-wav: the mel_config.json make_mels.py wrote; its hop '
                        'and n_mels must equal the arch\'s')
    p.add_argument('--mel-list', type=str, default=None, metavar='LIST',
                   help='(build extension) vocode a list: every LIST line is "vid<TAB>mel.npy[<TAB>name]" (voice '
                        'id, a .npy of [frames, n_lc_in], the output name; default: the mel file\'s stem); writes '
                        'OUTPUT_WAV_DIR/<name>.wav of frames x hop samples for every line.  The batch\'s streams '
                        'are recycled as utterances end (WaveNetGen.vocode); --gen-seconds, the teacher options '
                        'and --mel-npy / --mel-from-wav do not apply')
    p.add_argument('--mel-list-budget-mb', type=float, default=4096.0, metavar='MB',
                   help='(build extension) with --mel-list: the most the outputs, the upsampled mels and the '
                        'upsample stages\' scratch of one run may take on the device; a longer list is vocoded '
                        'in consecutive groups')
    p.add_argument('--mel-list-ring', type=int, default=0, metavar='STEPS',
                   help='(build extension) with --mel-list: vocode the whole list in one continuous schedule on a '
                        'ring plan whose outputs and upsampled mels hold STEPS steps per stream (>= --chunk-size), '
                        'whatever the list\'s length: no groups, --mel-list-budget-mb does not apply, and every '
                        'wav is written as its utterance completes (0 = off)')
    p.add_argument('--temperature', type=float, default=1.0,
                   help='(build extension) softmax temperature of the draw, finite and > 0 (1 = off)')
    p.add_argument('--top-k', type=int, default=0,
                   help='(build extension) draw among the k most likely codes, ties with the k-th kept '
                        '(0 = off, 1 = greedy)')
    p.add_argument('--top-p', type=float, default=1.0,
                   help='(build extension) nucleus sampling: draw among the most likely codes whose mass '
                        'reaches p, in (0, 1] (1 = off); applied after --top-k')
    p.add_argument('--ema', action='store_true',
                   help='(build extension) generate from the averaged weights the checkpoint holds '
                        '(<var>/ExponentialMovingAverage, written by train.py --ema-decay)')
    p.add_argument('arch_file', type=str, metavar='ARCH_FILE')
    p.add_argument('ckpt', metavar='CHECKPOINT_PREFIX', type=str)
    p.add_argument('wav_dir', metavar='OUTPUT_WAV_DIR', type=str)
    return p.parse_args(argv)


def load_teacher(path, sample_rate, start=None, duration=None):
    """librosa.load(path, sr, offset, duration, mono=True) restated with scipy: float in
    [-1, 1], mono mix, polyphase resampling to sample_rate."""
    import numpy as np
    from math import gcd
    from scipy.io import wavfile
    from scipy.signal import resample_poly
    sr, x = wavfile.read(path)
    if x.dtype.kind == 'i':
        x = x.astype(np.float32) / float(np.iinfo(x.dtype).max + 1)
    elif x.dtype.kind == 'u':
        x = (x.astype(np.float32) - 128.0) / 128.0
    x = x.astype(np.float32)
    if x.ndim > 1:
        x = x.mean(axis=1)
    if start:
        x = x[int(round(start * sr)):]
    if duration is not None:
        x = x[:int(round(duration * sr))]
    if sr != sample_rate:
        g = gcd(sr, sample_rate)
        x = resample_poly(x, sample_rate // g, sr // g).astype(np.float32)
    return x


def mel_list_bytes(total, batch_sz, n_lc_out, lc_upsample):
    """Device bytes a session run of ``total`` steps holds per plan in "samples", "wav" (4 bytes per stream
    and step each), "lc" (ceil(total / hop) frames x hop rows of n_lc_out floats per stream) and the
    upsample stack's scratch (the output of every stage before the last: frames x the product of the
    strides so far rows of n_lc_out floats per stream)."""
    hop = 1
    for s in lc_upsample:
        hop *= int(s)
    frames = -(-total // hop)
    rows, r = frames * hop, frames
    for s in list(lc_upsample)[:-1]:
        r *= int(s)
        rows += r
    return batch_sz * (8 * total + 4 * n_lc_out * rows)


def mel_list_groups(lengths, batch_sz, chunk, n_lc_out, lc_upsample, budget):
    """Consecutive groups of utterance indices, each as long as its schedule (plan_sessions) keeps
    mel_list_bytes within ``budget``; an utterance that alone exceeds it is a group of its own."""
    from lbwn.imodel import plan_sessions
    groups, cur = [], []
    for u in range(len(lengths)):
        total = plan_sessions([lengths[v] for v in cur + [u]], batch_sz, chunk)[1]
        if cur and mel_list_bytes(total, batch_sz, n_lc_out, lc_upsample) > budget:
            groups.append(cur)
            cur = []
        cur.append(u)
    if cur:
        groups.append(cur)
    return groups


def read_mel_list(path, n_lc_in, n_gc_category):
    """[(voice id, mel [frames, n_lc_in] float32, name)] of a --mel-list file; ValueError naming the line."""
    import numpy as np
    out, names = [], set()
    with open(path) as fp:
        for ln, line in enumerate(fp, 1):
            line = line.rstrip('\n')
            if not line.strip():
                continue
            f = line.split('\t')
            if len(f) not in (2, 3):
                raise ValueError('line %d: expected "vid<TAB>mel.npy[<TAB>name]", got %r' % (ln, line))
            try:
                vid = int(f[0])
            except ValueError:
                raise ValueError('line %d: voice id %r is not an integer' % (ln, f[0]))
            if n_gc_category and not 0 <= vid <= n_gc_category:
                raise ValueError('line %d: voice id %d is outside [0, %d]' % (ln, vid, n_gc_category))
            try:
                mel = np.load(f[1], allow_pickle=False)
            except (OSError, ValueError) as e:
                raise ValueError('line %d: cannot read mel %s: %s' % (ln, f[1], e))
            if mel.ndim != 2 or mel.shape[1] != n_lc_in or mel.shape[0] < 1:
                raise ValueError('line %d: mel %s has shape %s, expected [frames, %d]'
                                 % (ln, f[1], tuple(mel.shape), n_lc_in))
            name = f[2].strip() if len(f) == 3 and f[2].strip() else os.path.splitext(os.path.basename(f[1]))[0]
            if name in names or os.sep in name:
                raise ValueError('line %d: output name %r is taken by an earlier line or is not a file name'
                                 % (ln, name))
            names.add(name)
            out.append((vid, np.ascontiguousarray(mel, np.float32), name))
    if not out:
        raise ValueError('no utterances listed')
    return out


def main_mel_list(args, arch):
    """--mel-list: vocode every line of the list through WaveNetGen.vocode, one wav per line."""
    from sys import stderr
    import numpy as np
    from lbwn.arch import mel_hop_sz
    from lbwn.ckpt import ckpt_file
    from lbwn.imodel import WaveNetGen
    if args.mel_npy is not None or args.mel_from_wav is not None or args.teacher_wav is not None:
        print('--mel-list takes its mels from LIST: not with --mel-npy, --mel-from-wav or --teacher-wav',
              file=stderr)
        sys.exit(1)
    if arch['n_lc_out'] == 0:
        print('--mel-list: ARCH_FILE has no local conditioning, there is nothing to vocode from', file=stderr)
        sys.exit(1)
    if not os.access(args.mel_list, os.R_OK):
        print("Couldn't find mel list {}".format(args.mel_list), file=stderr)
        sys.exit(1)
    try:
        utts = read_mel_list(args.mel_list, arch['n_lc_in'], arch['n_gc_category'] if arch['n_gc_embed'] else 0)
    except ValueError as e:
        print('--mel-list {}: {}'.format(args.mel_list, e), file=stderr)
        sys.exit(1)
    if not os.access(ckpt_file(args.ckpt), os.R_OK):
        print("Couldn't find checkpoint file {}".format(ckpt_file(args.ckpt)), file=stderr)
        sys.exit(1)
    ring = int(args.mel_list_ring)
    if ring < 0 or 0 < ring < args.chunk_size:
        print('--mel-list-ring {}: must be 0 (off) or at least --chunk-size {}'.format(ring, args.chunk_size),
              file=stderr)
        sys.exit(1)
    hop = mel_hop_sz(arch)
    lengths = [m.shape[0] * hop for _, m, _ in utts]
    groups = [] if ring else mel_list_groups(lengths, args.batch_size, args.chunk_size, arch['n_lc_out'],
                                             arch['lc_upsample'], int(args.mel_list_budget_mb * 2 ** 20))
    net = WaveNetGen(arch['n_blocks'], arch['n_block_layers'], arch['n_quant'], arch['n_res'], arch['n_dil'],
                     arch['n_skip'], arch['n_post'], arch['n_gc_embed'], arch['n_gc_category'], arch['use_bias'],
                     args.batch_size, args.chunk_size, None, seed=args.seed, n_lc_in=arch['n_lc_in'],
                     n_lc_out=arch['n_lc_out'], lc_upsample=arch['lc_upsample'], temperature=args.temperature,
                     top_k=args.top_k, top_p=args.top_p, ring_steps=ring)
    print('Restoring from {}'.format(args.ckpt))
    try:
        net.restore(args.ckpt, ema=args.ema)
    except ValueError as e:
        if not args.ema:
            raise
        print('--ema: {}'.format(e), file=stderr)
        sys.exit(1)
    from scipy.io import wavfile
    os.makedirs(args.wav_dir, exist_ok=True)
    if ring:
        # one ring schedule for the whole list (WaveNetGen.vocode_iter): keys = the list positions, as below
        print('Vocoding {} utterances in one ring schedule of {} steps.'.format(len(utts), ring))
        wavs = [None] * len(utts)
        gcs = [v for v, _, _ in utts] if arch['n_gc_embed'] else None
        for u, w in net.vocode_iter((m for _, m, _ in utts), gc_ids=gcs):
            wavs[u] = w.cpu().numpy().astype(np.float32)
            path = os.path.join(args.wav_dir, utts[u][2] + '.wav')
            wavfile.write(path, args.sample_rate, wavs[u])
            print('Wrote {}'.format(path))
        print('Finished.')
        return wavs
    print('Vocoding {} utterances in {} group(s).'.format(len(utts), len(groups)))
    wavs = [None] * len(utts)
    for grp in groups:
        # the draw keys are the list positions: a wav does not depend on the batch size or the grouping
        out = net.vocode([utts[u][1] for u in grp], gc_ids=[utts[u][0] for u in grp] if arch['n_gc_embed'] else None,
                         keys=grp)
        for u, w in zip(grp, out):
            wavs[u] = w.cpu().numpy().astype(np.float32)
            path = os.path.join(args.wav_dir, utts[u][2] + '.wav')
            wavfile.write(path, args.sample_rate, wavs[u])
            print('Wrote {}'.format(path))
    print('Finished.')
    return wavs


def main(argv=None):
    args = get_args(argv)
    from sys import stderr
    import numpy as np
    import torch
    from lbwn.arch import mel_hop_sz, normalize_arch
    from lbwn.ckpt import ckpt_file
    from lbwn.imodel import WaveNetGen

    try:
        WaveNetGen._check_sampling(args.temperature, args.top_k, args.top_p)
    except ValueError as e:
        print('Bad sampling option: {}'.format(e), file=stderr)
        sys.exit(1)
    if args.prefill_fanout and args.teacher_wav is None:
        print('--prefill-fanout needs --teacher-wav: there is no prompt to prefill', file=stderr)
        sys.exit(1)
    if args.score_teacher and args.teacher_wav is None:
        print('--score-teacher needs --teacher-wav: there is no waveform to score', file=stderr)
        sys.exit(1)
    if args.score_teacher and args.prefill_fanout:
        print('--score-teacher scores every stream: it cannot be combined with --prefill-fanout', file=stderr)
        sys.exit(1)
    if args.score_npy is not None and not args.score_teacher:
        print('--score-npy needs --score-teacher', file=stderr)
        sys.exit(1)
    if args.mel_from_wav is not None and args.mel_npy is not None:
        print('--mel-from-wav and --mel-npy both give the mel: pass one of them', file=stderr)
        sys.exit(1)
    if args.mel_config is not None and args.mel_from_wav is None:
        print('--mel-config needs --mel-from-wav', file=stderr)
        sys.exit(1)
    with open(args.arch_file) as fp:
        arch = normalize_arch(json.load(fp))
    if args.mel_list is not None:
        return main_mel_list(args, arch)
    mel_cfg = None
    if args.mel_from_wav is not None:
        if arch['n_lc_out'] == 0:
            print('--mel-from-wav: ARCH_FILE has no local conditioning', file=stderr)
            sys.exit(1)
        mel_cfg = dict(sample_rate=args.sample_rate, hop=mel_hop_sz(arch), n_mels=arch['n_lc_in'])
        if args.mel_config is not None:
            from lbwn.mel import check_config
            try:
                with open(args.mel_config) as fp:
                    mel_cfg = json.load(fp)
                check_config(mel_cfg)
            except (OSError, ValueError) as e:           # unreadable, not JSON, or keys missing / unknown
                print('--mel-config {}: {}'.format(args.mel_config, e), file=stderr)
                sys.exit(1)
            if mel_cfg['hop'] != mel_hop_sz(arch) or mel_cfg['n_mels'] != arch['n_lc_in']:
                print('--mel-config {}: hop {} and n_mels {} do not match the arch (hop {}, n_lc_in {})'.format(
                    args.mel_config, mel_cfg['hop'], mel_cfg['n_mels'], mel_hop_sz(arch), arch['n_lc_in']),
                    file=stderr)
                sys.exit(1)
            if mel_cfg['sample_rate'] != args.sample_rate:
                print('--mel-config {}: sample_rate {} is not --sample-rate {}'.format(
                    args.mel_config, mel_cfg['sample_rate'], args.sample_rate), file=stderr)
                sys.exit(1)
    if not os.access(ckpt_file(args.ckpt), os.R_OK):                   # generate.py:43-47
        print("Couldn't find checkpoint file {}".format(ckpt_file(args.ckpt)), file=stderr)
        sys.exit(1)
    if args.teacher_wav is not None:
        teacher_vec = load_teacher(args.teacher_wav, args.sample_rate, args.teacher_start, args.teacher_duration)
        teacher_seconds = teacher_vec.shape[0] / args.sample_rate
    else:
        teacher_vec, teacher_seconds = None, 0

    gen_sz = int((args.gen_seconds + teacher_seconds) * args.sample_rate)
    mel = None
    if arch['n_lc_out'] > 0:
        if args.mel_npy is None and args.mel_from_wav is None:
            print('ARCH_FILE has local conditioning: --mel-npy is required', file=stderr)
            sys.exit(1)
        if args.mel_from_wav is not None:
            if not os.access(args.mel_from_wav, os.R_OK):
                print("Couldn't find wav file {}".format(args.mel_from_wav), file=stderr)
                sys.exit(1)
            from lbwn.mel import MelSpectrogram
            same = args.mel_from_wav == args.teacher_wav
            mel_wav = load_teacher(args.mel_from_wav, args.sample_rate, args.teacher_start if same else None,
                                   args.teacher_duration if same else None)
            try:
                mel = MelSpectrogram.from_config(mel_cfg)(mel_wav).cpu().numpy()
            except (RuntimeError, ValueError, TypeError) as e:     # a setting the library refuses
                                                                   # (LbwnError), or of the wrong type
                print('--mel-from-wav {}: {}'.format(args.mel_from_wav, e), file=stderr)
                sys.exit(1)
        else:
            if not os.access(args.mel_npy, os.R_OK):
                print("Couldn't find mel file {}".format(args.mel_npy), file=stderr)
                sys.exit(1)
            mel = np.load(args.mel_npy)
        hop = mel_hop_sz(arch)
        if mel.ndim not in (2, 3) or gen_sz > mel.shape[-2] * hop + 1:
            print('mel {} is too short: {} steps ({} s generated + {} s teacher) need {} frames of hop {}'.format(
                tuple(mel.shape), gen_sz, args.gen_seconds, teacher_seconds, -(-(gen_sz - 1) // hop), hop),
                file=stderr)
            sys.exit(1)
        if args.prefill_fanout and mel.ndim != 2:
            print('--prefill-fanout takes the shared mel shape [frames, n_lc_in] only, got {}'.format(
                tuple(mel.shape)), file=stderr)
            sys.exit(1)

    net = WaveNetGen(arch['n_blocks'], arch['n_block_layers'], arch['n_quant'], arch['n_res'], arch['n_dil'],
                     arch['n_skip'], arch['n_post'], arch['n_gc_embed'], arch['n_gc_category'], arch['use_bias'],
                     args.batch_size, args.chunk_size, teacher_vec, seed=args.seed, n_lc_in=arch['n_lc_in'],
                     n_lc_out=arch['n_lc_out'], lc_upsample=arch['lc_upsample'], temperature=args.temperature,
                     top_k=args.top_k, top_p=args.top_p)
    print('Building graph.')
    print('Restoring from {}'.format(args.ckpt))
    try:
        net.restore(args.ckpt, ema=args.ema)
    except ValueError as e:
        if not args.ema:
            raise
        print('--ema: {}'.format(e), file=stderr)
        sys.exit(1)
    print('Initializing buffers.')
    ids = [int(v) for v in args.gc_ids.split(',') if v.strip()]
    gc_ids = [ids[i % len(ids)] for i in range(args.batch_size)] if arch['n_gc_embed'] else None
    print('Starting inference...')
    mode = 'fanout' if args.prefill_fanout else 'score' if args.score_teacher else args.teacher_prefill
    n, wav_streams, wpos = net.run(gen_sz, gc_ids=gc_ids, mel=mel, prefill=mode)
    if args.score_teacher:
        logp = net.teacher_logp.cpu().numpy()
        for i in range(args.batch_size):
            nats = -float(logp[i].mean())
            print('score stream {}: {} codes, mean -logp {:.6f} nats, {:.6f} bits per sample'.format(
                i, logp.shape[1], nats, nats / np.log(2.0)), file=stderr)
        if args.score_npy is not None:
            np.save(args.score_npy, logp.astype(np.float32), allow_pickle=False)
    wav_streams = wav_streams.cpu().numpy()

    from scipy.io import wavfile
    print('Writing wav files.')
    os.makedirs(args.wav_dir, exist_ok=True)
    for i in range(args.batch_size):
        path = os.path.join(args.wav_dir, 'gen.i{}.wav'.format(i))
        wavfile.write(path, args.sample_rate, wav_streams[i].astype(np.float32))
        print('Wrote {}'.format(path))
    print('Finished.')
    return wav_streams


if __name__ == '__main__':
    main()
