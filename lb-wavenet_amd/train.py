"""train.py drop-in (train.py:1-244 of the reference) on MI355X.

Same positional arguments (CKPT_PATH_PFX ARCH_FILE PAR_FILE SAMPLES_FILE) and flags; the
TF session/graph becomes WaveNetTrain's lbwn plan, the optimizer lbwn's TF1 Adam, the
dataset MaskedSliceWav.  Checkpoints: '<pfx>.net-<step>.safetensors' (model variables under
the reference serial names + Adam slots) and '<pfx>.dset-<step>.safetensors' (shuffle seed
and file position), at the reference's cadence (train.py:236-240).

Multi-GPU: launch with torch.distributed.run (one process per GPU); --batch-size is then
the per-GPU batch, the dealer runs over the global batch and each rank trains on its rows,
gradients are summed over ranks before the (replicated) Adam step (lbwn.dist).

Build extensions of the optimizer step, all decided on the device (lbwn_adam_ex): --clip-norm,
--skip-nonfinite, --ema-decay, --lr-warmup-steps, --lr-decay-steps, --lr-decay-rate, --log-grad-norm;
each overrides the PAR_FILE key of the same name (clip_norm, ..., log_grad_norm; all optional).  With
clipping or --log-grad-norm a second line follows each progress line:
grad_norm, scale, lr and nonfinite_skips of the last applied step.

Held-out evaluation (build extension, lbwn_train_eval): --valid-file names a second samples file; every
--valid-interval steps (default 1000; the loop's step number, the one --save-interval counts and names
checkpoints by, so a step that --skip-nonfinite left unapplied counts too), after the optimizer step, the
whole file (or its first --valid-batches slices) is dealt once through the same plan with an evaluation
state of its own, and rank 0 prints `valid <step> <nll> <bits> <top1> <avg_diff> <n>` (tab-separated) to
stderr and appends it to <CKPT_PATH_PFX>.valid.tsv; --valid-ema adds a `valid_ema` line for the EMA
shadows.  --eval-only (with --resume-step) restores, evaluates, prints and returns without a training
step.  PAR_FILE keys: valid_file, valid_interval, valid_batches, valid_ema.

Distillation and label smoothing (build extension, lbwn_train_forward_ex): --teacher-arch JSON
--teacher-ckpt PATH [--teacher-ema] load a second net whose logits of every slice are the soft targets;
--distill-alpha (default 0.5 with a teacher) weighs the soft term, --distill-temp (default 1) is its
temperature, --label-smoothing smooths the hard targets (with or without a teacher).  The dataset's
receptive field is then the larger of the two nets', checkpoints carry the teacher's lookback under
TEACHER/<save var>, and the progress line's total and mean are the objective that is optimised; with a
teacher two columns follow the existing ones: the plain xent and the KL (means over this rank's scored
positions).  --valid-file still reports the hard xent.  PAR_FILE keys: teacher_arch, teacher_ckpt,
teacher_ema, distill_alpha, distill_temp, label_smoothing.

TF-only switches are accepted for command-line compatibility: --tf-eager is implied,
--add-summary/--tb-dir/--prof-dir/--timeline-file print what replaces them (rocprofv3),
--tf-debug and --cpu-only exit(1) (there is no CPU execution path).
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
    p.add_argument('--timeline-file', '-tf', type=str, help='Enable profiling and write info to <timeline_file>')
    p.add_argument('--prof-dir', '-pd', type=str, metavar='DIR', help='Output profiling events to <prof_dir>')
    p.add_argument('--resume-step', '-rs', type=int, metavar='INT',
                   help='Resume training from CKPT_DIR/<ckpt_pfx>-<resume_step> checkpoints')
    p.add_argument('--add-summary', '-s', action='store_true', default=False,
                   help='If present, add summary histogram nodes to graph for TensorBoard')
    p.add_argument('--cpu-only', '-cpu', action='store_true', default=False,
                   help='If present, do all computation on CPU')
    p.add_argument('--tb-dir', '-tb', type=str, metavar='DIR', help='TensorBoard directory for summary events')
    p.add_argument('--save-interval', '-si', type=int, default=1000, metavar='INT',
                   help='Save a checkpoint after this many steps each time')
    p.add_argument('--progress-interval', '-pi', type=int, default=10, metavar='INT',
                   help='Print a progress message at this interval')
    p.add_argument('--tf-debug', '-tdb', action='store_true', default=False, help='Enable tf_debug debugging console')
    p.add_argument('--tf-eager', '-te', action='store_true', default=False, help='Enable tf Eager mode')
    p.add_argument('--max-steps', '-ms', type=int, default=int(1e20), help='Maximum number of training steps')
    p.add_argument('--batch-size', '-bs', type=int, metavar='INT', help='Batch size (overrides PAR_FILE setting)')
    p.add_argument('--slice-size', '-ss', type=int, metavar='INT', help='Slice size (overrides PAR_FILE setting)')
    p.add_argument('--l2-factor', '-l2', type=float, metavar='FLOAT', help='Loss = Xent loss + l2_factor * l2_loss')
    p.add_argument('--learning-rate', '-lr', type=float, metavar='FLOAT',
                   help='Learning rate (overrides PAR_FILE setting)')
    p.add_argument('--num-global-cond', '-gc', type=int, metavar='INT',
                   help='Number of global conditioning categories')
    p.add_argument('--seed', type=int, default=None, help='(build extension) weight / shuffle seed')
    p.add_argument('--clip-norm', type=float, metavar='FLOAT',
                   help='(build extension) clip the gradient to this global norm, on the device (0 = off)')
    p.add_argument('--skip-nonfinite', action='store_true', default=None,
                   help='(build extension) leave a step whose gradient norm is NaN/Inf unapplied and count it '
                        '(implied by --clip-norm)')
    p.add_argument('--ema-decay', type=float, metavar='FLOAT',
                   help='(build extension) keep an exponential moving average of the weights, decay in (0, 1); '
                        'saved as <var>/ExponentialMovingAverage (generate.py --ema)')
    p.add_argument('--lr-warmup-steps', type=int, metavar='INT',
                   help='(build extension) linear learning-rate warmup over this many Adam steps')
    p.add_argument('--lr-decay-steps', type=int, metavar='INT',
                   help='(build extension) exponential decay: lr * rate^(t / steps)')
    p.add_argument('--lr-decay-rate', type=float, metavar='FLOAT', help='(build extension) its rate, in (0, 1]')
    p.add_argument('--log-grad-norm', action='store_true', default=None,
                   help='(build extension) print the gradient norm with the progress line, without clipping')
    p.add_argument('--valid-file', type=str, metavar='SAMPLES',
                   help='(build extension) held-out samples file, evaluated every --valid-interval steps')
    p.add_argument('--valid-interval', type=int, metavar='INT',
                   help='(build extension) evaluate after the optimizer step of every INT-th step, counted like '
                        '--save-interval (default 1000)')
    p.add_argument('--valid-batches', type=int, metavar='INT',
                   help='(build extension) evaluate only the first INT slices of the deal (default: all)')
    p.add_argument('--valid-ema', action='store_true', default=None,
                   help='(build extension) also evaluate the EMA shadows (needs --ema-decay)')
    p.add_argument('--eval-only', action='store_true', default=False,
                   help='(build extension) restore --resume-step, evaluate --valid-file, print and exit')
    p.add_argument('--teacher-arch', type=str, metavar='JSON',
                   help='(build extension) ARCH_FILE of a teacher net to distil from (needs --teacher-ckpt)')
    p.add_argument('--teacher-ckpt', type=str, metavar='PATH',
                   help='(build extension) the teacher\'s checkpoint: a .safetensors file or a <pfx>-<step> prefix')
    p.add_argument('--teacher-ema', action='store_true', default=None,
                   help='(build extension) take the teacher\'s EMA shadows from the checkpoint')
    p.add_argument('--distill-alpha', type=float, metavar='FLOAT',
                   help='(build extension) weight of the soft term, in [0, 1] (default 0.5 with a teacher)')
    p.add_argument('--distill-temp', type=float, metavar='FLOAT',
                   help='(build extension) temperature of the soft term, > 0 (default 1)')
    p.add_argument('--label-smoothing', type=float, metavar='FLOAT',
                   help='(build extension) smooth the hard targets: (1-eps) one-hot + eps/n_quant, eps in [0, 1)')
    p.add_argument('ckpt_path', type=str, metavar='CKPT_PATH_PFX')
    p.add_argument('arch_file', type=str, metavar='ARCH_FILE')
    p.add_argument('par_file', type=str, metavar='PAR_FILE')
    p.add_argument('sam_file', type=str, metavar='SAMPLES_FILE')
    return p.parse_args(argv)


def prepare_arch(arch, num_global_cond):
    """The ARCH_FILE dict brought to WaveNetTrain's 14 keys; -gc may supply the
    n_gc_category the file lacks (train.py:77-80, :138-146: par/arch2.json, arch4.json).
    Errors print to stderr and exit(1), like the reference."""
    from lbwn.arch import ArchError, normalize_arch
    try:
        return normalize_arch(arch, num_global_cond=num_global_cond)
    except ArchError as e:
        print(str(e), file=sys.stderr)
        sys.exit(1)


OPT_KEYS = ('clip_norm', 'skip_nonfinite', 'ema_decay', 'lr_warmup_steps', 'lr_decay_steps', 'lr_decay_rate',
            'log_grad_norm')
VALID_KEYS = ('valid_file', 'valid_interval', 'valid_batches', 'valid_ema')
DISTILL_KEYS = ('teacher_arch', 'teacher_ckpt', 'teacher_ema', 'distill_alpha', 'distill_temp', 'label_smoothing')


def override_par(args, par):
    """Command-line values replace the PAR_FILE's keys of the same name (a flag not given leaves the key)."""
    for flag, key in (('batch_size', 'batch_sz'), ('slice_size', 'slice_sz'), ('l2_factor', 'l2_factor'),
                      ('learning_rate', 'learning_rate')) + tuple((k, k) for k in OPT_KEYS + VALID_KEYS + DISTILL_KEYS):
        if getattr(args, flag) is not None:
            par[key] = getattr(args, flag)
    return par


def optimizer_kwargs(par):
    """AdamOptimizer's arguments from the par dict; the optional keys are read with .get."""
    return dict(learning_rate=par['learning_rate'], clip_norm=par.get('clip_norm') or None,
                skip_nonfinite=bool(par.get('skip_nonfinite', False)), ema_decay=par.get('ema_decay') or None,
                warmup_steps=par.get('lr_warmup_steps', 0), decay_steps=par.get('lr_decay_steps', 0),
                decay_rate=par.get('lr_decay_rate', 1.0), log_norm=bool(par.get('log_grad_norm', False)))


def valid_options(par, eval_only=False):
    """The held-out evaluation's options from the par dict: None without a valid_file, else
    (file, interval, batches or None, ema).  Errors print to stderr and exit(1) like the others."""
    vf = par.get('valid_file')
    if not vf:
        given = [k for k in VALID_KEYS[1:] if par.get(k) is not None and par.get(k) is not False]
        if given or eval_only:
            print('Error: --{} needs --valid-file'.format((given + ['eval_only'])[0].replace('_', '-')), file=sys.stderr)
            sys.exit(1)
        return None
    interval = par.get('valid_interval')
    interval = int(interval) if interval is not None else 1000
    batches = par.get('valid_batches')
    if interval < 1 or (batches is not None and int(batches) < 1):
        print('Error: --valid-interval and --valid-batches must be >= 1', file=sys.stderr)
        sys.exit(1)
    ema = bool(par.get('valid_ema', False))
    if ema and not par.get('ema_decay'):
        print('Error: --valid-ema needs an EMA of the weights (--ema-decay)', file=sys.stderr)
        sys.exit(1)
    return vf, interval, int(batches) if batches is not None else None, ema


def distill_options(par, eval_only=False):
    """The distillation / label-smoothing options from the par dict:
    dict(teacher_arch, teacher_ckpt, teacher_ema, alpha, temp, smoothing), teacher_arch None without a
    teacher.  Errors print to stderr and exit(1) like the others, before a GPU is needed."""
    import math

    def fail(msg):
        print('Error: ' + msg, file=sys.stderr)
        sys.exit(1)

    ta, tc = par.get('teacher_arch'), par.get('teacher_ckpt')
    alpha, temp, eps = par.get('distill_alpha'), par.get('distill_temp'), par.get('label_smoothing')
    if tc and not ta:
        fail('--teacher-ckpt needs --teacher-arch')
    if ta and not tc:
        fail('--teacher-arch needs --teacher-ckpt')
    if not ta:
        if par.get('teacher_ema'):
            fail('--teacher-ema needs a teacher (--teacher-arch, --teacher-ckpt)')
        if alpha is not None and float(alpha) > 0:
            fail('--distill-alpha needs a teacher (--teacher-arch, --teacher-ckpt)')
        if temp is not None:
            fail('--distill-temp needs a teacher (--teacher-arch, --teacher-ckpt)')
    elif eval_only:
        fail('a teacher (--teacher-arch) cannot be combined with --eval-only: the evaluation scores the net alone')
    alpha = float(alpha) if alpha is not None else (0.5 if ta else 0.0)
    temp = float(temp) if temp is not None else 1.0
    eps = float(eps) if eps is not None else 0.0
    if not 0.0 <= alpha <= 1.0:
        fail('--distill-alpha must be in [0, 1]')
    if not (math.isfinite(temp) and temp > 0.0):
        fail('--distill-temp must be finite and > 0')
    if not 0.0 <= eps < 1.0:
        fail('--label-smoothing must be in [0, 1)')
    return dict(teacher_arch=ta or None, teacher_ckpt=tc or None, teacher_ema=bool(par.get('teacher_ema', False)),
                alpha=alpha, temp=temp, smoothing=eps)


def load_teacher(opts, num_global_cond, batch_sz, log):
    """The teacher net of --teacher-arch with the weights of --teacher-ckpt (its EMA shadows with
    --teacher-ema).  Its SAVE is not taken from that checkpoint: the distiller keeps its own."""
    from lbwn.ckpt import load_tensors
    from lbwn.optim import EMA_SUFFIX
    from lbwn.tmodel import WaveNetTrain
    import torch
    with open(opts['teacher_arch']) as fp:
        tarch = prepare_arch(json.load(fp), num_global_cond)
    teacher = WaveNetTrain(**tarch, batch_sz=batch_sz, l2_factor=0.0, print_interval=0)
    loaded = load_tensors(opts['teacher_ckpt'])
    suffix = EMA_SUFFIX if opts['teacher_ema'] else ''
    with torch.no_grad():
        for name, dst in teacher.vars.items():
            src = loaded.get(name + suffix)
            if src is None or tuple(src.shape) != tuple(dst.shape):
                print('Error: --teacher-ckpt {} {} {}{}'.format(
                    opts['teacher_ckpt'], 'lacks' if src is None else 'has another shape for', name, suffix), file=log)
                sys.exit(1)
            dst.copy_(src.to(dst.dtype))
    return teacher


def valid_files(sam_file, want_mel):
    """The held-out catalogue's files in catalogue order, loaded as they are dealt."""
    import numpy as np
    with open(sam_file) as fh:
        for line in fh:
            line = line.strip()
            if not line:
                continue
            vid, wav_path, mel_path = line.split('\t')
            yield int(vid), np.load(wav_path), (np.load(mel_path).astype(np.float32) if want_mel else None)


def main(argv=None):
    args = get_args(argv)
    from sys import stderr

    with open(args.arch_file) as fp:
        arch = json.load(fp)
    with open(args.par_file) as fp:
        par = json.load(fp)

    if args.num_global_cond is None and 'n_gc_category' not in arch:     # train.py:77-80
        print('Error: must provide n_gc_category in ARCH_FILE, or --num-global-cond', file=stderr)
        sys.exit(1)
    if args.tf_eager and args.tf_debug:
        print('Error: --tf-debug and --tf-eager cannot both be set', file=stderr)
        sys.exit(1)
    if args.tf_debug or args.cpu_only:
        print('Error: --tf-debug / --cpu-only have no equivalent here: the training step runs only as '
              'HIP kernels on an MI355X (liblbwn.so)', file=stderr)
        sys.exit(1)
    if args.add_summary and args.tb_dir is None:                           # train.py:206-210
        print('Error: must provide --tb-dir argument if there are summaries in the graph', file=stderr)
        sys.exit(1)
    for flag in ('timeline_file', 'prof_dir', 'tb_dir'):
        if getattr(args, flag):
            print('Note: --{} is a TF profiler/summary hook; profile this build with '
                  '`rocprofv3 --kernel-trace --stats -- python train.py ...`'.format(flag.replace('_', '-')),
                  file=stderr)

    override_par(args, par)
    valid = valid_options(par, args.eval_only)
    if args.eval_only and not args.resume_step:
        print('Error: --eval-only needs --resume-step', file=stderr)
        sys.exit(1)
    distill = distill_options(par, args.eval_only)

    import torch
    from lbwn import dist as lbdist
    from lbwn.arch import normalize_arch, mel_hop_sz as hop_of
    from lbwn.data import DeviceBatches, MaskedSliceWav, eval_batches
    from lbwn.optim import AdamOptimizer
    from lbwn.tmodel import WaveNetTrain

    arch = prepare_arch(arch, args.num_global_cond)
    dp = lbdist.init()
    hop = hop_of(arch)
    B = par['batch_sz']
    dset = MaskedSliceWav(None, args.sam_file, par['sample_rate'], par['slice_sz'], par['prefetch_sz'],
                          arch['n_lc_in'], hop, B * dp.world, par['n_keep_checkpoints'],
                          '{}.dset'.format(args.ckpt_path), args.resume_step or 0, random_seed=args.seed,
                          rows=dp.rows(B) if dp.enabled else None)
    dset.init_sample_catalog()
    if args.num_global_cond is not None:                                    # train.py:138-145
        if args.num_global_cond < dset.get_max_id():
            print('Error: --num-global-cond must be >= {}, the highest ID in the dataset.'.format(
                dset.get_max_id()), file=stderr)
            sys.exit(1)
        arch['n_gc_category'] = args.num_global_cond
        arch = normalize_arch(arch)

    net = WaveNetTrain(**arch, batch_sz=B, l2_factor=par['l2_factor'], add_summary=par.get('add_summary', False),
                       n_keep_checkpoints=par['n_keep_checkpoints'], ckpt_path='{}.net'.format(args.ckpt_path),
                       resume_step=args.resume_step or 0, n_valid_total=par.get('n_valid_total', 0),
                       print_interval=args.progress_interval if dp.rank == 0 else 0,
                       seed=args.seed if args.seed is not None else 0)
    net.dp = dp
    distiller = None
    if distill['teacher_arch']:
        from lbwn.distill import Distiller
        try:
            distiller = Distiller(net, load_teacher(distill, args.num_global_cond, B, stderr), distill['alpha'],
                                  distill['temp'], distill['smoothing'])
        except ValueError as e:
            print('Error: {}'.format(e), file=stderr)
            sys.exit(1)
    # with a teacher the invalid-window mask covers the deeper of the two nets
    dset.set_receptive_field_size(distiller.recep_field_sz() if distiller else net.get_recep_field_sz())
    dset.build()
    dset.init_vars()
    try:
        optimizer = AdamOptimizer(**optimizer_kwargs(par))
    except ValueError as e:
        print('Error: {}'.format(e), file=stderr)
        sys.exit(1)
    log_norm = optimizer.norm_pass and dp.rank == 0
    skips_seen = 0
    print('Built graph.', file=stderr)

    if args.resume_step:
        loaded = net.restore(optimizer)
        if distiller:
            distiller.load_state_tensors(loaded, log=stderr if dp.rank == 0 else open(os.devnull, 'w'))
        dset.restore()
        print('Restored net and dset from checkpoint', file=stderr)
        if log_norm:
            skips_seen = optimizer.nonfinite_skips(net)
    dp.broadcast_params(net)

    def validate(at_step):
        """One deal of the held-out file through an evaluation state of its own (net.evaluate);
        rank 0 prints and logs the line(s)."""
        import io
        import itertools
        vf, _, vbatches, vema = valid
        n_mel = arch['n_lc_in'] if arch['n_lc_out'] > 0 else 0
        flats = [('valid', None)] + ([('valid_ema', optimizer.ex_slots(net)['ema'])] if vema else [])
        for tag, flat in flats:
            deal = eval_batches(valid_files(vf, n_mel > 0), B * dp.world, dset.slice_sz, net.get_recep_field_sz(),
                                hop, n_mel, rows=dp.rows(B) if dp.enabled else None,
                                log=stderr if not validate.warned and dp.rank == 0 else io.StringIO())
            validate.warned = True   # the dealer's skipped-file warnings once, not per evaluation
            r = net.evaluate(itertools.islice(deal, vbatches), flat=flat)
            if dp.rank == 0:
                line = '%s\t%d\t%.6f\t%.6f\t%.6f\t%.4f\t%d' % (tag, at_step, r['nll'], r['bits'], r['top1'],
                                                                r['avg_diff'], r['n'])
                print(line, file=stderr)
                os.makedirs(os.path.dirname(os.path.abspath(args.ckpt_path)), exist_ok=True)
                with open('{}.valid.tsv'.format(args.ckpt_path), 'a') as fh:
                    fh.write(line + '\n')

    validate.warned = False
    if valid and arch['n_gc_embed'] > 0:
        with open(valid[0]) as fh:
            vmax = max([int(l.split('\t')[0]) for l in fh if l.strip()] or [0])
        if vmax > arch['n_gc_category']:
            print('Error: --valid-file has voice id {}, above n_gc_category {}'.format(vmax, arch['n_gc_category']),
                  file=stderr)
            sys.exit(1)
    if args.eval_only:
        validate(args.resume_step)
        return net

    print('Starting training...', file=stderr)
    step = args.resume_step or 1
    itr = DeviceBatches(dset.get_itr(), net.device)   # pinned buffers, non-blocking H2D: no per-step sync
    while step < args.max_steps:
        try:
            file_read_count, wav_input, mel_input, id_mask = next(itr)
        except StopIteration:
            break
        if distiller:
            distiller.step(wav_input, mel_input, id_mask, backward=True)
        else:
            net.forward(wav_input, mel_input, id_mask, backward=True, label_smoothing=distill['smoothing'])
        dp.reduce_grads(net)
        if args.progress_interval and net.global_step_host % args.progress_interval == 0:
            net.check_status()                # cumulative: any timed-out step since the start (never applied)
        net.maybe_print()                     # tmodel.py:272-281 prints before the step counters advance
        if (log_norm and args.progress_interval and net.global_step_host % args.progress_interval == 0
                and step > (args.resume_step or 1)):
            # the last applied step's norm; the progress line above has synchronised already
            info = optimizer.grad_info(net).tolist()
            skips = optimizer.nonfinite_skips(net)
            print('grad_norm\t%.4g\tscale\t%.4g\tlr\t%.4g\tnonfinite_skips\t%d' % (info[0], info[1], info[3], skips),
                  file=stderr)
            if skips > skips_seen:
                print('Warning: {} more step(s) had a non-finite gradient norm and were not applied'.format(
                    skips - skips_seen), file=stderr)
                skips_seen = skips
        optimizer.apply(net)
        if valid and step % valid[1] == 0:
            validate(step)
        if step % args.save_interval == 0 and step != args.resume_step:
            net.check_status()
            # collective under DP; with a teacher its SAVE rides along under TEACHER/
            net_save_path = net.save(step, optimizer, more=distiller.state_tensors() if distiller else None)
            if dp.rank == 0:
                dset_save_path = dset.save(step, file_read_count)
                print('Saved checkpoints to {} and {}'.format(net_save_path, dset_save_path), file=stderr)
        step += 1
    torch.cuda.synchronize()
    if step > (args.resume_step or 1):
        net.check_status()
    return net


if __name__ == '__main__':
    main()
