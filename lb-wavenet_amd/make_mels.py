"""make_mels.py ARCH_FILE PAR_FILE IN_LIST OUT_DIR OUT_CATALOG [--mel-config JSON]

Turns a list of recordings into the `vid \\t wav.npy \\t mel.npy` catalogue train.py reads, with the mel
computed on the device (lbwn.mel.MelSpectrogram; the reference made these files offline with librosa).

IN_LIST lines are `vid \\t path`; path is a .wav (read like generate.py's --teacher-wav and resampled to
PAR_FILE's sample_rate) or a float .npy already at that rate.  For each line: the wav trimmed to
frames·hop samples goes to OUT_DIR/audio/<name>.npy, its mel [frames, n_lc_in] to
OUT_DIR/mel/<name>.npy, and one line to OUT_CATALOG, so len(wav) == len(mel)·hop holds for every pair.
The audio is written as train.py reads it: int32 µ-law codes (ops.mu_encode_np of the signal clipped to
[-1, 1], ARCH_FILE's n_quant levels), for `wav_input_type: mu_law_quant`, the arch files' default.  The mel
is computed from the float signal.  An ARCH_FILE with `wav_input_type: raw` is refused: train.py's batches
carry the audio as int32, so a float file would train on all-zero samples.
hop and n_mels come from ARCH_FILE (mel_hop_sz, n_lc_in); the other settings are MelSpectrogram's
defaults unless --mel-config gives a JSON of them (its hop and n_mels must equal the arch's).  The
settings used are written once to OUT_DIR/mel_config.json, which generate.py --mel-config takes.
Files of equal length share a launch.  A file too short for one frame is skipped with a warning.
"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

MAX_BATCH = 16


def get_args(argv=None):
    p = argparse.ArgumentParser(description='wav list -> train.py catalogue with device-computed mels')
    p.add_argument('--mel-config', type=str, default=None, metavar='JSON',
                   help='mel settings (the keys of MelSpectrogram.config()); hop and n_mels must equal the arch\'s')
    p.add_argument('arch_file', type=str, metavar='ARCH_FILE')
    p.add_argument('par_file', type=str, metavar='PAR_FILE')
    p.add_argument('in_list', type=str, metavar='IN_LIST')
    p.add_argument('out_dir', type=str, metavar='OUT_DIR')
    p.add_argument('out_catalog', type=str, metavar='OUT_CATALOG')
    return p.parse_args(argv)


def read_list(path):
    items = []
    with open(path) as fh:
        for line in fh:
            line = line.strip()
            if line:
                vid, src = line.split('\t')
                items.append((int(vid), src))
    return items


def unique_names(items):
    """<name> of each line: the file's base name, numbered when two lines share one."""
    seen, names = {}, []
    for _, src in items:
        base = os.path.splitext(os.path.basename(src))[0]
        k = seen.get(base, 0)
        seen[base] = k + 1
        names.append(base if k == 0 else '{}.{}'.format(base, k))
    return names


def main(argv=None):
    args = get_args(argv)
    from sys import stderr
    import numpy as np
    from generate import load_teacher
    from lbwn.arch import mel_hop_sz, normalize_arch
    from lbwn.ops import mu_encode_np

    with open(args.arch_file) as fp:
        arch = normalize_arch(json.load(fp))
    with open(args.par_file) as fp:
        par = json.load(fp)
    if arch['n_lc_out'] == 0:
        print('ARCH_FILE has no local conditioning: there is no mel to make', file=stderr)
        sys.exit(1)
    if arch['wav_input_type'] != 'mu_law_quant':
        # train.py's batches carry the audio as int32 (lbwn.data.DeviceBatches): a float file would reach
        # the model as all-zero samples, so no catalogue is written that would train on silence
        print('ARCH_FILE has wav_input_type {!r}: make_mels.py writes mu-law codes, the form train.py\'s batches '
              'carry; use wav_input_type mu_law_quant'.format(arch['wav_input_type']), file=stderr)
        sys.exit(1)
    hop, n_mels, sr = mel_hop_sz(arch), arch['n_lc_in'], par['sample_rate']
    cfg = dict(sample_rate=sr, hop=hop, n_mels=n_mels)
    from lbwn.mel import MelSpectrogram, check_config
    if args.mel_config is not None:
        try:
            with open(args.mel_config) as fp:
                cfg = json.load(fp)
            check_config(cfg)
        except (OSError, ValueError) as e:               # unreadable, not JSON, or keys missing / unknown
            print('--mel-config {}: {}'.format(args.mel_config, e), file=stderr)
            sys.exit(1)
        if cfg['hop'] != hop or cfg['n_mels'] != n_mels:
            print('--mel-config {}: hop {} and n_mels {} do not match the arch (hop {}, n_lc_in {})'.format(
                args.mel_config, cfg['hop'], cfg['n_mels'], hop, n_mels), file=stderr)
            sys.exit(1)
        if cfg['sample_rate'] != sr:
            print('--mel-config {}: sample_rate {} is not PAR_FILE\'s {}'.format(
                args.mel_config, cfg['sample_rate'], sr), file=stderr)
            sys.exit(1)

    try:
        ms = MelSpectrogram.from_config(cfg)
    except (RuntimeError, ValueError, TypeError) as e:   # a setting the library refuses, or of the wrong type
        print('mel settings {}: {}'.format(cfg, e), file=stderr)
        sys.exit(1)
    items = read_list(args.in_list)
    names = unique_names(items)
    adir, mdir = os.path.join(args.out_dir, 'audio'), os.path.join(args.out_dir, 'mel')
    os.makedirs(adir, exist_ok=True)
    os.makedirs(mdir, exist_ok=True)
    with open(os.path.join(args.out_dir, 'mel_config.json'), 'w') as fp:
        json.dump(ms.config(), fp, indent=1, sort_keys=True)

    # load, trim to frames·hop, and group by length so equal lengths share a launch
    groups, order = {}, []
    for i, (vid, src) in enumerate(items):
        if src.endswith('.npy'):
            x = np.load(src).astype(np.float32)       # never allow_pickle
            if x.ndim != 1:
                print('Skipping {}: expected a mono [n] array, got shape {}'.format(src, x.shape), file=stderr)
                continue
        else:
            x = load_teacher(src, sr)
        F = ms.frames(len(x))
        if F < 1:
            print('Skipping {}: {} samples give no mel frame (needs more than n_fft/2 = {} and at least hop = {})'
                  .format(src, len(x), ms.n_fft // 2, hop), file=stderr)
            continue
        x = x[:F * hop]
        groups.setdefault(len(x), []).append((i, x))
        order.append(i)

    written = {}
    for n, members in groups.items():
        for s in range(0, len(members), MAX_BATCH):
            part = members[s:s + MAX_BATCH]
            mel = ms(np.stack([x for _, x in part])).cpu().numpy()
            for (i, x), m in zip(part, mel):
                wp = os.path.abspath(os.path.join(adir, names[i] + '.npy'))
                mp = os.path.abspath(os.path.join(mdir, names[i] + '.npy'))
                # the mel above is of the float signal; train.py reads codes (ops.py:23-28)
                x = mu_encode_np(np.clip(x.astype(np.float64), -1.0, 1.0), arch['n_quant']).astype(np.int32)
                np.save(wp, x, allow_pickle=False)
                np.save(mp, m, allow_pickle=False)
                assert len(x) == len(m) * hop
                written[i] = (items[i][0], wp, mp)
    with open(args.out_catalog, 'w') as fp:
        for i in order:
            fp.write('{}\t{}\t{}\n'.format(*written[i]))
    print('Wrote {} of {} files to {}'.format(len(written), len(items), args.out_catalog))
    return [written[i] for i in order]


if __name__ == '__main__':
    main()
