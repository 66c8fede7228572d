"""Temperature / top-k / top-p sampling of the cached generator, host side (no GPU): the two C-ABI
symbols (ABI still 5), their plan-state behaviour and refusals (no launch, no device), WaveNetGen's
keyword validation before any library call, the CLI flags, the float64 reference's own properties
(tests/sampling_ref.py), and that the inputs the GPU tests use exercise the filters without sitting
on near ties."""
import ctypes
import os
import re

import numpy as np
import pytest

from lbwn import _lib
from oracle import wavenet_ref as R
from tests import sampling_ref as S
from tests.conftest import ROOT

SMALL = dict(n_blocks=2, n_block_layers=4, n_quant=256, n_res=32, n_dil=32, n_skip=64, n_post=32,
             n_gc_embed=0, n_gc_category=0, use_bias=True)


def c_arch(arch=SMALL):
    a = _lib.Arch()
    for k in ('n_blocks', 'n_block_layers', 'n_quant', 'n_res', 'n_dil', 'n_skip', 'n_post', 'n_gc_embed',
              'n_gc_category'):
        setattr(a, k, int(arch[k]))
    a.use_bias = 1
    return a


def make_plan(lib, a, B=3, max_steps=64):
    h = ctypes.c_void_p()
    assert lib.lbwn_gen_plan_create(ctypes.byref(a), B, max_steps, 0, ctypes.byref(h)) == 0, lib.lbwn_last_error()
    return h


def get(lib, h):
    T, k, p = ctypes.c_float(-1), ctypes.c_int(-1), ctypes.c_float(-1)
    assert lib.lbwn_gen_get_sampling(h, ctypes.byref(T), ctypes.byref(k), ctypes.byref(p)) == 0
    return T.value, k.value, p.value


def test_sampling_symbols_exported_declared_abi_still_5():
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, 'include', 'lbwn.h')).read()
    code = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    for name in ('lbwn_gen_set_sampling', 'lbwn_gen_get_sampling'):
        assert hasattr(lib, name)
        assert name in _lib.EXPORTED
        assert re.search(r'\bint %s\s*\(' % name, code)
    assert re.search(r'#define LBWN_ABI_VERSION 5\b', hdr)
    assert lib.lbwn_abi_version() == 5 == _lib.ABI_VERSION


def test_sampling_plan_state_roundtrip_and_normalisation():
    lib = _lib.load()
    h = make_plan(lib, c_arch())
    ws0 = lib.lbwn_gen_workspace_bytes(h)
    assert get(lib, h) == (1.0, 0, 1.0)                       # the defaults of a fresh plan
    assert lib.lbwn_gen_set_sampling(h, 0.75, 40, 0.5) == 0
    assert get(lib, h) == (0.75, 40, 0.5)
    assert lib.lbwn_gen_set_sampling(h, 2.0, 255, 1.0) == 0
    assert get(lib, h) == (2.0, 255, 1.0)
    for k in (256, 256 + 5):                                  # top_k >= n_quant keeps every code: off
        assert lib.lbwn_gen_set_sampling(h, 0.75, k, 0.5) == 0
        assert get(lib, h) == (0.75, 0, 0.5)
    assert lib.lbwn_gen_workspace_bytes(h) == ws0
    # NULL outputs are skipped
    k = ctypes.c_int(-1)
    assert lib.lbwn_gen_get_sampling(h, None, ctypes.byref(k), None) == 0 and k.value == 0
    lib.lbwn_gen_plan_destroy(h)
    a100 = dict(SMALL, n_quant=100)
    h = make_plan(lib, c_arch(a100))
    assert lib.lbwn_gen_set_sampling(h, 1.0, 100, 1.0) == 0 and get(lib, h) == (1.0, 0, 1.0)
    assert lib.lbwn_gen_set_sampling(h, 1.0, 99, 1.0) == 0 and get(lib, h) == (1.0, 99, 1.0)
    lib.lbwn_gen_plan_destroy(h)


def test_sampling_refusals_name_the_argument_and_change_nothing():
    lib = _lib.load()
    h = make_plan(lib, c_arch())
    assert lib.lbwn_gen_set_sampling(h, 0.5, 7, 0.25) == 0
    nan, inf = float('nan'), float('inf')
    assert lib.lbwn_gen_set_sampling(None, 1.0, 0, 1.0) == 22 and b'plan' in lib.lbwn_last_error()
    T, k, p = ctypes.c_float(), ctypes.c_int(), ctypes.c_float()
    assert lib.lbwn_gen_get_sampling(None, ctypes.byref(T), ctypes.byref(k), ctypes.byref(p)) == 22
    assert b'plan' in lib.lbwn_last_error()
    for bad in (0.0, -1.0, nan, inf, -inf):
        assert lib.lbwn_gen_set_sampling(h, bad, 3, 0.9) == 22, bad
        assert b'temperature' in lib.lbwn_last_error()
        assert get(lib, h) == (0.5, 7, 0.25)
    for bad in (-1, -100):
        assert lib.lbwn_gen_set_sampling(h, 1.0, bad, 0.9) == 22, bad
        assert b'top_k' in lib.lbwn_last_error()
        assert get(lib, h) == (0.5, 7, 0.25)
    for bad in (nan, 0.0, -0.5, 1.0000001, 2.0, inf):
        assert lib.lbwn_gen_set_sampling(h, 1.0, 3, bad) == 22, bad
        assert b'top_p' in lib.lbwn_last_error()
        assert get(lib, h) == (0.5, 7, 0.25)
    lib.lbwn_gen_plan_destroy(h)


def make_host_gen(**kw):
    from lbwn.imodel import WaveNetGen
    return WaveNetGen(2, 4, 256, 32, 32, 64, 32, 0, 0, True, 3, 8, None, device='cpu', **kw)


class _Spy:
    """Stands in for the library: records every symbol looked up."""

    def __init__(self):
        self.called = []

    def __getattr__(self, name):
        self.called.append(name)
        return lambda *a: 0


def test_wavenetgen_sampling_keywords_validate_before_the_library(monkeypatch):
    spy = _Spy()
    monkeypatch.setattr(_lib, 'load', lambda *a, **k: spy)
    nan, inf = float('nan'), float('inf')
    bad = ([dict(temperature=v) for v in (0, -1.0, nan, inf, 'hot', None)]
           + [dict(top_k=v) for v in (-1, 2.5, '3', True, None)]
           + [dict(top_p=v) for v in (0, -0.1, 1.5, nan, None)])
    for kw in bad:
        with pytest.raises(ValueError, match=list(kw)[0]):
            make_host_gen(**kw)
    g = make_host_gen()
    assert g.sampling == (1.0, 0, 1.0)
    g = make_host_gen(temperature=0.8, top_k=40, top_p=0.95)
    assert g.sampling == (0.8, 40, 0.95)
    # positional use is not part of the interface
    with pytest.raises(TypeError):
        from lbwn.imodel import WaveNetGen
        WaveNetGen(2, 4, 256, 32, 32, 64, 32, 0, 0, True, 3, 8, None, True, 0, 'cpu', True, 0, 0, (), 0.8)
    for kw in bad:
        if list(kw.values())[0] is None:
            continue                                          # None keeps the value in set_sampling
        with pytest.raises(ValueError, match=list(kw)[0]):
            g.set_sampling(**kw)
        assert g.sampling == (0.8, 40, 0.95)
    assert not spy.called


def test_set_sampling_keeps_none_drops_the_graph_and_updates_the_plan(monkeypatch):
    spy = _Spy()
    monkeypatch.setattr(_lib, 'load', lambda *a, **k: spy)
    g = make_host_gen(temperature=0.8, top_k=40, top_p=0.95)
    g._graph = object()
    assert g.set_sampling(top_k=8) is g
    assert g.sampling == (0.8, 8, 0.95)
    assert g._graph is None
    assert not spy.called                                     # no plan yet: nothing to update
    g.set_sampling(temperature=1, top_p=1.0)
    assert g.sampling == (1.0, 8, 1.0)
    # with a plan, the values go to the library (and build_graph applies the constructor's)
    sent = []
    g._plan = ctypes.c_void_p(64)
    monkeypatch.setattr(g, 'lib', type('L', (), {'lbwn_gen_set_sampling': lambda s, *a: sent.append(a) or 0})())
    g._graph = object()
    g.set_sampling(0.5, 0, 0.9)
    assert sent == [(g._plan, 0.5, 0, 0.9)] and g._graph is None


def test_build_graph_applies_the_constructors_sampling():
    """On the real library (plan creation needs no device): build_graph leaves the keywords' values in
    the plan, and set_sampling replaces them."""
    lib = _lib.load()
    g = make_host_gen(temperature=0.5, top_k=300, top_p=0.75)
    g.build_graph(32)
    assert get(lib, g._plan) == (0.5, 0, 0.75)                # top_k >= n_quant: normalised by the library
    g.set_sampling(top_k=12)
    assert get(lib, g._plan) == (0.5, 12, 0.75)
    g.set_sampling(1, 0, 1)
    assert get(lib, g._plan) == (1.0, 0, 1.0)


def test_generate_cli_parses_and_checks_the_sampling_flags(capsys):
    import generate
    a = generate.get_args(['a', 'b', 'c'])
    assert (a.temperature, a.top_k, a.top_p) == (1.0, 0, 1.0)
    a = generate.get_args(['--temperature', '0.8', '--top-k', '40', '--top-p', '0.95', 'a', 'b', 'c'])
    assert (a.temperature, a.top_k, a.top_p) == (0.8, 40, 0.95)
    for flag, v in (('--temperature', '0'), ('--top-k', '-2'), ('--top-p', '1.5')):
        with pytest.raises(SystemExit) as ei:
            generate.main([flag, v, 'no_arch.json', 'no_ckpt', 'no_dir'])
        assert ei.value.code == 1
        assert flag[2:].replace('-', '_') in capsys.readouterr().err


# ---- the reference's own properties -------------------------------------------------------------

def _rows(n=200, Q=256, seed=11):
    rng = np.random.default_rng(seed)
    return [rng.normal(0, rng.uniform(0.5, 8), Q) for _ in range(n)]


def test_reference_nucleus_is_the_shortest_prefix():
    for i, lg in enumerate(_rows()):
        T, p = (0.7, 1.0, 1.5)[i % 3], (0.5, 0.9, 0.95, 0.999)[i % 4]
        e0 = np.exp((lg - lg.max()) / T)
        keep, e = S.keep_and_e(lg, T, 0, p)
        assert np.array_equal(e > 0, keep) and np.array_equal(e[keep], e0[keep])
        assert e.sum() >= p * e0.sum()                                    # the nucleus has mass >= p
        assert e0[keep & (e0 > e0[keep].min())].sum() < p * e0.sum()      # without its smallest e: below p
        assert e0[keep].min() >= e0[~keep].max() if (~keep).any() else True
    # ties with the prefix's last member are kept
    lg = np.log(np.array([0.4, 0.2, 0.2, 0.2]))
    assert S.keep_and_e(lg, 1.0, 0, 0.5)[0].tolist() == [True, True, True, True]
    assert S.keep_and_e(lg, 1.0, 0, 0.3)[0].tolist() == [True, False, False, False]


def test_reference_top_k_keeps_k_and_its_ties():
    for i, lg in enumerate(_rows()):
        k = (1, 2, 8, 40, 255)[i % 5]
        keep, e = S.keep_and_e(lg, 1.0, k, 1.0)
        assert keep.sum() == k                                            # continuous draws: no ties
        assert lg[keep].min() > lg[~keep].max()
        tied = lg.copy()
        tied[np.argsort(-lg)[k]] = np.sort(lg)[::-1][k - 1]               # the (k+1)-th ties the k-th
        assert S.keep_and_e(tied, 1.0, k, 1.0)[0].sum() == k + 1
        for kk in (0, 256, 300):
            assert S.keep_and_e(lg, 1.0, kk, 1.0)[0].all()
    assert S.ref_draw(np.array([0.1, 3.0, 2.9]), 0.999, 1.0, 1, 1.0) == 1     # greedy


def test_reference_neutral_is_sample_from_logits():
    rng = np.random.default_rng(5)
    for lg in _rows(300):
        u = rng.random()
        assert S.ref_draw(lg, u, 1.0, 0, 1.0) == R.sample_from_logits(lg, u)
        assert S.ref_draw(lg, u, 1.0, 256, 1.0) == R.sample_from_logits(lg, u)


# ---- the inputs earn their keep --------------------------------------------------------------------

@pytest.mark.parametrize('Q', [256, 100, 300])
def test_inputs_exercise_the_filters_away_from_near_ties(Q, monkeypatch):
    """Conditions on the GPU tests' inputs, not on the code under test: along the free-running filtered
    trajectory of each setting (B = 3, n = 64), at most 8 % of the 192 draws carry a near-tie flag, and
    the filtered draw differs from the unfiltered draw of the same logits at >= 10 % of them."""
    arch = S.small(Q)
    _, P = S.host_params(arch, S.POST2_SCALE[Q])
    B, n = 3, 64
    worst_flag, least_diff = 0, B * n
    for st in S.S_ALL:
        got, _, lg = S.filtered_generate(monkeypatch, arch, P, B, n, st)
        flagged = differ = 0
        for b in range(B):
            for i in range(n):
                u = R.philox_uniform(S.SEED, b, i)
                assert got[b, i] == S.ref_draw(lg[b, i], u, *st)
                flagged += bool(S.flags(lg[b, i], u, *st))
                differ += got[b, i] != R.sample_from_logits(lg[b, i], u)
        print('Q %d setting %s: flagged %d / %d, differing from the plain draw %d / %d, max |logit| %.2f'
              % (Q, st, flagged, B * n, differ, B * n, np.abs(lg).max()))
        worst_flag, least_diff = max(worst_flag, flagged), min(least_diff, differ)
    assert worst_flag <= 0.08 * B * n, worst_flag
    assert least_diff >= 0.10 * B * n, least_diff
