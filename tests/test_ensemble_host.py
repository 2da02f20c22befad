"""CPU: the host side of N-sample ensembles - the restatement of the keyed draws against numpy.random.Philox, the C ABI declarations and
bindings of mud_randn_keyed / mud_ensemble_stats, their refusals before any launch, the host key checks and the drivers' flag rules."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

from conftest import REPO
import ensemble_ref as R

ENSEMBLE_SYMBOLS = ('mud_randn_keyed', 'mud_ensemble_stats')


def _numpy_block(ctr, key):
    c = ctr[0] + (ctr[1] << 64) + (ctr[2] << 128) + (ctr[3] << 192)
    g = np.random.Philox(key=key[0] + (key[1] << 64), counter=(c - 1) % (1 << 256))   # numpy increments (mod 2^256) before it generates
    return tuple(int(v) for v in g.random_raw(4))


def test_restatement_words_equal_numpy_philox():
    """Counters whose word 0 is 0 make numpy's decrement-then-increment carry across words; the others are plain blocks."""
    cases = [(0, 0, 0, 0, 0), (0, 1, 0, 0, 0), (0, 160, 7, 3, 2), (5, 0, 0, 0, 1), (16383, 99, (1 << 31) - 1, (1 << 24) - 1, 2),
             (0, (1 << 63) - 1, 12, 0, 1), (1 << 40, 3, 2, 9, 0)]
    for seed in (0, 1024, (1 << 64) - 1):
        for blk, s, j, step, kind in cases:
            ctr, key = R.counter(blk, s, j, step, kind), R.key(seed)
            assert R.philox4x64(ctr, key) == _numpy_block(ctr, key), (seed, blk, s, j, step, kind)
    # the counter layout of the issue: (e / 4, slice, (sample << 32) | (step << 8) | kind, 0) and the key (seed, 0x4D55444946460001)
    assert R.counter(3, 5, 2, 1, 2) == (3, 5, (2 << 32) | (1 << 8) | 2, 0)
    assert R.key(7) == (7, 0x4D55444946460001)


def test_restatement_normals_follow_the_definition():
    w = R.philox4x64(R.counter(0, 4, 1, 2, 1), R.key(11))
    got = R.randn_keyed([[4, 1]], 4, 11, 2, 1)[0]
    for lane in range(4):
        wa, wb = w[2 * (lane // 2)], w[2 * (lane // 2) + 1]
        r = math.sqrt(-2.0 * math.log(((wa >> 11) + 1) * 2.0 ** -53))
        th = 6.283185307179586 * ((wb >> 11) * 2.0 ** -53)
        assert got[lane] == np.float32(r * (math.cos(th) if lane % 2 == 0 else math.sin(th)))
    # a row of 6 ends inside its second block; the first 4 equal a row of 4
    six = R.randn_keyed([[4, 1]], 6, 11, 2, 1)[0]
    assert np.array_equal(six[:4], got)


def test_restatement_statistics_order_and_nan():
    rng = np.random.default_rng(0)
    x = rng.uniform(-1.5, 1.5, (2, 5, 3, 4)).astype(np.float32)
    x[1, 2, 0, 0] = np.nan
    m, s = R.ensemble_stats(x, 0.5, 0.5, 0.0, 1.0)
    assert np.isnan(m[1, 0, 0]) and np.isnan(s[1, 0, 0]) and np.isfinite(m[0]).all()
    y = np.clip(x[0].astype(np.float32) * np.float32(0.5) + np.float32(0.5), 0, 1).astype(np.float64)
    acc = 0.0
    for j in range(5):
        acc += y[j, 2, 3]
    assert m[0, 2, 3] == np.float32(acc / 5)
    assert (s[0] >= 0).all()


# ---------------------------------------------------------------------------------------------------
def test_ensemble_symbols_are_declared_and_bound():
    import mudiff_hip
    txt = open(os.path.join(REPO, 'include', 'mudiff_hip.h')).read()
    for name in ENSEMBLE_SYMBOLS:
        assert re.search(r'\b' + name + r'\s*\(', txt), name
        assert name in mudiff_hip._SIGNATURES and name in mudiff_hip.EXPORTED_SYMBOLS, name
    lib = mudiff_hip.load()
    assert lib.mud_version() >= 114
    for name in ENSEMBLE_SYMBOLS:
        assert getattr(lib, name).restype is C.c_int


def test_ensemble_entries_refuse_bad_arguments_before_any_launch():
    """Every refusal returns MUD_ERR_ARG (1) before a launch, so the checks run without a GPU."""
    import mudiff_hip
    lib = mudiff_hip.load()
    fake = C.c_void_p(1 << 20)                                # never dereferenced: the call is refused first
    ok = dict(out=fake, rows=2, row_len=8, keys=fake, seed=1, step=0, kind=0)
    bad = [(dict(out=None), 'null'), (dict(keys=None), 'null'), (dict(rows=-1), 'bad sizes'), (dict(row_len=0), 'bad sizes'),
           (dict(row_len=-4), 'bad sizes'), (dict(kind=3), 'kind'), (dict(kind=-1), 'kind'), (dict(step=-1), 'step'),
           (dict(step=1 << 24), 'step')]
    for change, msg in bad:
        a = dict(ok, **change)
        code = lib.mud_randn_keyed(a['out'], a['rows'], a['row_len'], a['keys'], a['seed'], a['step'], a['kind'], None)
        assert code == 1, change
        assert msg in lib.mud_last_error().decode(), (change, lib.mud_last_error())
    ok = dict(x=fake, n=2, N=3, hw=16, mean=fake, std=fake)
    bad = [(dict(x=None), 'null'), (dict(mean=None), 'null'), (dict(std=None), 'null'), (dict(n=-1), 'bad sizes'), (dict(hw=0), 'bad sizes'),
           (dict(N=1), 'N must be'), (dict(N=0), 'N must be'), (dict(N=-2), 'N must be')]
    for change, msg in bad:
        a = dict(ok, **change)
        code = lib.mud_ensemble_stats(a['x'], a['n'], a['N'], a['hw'], 1.0, 0.0, -math.inf, math.inf, a['mean'], a['std'], None)
        assert code == 1, change
        assert msg in lib.mud_last_error().decode(), (change, lib.mud_last_error())


def test_host_key_checks():
    from mudiff_hip import MudiffHipError, ops
    k = ops.check_keys(torch.tensor([[0, 0], [5, (1 << 31) - 1]]))
    assert k.dtype == torch.int64 and tuple(k.shape) == (2, 2)
    assert ops.check_keys(np.zeros((0, 2), np.int64)).shape == (0, 2)
    for keys, msg in (([[0, 1 << 31]], '2\\^31'), ([[0, -1]], '2\\^31'), ([[-1, 0]], 'slice'), ([[1, 2, 3]], 'rows, 2'), ([1, 2], 'rows, 2')):
        with pytest.raises(MudiffHipError, match=msg):
            ops.check_keys(torch.tensor(keys))
    with pytest.raises(MudiffHipError, match='seed'):
        ops._seed64(-1)
    with pytest.raises(MudiffHipError, match='seed'):
        ops._seed64(1 << 64)
    with pytest.raises(MudiffHipError, match='seed'):              # refused on the host, before any device is needed
        ops.randn_keyed(torch.tensor([[0, 0]]), 4, -5, 0, 0)


def test_default_chunk_bounds_the_sample_buffer():
    from mudiff_hip import ensemble
    assert ensemble.default_chunk(8, 256, 161) == 161
    assert ensemble.default_chunk(8, 256, 10 ** 6) * 4 * 8 * 256 * 256 <= ensemble.CHUNK_BYTES
    assert ensemble.default_chunk(8, 256, 10 ** 6) == 512
    assert ensemble.default_chunk(4096, 1024, 3) == 1            # never below one slice
    assert ensemble.premap(True) == (0.5, 0.5, 0.0, 1.0) and ensemble.premap(False)[:2] == (1.0, 0.0)


# ---------------------------------------------------------------------------------------------------
def test_driver_num_samples_flag_rules():
    from mudiff_hip import driver
    a = driver.parse_args([])
    assert a.num_samples is None and a.ensemble_seed == 1024             # absent: the default path (sample_slices) is taken
    a = driver.parse_args(['--device_metrics'])
    assert a.num_samples is None
    a = driver.parse_args(['--device_metrics', '--num_samples', '4', '--ensemble_seed', '7'])
    assert (a.num_samples, a.ensemble_seed) == (4, 7)
    a = driver.parse_args(['--device_metrics', '--num_samples', '2', '--lpips_weights', 'w.pth'])
    assert a.num_samples == 2
    with pytest.raises(SystemExit):
        driver.parse_args(['--device_metrics', '--num_samples', '1'])
    with pytest.raises(SystemExit):
        driver.parse_args(['--num_samples', '4'])
    with pytest.raises(SystemExit):
        driver.parse_args(['--device_metrics', '--num_samples', '4', '--ensemble_seed', '-1'])


def test_volume_num_samples_flag():
    from mudiff_hip import volume as V
    base = ['--target_modality', 'T1CE', '--output_dir', 'o', '--exp', 'e']
    assert V.build_argparser(base).num_samples is None
    assert V.build_argparser(base + ['--num_samples', '8']).num_samples == 8
    with pytest.raises(SystemExit):
        V.build_argparser(base + ['--num_samples', '1'])
