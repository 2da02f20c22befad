"""CPU: sampling with a partly acquired target (csrc/known_region.hip, mudiff_hip.known_region): the refusals of
the two C entries before any launch, the numpy restatement's own sanity, the sampler's and the wrappers' argument checks."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from conftest import REPO
import known_region_ref as R

SYMBOLS = ('mud_known_constrain', 'mud_known_coverage')


def test_symbols_are_declared_and_bound():
    import mudiff_hip
    from mudiff_hip import ops
    txt = open(os.path.join(REPO, 'include', 'mudiff_hip.h')).read()
    for name in SYMBOLS:
        assert re.search(r'\b' + name + r'\s*\(', txt), name
        assert name in mudiff_hip._SIGNATURES and name in mudiff_hip.EXPORTED_SYMBOLS, name
    lib = mudiff_hip.load()
    assert lib.mud_version() >= 120
    assert (ops.KIND_X_INIT, ops.KIND_Z, ops.KIND_NOISE, ops.KIND_KNOWN, ops.KIND_RENOISE) == (0, 1, 2, 3, 4)
    readme = open(os.path.join(REPO, 'README.md')).read()
    assert f'C ABI ({len(mudiff_hip.EXPORTED_SYMBOLS)} entry points)' in readme


def _constrain(lib, a):
    return lib.mud_known_constrain(a['x_new'], a['known'], a['mask'], a['noise'], a['keys'], a['seed'], a['step'], a['kind'], a['t'], a['toff'],
                                   a['a_tab'], a['s_tab'], a['ntab'], a['clean'], a['out'], a['rows'], a['row_len'], None)


def test_constrain_refuses_bad_arguments_before_any_launch():
    """Every refusal returns MUD_ERR_ARG (1) before a launch, so the checks run without a GPU."""
    import mudiff_hip
    lib = mudiff_hip.load()
    fake = C.c_void_p(1 << 20)                                # never dereferenced: the call is refused first
    ok = dict(x_new=fake, known=fake, mask=fake, noise=None, keys=fake, seed=1, step=0, kind=3, t=fake, toff=0, a_tab=fake, s_tab=fake, ntab=5,
              clean=0, out=fake, rows=2, row_len=8)
    bad = [(dict(known=None), 'null'), (dict(out=None), 'null'), (dict(x_new=None), 'null'), (dict(t=None), 'null'), (dict(a_tab=None), 'null'),
           (dict(s_tab=None), 'null'), (dict(rows=0), 'bad sizes'), (dict(rows=-1), 'bad sizes'), (dict(row_len=0), 'bad sizes'),
           (dict(row_len=-4), 'bad sizes'), (dict(ntab=0), 'ntab'), (dict(ntab=-3), 'ntab'), (dict(kind=16), 'kind'), (dict(kind=-1), 'kind'),
           (dict(step=-1), 'step'), (dict(step=1 << 24), 'step'), (dict(keys=None), 'keys'), (dict(keys=None, mask=None, x_new=None), 'keys')]
    for change, msg in bad:
        assert _constrain(lib, dict(ok, **change)) == 1, change
        assert msg in lib.mud_last_error().decode(), (change, lib.mud_last_error())
    # mud_randn_keyed itself keeps refusing the new kinds
    assert lib.mud_randn_keyed(fake, 2, 8, fake, 1, 0, 3, None) == 1 and 'kind' in lib.mud_last_error().decode()


def test_coverage_refuses_bad_arguments_before_any_launch():
    import mudiff_hip
    lib = mudiff_hip.load()
    fake = C.c_void_p(1 << 20)
    eye = [1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0, 0]
    ok = dict(m=eye, S=(7, 9, 11), D=(8, 8, 8), out=fake)
    nan, inf = list(eye), list(eye)
    nan[5], inf[11] = float('nan'), float('inf')
    bad = [(dict(m=None), 'null'), (dict(out=None), 'null'), (dict(S=(0, 9, 11)), 'bad sizes'), (dict(S=(7, 9, -1)), 'bad sizes'),
           (dict(D=(8, 0, 8)), 'bad sizes'), (dict(D=(-8, 8, 8)), 'bad sizes'), (dict(D=(2048, 2048, 512)), '2^31'), (dict(m=nan), 'finite'),
           (dict(m=inf), 'finite')]
    for change, msg in bad:
        a = dict(ok, **change)
        m = None if a['m'] is None else (C.c_double * 12)(*a['m'])
        assert lib.mud_known_coverage(m, *a['S'], *a['D'], a['out'], None) == 1, change
        assert msg in lib.mud_last_error().decode(), (change, lib.mud_last_error())


def test_wrappers_refuse_on_the_host():
    from mudiff_hip import MudiffHipError, ops
    with pytest.raises(MudiffHipError, match='no CPU'):
        ops.known_constrain(torch.zeros(2, 8), torch.zeros(2, 8), torch.zeros(2, 8, dtype=torch.uint8), torch.zeros(2, dtype=torch.int64), 0,
                            torch.ones(3), torch.ones(3), noise=torch.zeros(2, 8))
    with pytest.raises(ValueError, match='3 x 4'):
        ops.known_coverage(np.eye(3), (4, 4, 4), (4, 4, 4), 'cpu')


# ---------------------------------------------------------------------------------------------------
def test_restatement_of_the_constraint():
    a_tab, s_tab = np.array([1.0, 0.5], np.float32), np.array([0.0, 0.75], np.float32)
    x = np.array([[1, 2, 3, 4], [5, 6, 7, 8]], np.float32)
    k = np.array([[0.5, np.nan, -0.5, 0.25], [np.inf, 1, 1, -1]], np.float32)
    m = np.array([[1, 0, 1, 0], [0, 1, 0, 1]], np.uint8)
    eta = np.full((2, 4), 2.0, np.float32)
    out = R.constrain(x, k, m, eta, [0, 9], 0, a_tab, s_tab)          # row 1's level is clamped to the table's end
    assert out.dtype == np.float32 and out.tolist() == [[0.5, 2.0, -0.5, 4.0], [5.0, 2.0, 7.0, 1.0]]
    assert R.constrain(x, k, m, eta, [0, 9], 0, a_tab, s_tab, clean=True).tolist() == [[0.5, 2.0, -0.5, 4.0], [5.0, 1.0, 7.0, -1.0]]
    assert R.constrain(x, k, np.zeros_like(m), eta, [0, 0], 0, a_tab, s_tab).tolist() == x.tolist()
    full = R.constrain(None, np.nan_to_num(k, posinf=0.0), None, eta, [-5, 0], 1, a_tab, s_tab)      # toff 1: rows at levels 0 and 1
    assert full.tolist() == [[0.5, 0.0, -0.5, 0.25], [1.5, 2.0, 2.0, 1.0]]
    # un-contracted fp32: mul, mul, add, each rounded once
    a, s, kv, e = np.float32(0.1), np.float32(0.3), np.float32(1 / 3), np.float32(0.7)
    want = np.float32(np.float32(a * kv) + np.float32(s * e))
    assert R.constrain(np.zeros((1, 1)), [[kv]], [[1]], [[e]], [0], 0, [a], [s])[0, 0] == want


def test_restatement_of_the_coverage():
    src = (7, 9, 11)
    assert R.coverage(np.eye(4), src, src).all()
    shift = np.eye(4)
    shift[0, 3] = 0.5                                        # +0.5 source voxel along x: the last x-plane would need zero padding
    cov = R.coverage(shift, src, src)
    assert int(cov.sum()) == 6 * 9 * 11 and cov[:6].all() and not cov[6].any()
    shift[0, 3] = -0.5
    cov = R.coverage(shift, src, src)
    assert int(cov.sum()) == 6 * 9 * 11 and cov[1:].all() and not cov[0].any()
    assert R.coverage(np.eye(4), src, (8, 8, 8)).sum() == 7 * 8 * 8
    near = R.near_a_bound(np.eye(4), src, src)               # the identity puts the outer shell on the bounds, and nothing else
    assert near[0].all() and near[:, :, 10].all() and not near[1:6, 1:8, 1:10].any()


# ---------------------------------------------------------------------------------------------------
# the flags, the composition of the known region, the manifest
# ---------------------------------------------------------------------------------------------------
def test_flags_are_parsed_and_checked():
    import volume_support as VS
    from mudiff_hip import known_region as KR, volume as V
    a = V.build_argparser(VS.cli_argv())
    assert (a.known_volume, a.known_mask, a.known_drop_slices, a.known_resample) == (None, None, None, 1)
    assert KR.options_from(a) is None and KR.suffix(None) == '' and V._done_tail(a, 'auto') == ''
    a = V.build_argparser(VS.cli_argv('--known_volume', 'k.nii.gz', '--known_mask', 'm.nii.gz', '--known_drop_slices', '3:5', '7:7',
                                      '--known_resample', '2'))
    assert KR.options_from(a) == dict(volume='k.nii.gz', mask='m.nii.gz', drop=[(3, 5), (7, 7)], resample=2)
    bad = [(['--known_mask', 'm.nii.gz'], '--known_mask needs --known_volume'), (['--known_drop_slices', '1:2'], '--known_drop_slices needs'),
           (['--known_resample', '2'], '--known_resample needs'), (['--known_volume', 'k', '--known_resample', '0'], '--known_resample must'),
           (['--known_volume', 'k', '--known_resample', '-1'], '--known_resample must'), (['--known_volume', 'k', '--known_drop_slices', '5:3'], '5:3'),
           (['--known_volume', 'k', '--known_drop_slices', 'a:b'], 'a:b'), (['--known_volume', 'k', '--known_drop_slices', '3'], "'3'"),
           (['--known_volume', 'k', '--seed', '-1'], '--seed')]
    with pytest.raises(ValueError, match='--known_drop_slices'):
        KR.parse_drop_slices(['-1:2'])
    for argv, msg in bad:
        ns = V.make_parser().parse_args(VS.cli_argv(*argv))
        with pytest.raises(ValueError, match=re.escape(msg)):
            KR.options_from(ns)
        with pytest.raises(SystemExit):                       # the command line refuses it before anything is read
            V.build_argparser(VS.cli_argv(*argv))
    # the parsers whose option lists are pinned keep them: the new flags sit in one of their own, before the last
    p = V.make_parser()
    new = ['--known_volume', '--known_mask', '--known_drop_slices', '--known_resample']
    assert [o for a in p.lates[-2]._actions for o in a.option_strings] == new
    assert not any(o in new for late in [p] + p.lates[:-2] + p.lates[-1:] for a in late._actions for o in a.option_strings)
    # a cohort takes K from its manifest and the other two flags from the command line
    from mudiff_hip import cohort as Co
    c = Co.build_argparser(VS.cli_argv('--manifest', 'c.tsv', '--known_drop_slices', '3:5', '--known_resample', '2'))
    assert KR.options_from(c) is None and c.known_drop_slices == ['3:5']
    with pytest.raises(SystemExit):
        Co.build_argparser(VS.cli_argv('--manifest', 'c.tsv', '--known_volume', 'k.nii.gz'))


def test_mask_composition_on_a_small_case():
    from mudiff_hip import known_region as KR
    shape = (2, 3, 6)
    cov = np.ones(shape, np.uint8)
    cov[0, 0, :] = 0                                          # one column outside K's field of view
    K = np.ones(shape)
    K[1, 1, 2] = np.nan
    K[1, 2, 4] = np.inf
    trust = np.ones(shape)
    trust[1, 0, :] = 0
    drop, s0, s1 = [(3, 3)], 1, 4
    mask, counts = KR.compose_mask(cov, np.isfinite(K), trust, drop, s0, s1)
    assert np.array_equal(mask, R.compose(cov, K, trust, drop, s0, s1))
    want = np.zeros(shape, bool)
    for z in (1, 2, 4):                                       # the slab 1..4 without the dropped slice 3
        want[:, :, z] = [[False, True, True], [False, True, True]]
    want[1, 1, 2] = want[1, 2, 4] = False
    assert np.array_equal(mask, want) and int(mask.sum()) == 10
    assert counts == dict(coverage=30, finite=34, mask=30, not_dropped=30, slab=24)
    mask, counts = KR.compose_mask(None, np.ones(shape, bool), None, [], 0, 5)
    assert mask.all() and counts == dict(coverage=36, finite=36, not_dropped=36, slab=36)
    mask, _ = KR.compose_mask(None, np.ones(shape, bool), None, [(4, 99), (0, 0)], 0, 5)      # a range may run past the volume
    assert mask[:, :, 1:4].all() and not mask[:, :, 0].any() and not mask[:, :, 4:].any()


def test_region_bits_and_suffix():
    from mudiff_hip import known_region as KR
    mask = np.zeros((2, 2, 5), bool)
    mask[0, :, 1:3] = True
    region = KR.KnownRegion(mask, None, None, dict(fraction_of_slab=4 / 12), 1)
    bits = KR.region_bits(region, 1, 3, 2)
    assert bits.shape == (3, 2, 2) and bits.dtype == np.uint8 and KR.REGION_NAMES == ('known', 'synthesised')
    assert bits[0].tolist() == [[4, 4], [8, 8]] and bits[2].tolist() == [[8, 8], [8, 8]]
    assert KR.suffix(region) == ' | known=0.333'
    region.resample = 3
    assert KR.suffix(region) == ' | known=0.333 x3'


def test_a_known_volume_of_another_shape_is_refused_without_regrid(tmp_path):
    import volume_support as VS
    from mudiff_hip import known_region as KR, volume as V, volume_prepare as VP
    first, same, other = (str(tmp_path / f'{k}.nii.gz') for k in ('first', 'same', 'other'))
    V.write_nifti(first, np.ones((8, 8, 9), np.float32), np.eye(4))
    V.write_nifti(same, np.full((8, 8, 9), 2, np.float32), np.eye(4))
    V.write_nifti(other, np.ones((8, 8, 5), np.float32), np.eye(4))
    for k, m, msg in ((other, None, '--known_volume: shape (8, 8, 5)'), (same, other, '--known_mask: shape (8, 8, 5)')):
        args = V.build_argparser(VS.cli_argv('--input_t1', first, '--input_t2', first, '--input_flair', first, '--known_volume', k,
                                             *(() if m is None else ('--known_mask', m))))
        with pytest.raises(ValueError, match=re.escape(msg)):
            V._load_known_inputs(args, {})
    args = V.build_argparser(VS.cli_argv('--input_t1', first, '--input_t2', first, '--input_flair', first, '--known_volume', same))
    inputs = V._load_known_inputs(args, {})                   # nothing to resample: host work only
    assert inputs.shape == (8, 8, 9) and inputs.coverage is None and inputs.trust is None and inputs.resampled == [] and (inputs.values == 2).all()
    options = VP.IntakeOptions.from_args(args)
    assert KR.read_inputs(KR.options_from(args), options)[1] is None


def test_manifest_columns(tmp_path):
    from mudiff_hip import cohort as Co
    path = tmp_path / 'c.tsv'
    path.write_text('id\tt1\tt1ce\tt2\tflair\tgt\tknown\tknown_mask\n'
                    's0\ta.nii\t\tb.nii\tc.nii\t\tk0.nii\t/abs/m0.nii\n'
                    's1\ta.nii\t\tb.nii\tc.nii\tg.nii\t\t\n')
    s0, s1 = Co.read_manifest(str(path))
    assert s0.known == str(tmp_path / 'k0.nii') and s0.known_mask == '/abs/m0.nii' and s0.gt is None
    assert (s1.known, s1.known_mask, s1.gt) == (None, None, str(tmp_path / 'g.nii'))
    path.write_text('id\tt1\tt1ce\tt2\tflair\ns0\ta.nii\t\tb.nii\tc.nii\n')      # the columns are optional
    assert Co.read_manifest(str(path))[0][4:] == (None, None)
    assert Co.Subject('s', {}, None, None) == Co.Subject('s', {}, None, None, None, None)
    path.write_text('id\tt1\tt1ce\tt2\tflair\tknown_mask\ns0\ta.nii\t\tb.nii\tc.nii\tm.nii\n')
    with pytest.raises(ValueError, match='known_mask without a known'):
        Co.read_manifest(str(path))


def test_sampling_paths_without_the_captured_sampler_refuse_a_known_region():
    from mudiff_hip import volume as V
    import argparse
    args = argparse.Namespace(image_size=16, num_timesteps=4, nz=100)
    stacks = [np.zeros((2, 16, 16), np.float32)] * 3
    for kw, msg in ((dict(use_graph=False, seed=1), 'captured sampler'), (dict(seed=None), 'needs a seed'),
                    (dict(seed=1, x_inits=torch.zeros(2, 1, 16, 16)), 'injected')):
        with pytest.raises(ValueError, match=msg):
            V.predict_slices(args, None, None, stacks, 'cpu', known=(None, None), **kw)
