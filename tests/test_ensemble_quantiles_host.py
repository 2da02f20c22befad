"""CPU: the order statistics of an ensemble - the numpy restatements the kernels are held to
(tests/ensemble_quantile_ref.py, tests/volume_coverage_ref.py), the flags of the two command lines, the file-name rule, the report of
mudiff_hip.volume_coverage and the two C-ABI symbols."""
import argparse
import os

import numpy as np
import pytest

import ensemble_quantile_ref as Q
import volume_coverage_ref as C
import volume_support as VS

QS = (0.0, 0.05, 0.25, 0.5, 0.75, 0.95, 1.0)


@pytest.mark.parametrize('N', [2, 3, 8, 33])
def test_restatement_agrees_with_np_quantile(N):
    x = np.random.default_rng(N).standard_normal((3, N, 5, 7)).astype(np.float32)
    got = Q.quantiles(x, QS)
    want = np.quantile(x.astype(np.float64), QS, axis=1)
    assert got.shape == want.shape == (len(QS), 3, 5, 7) and got.dtype == np.float32
    assert float(np.abs(got - want).max()) <= 1e-6
    # the [0, 1] pre-map is applied before the sort
    y = np.clip(x * np.float32(0.5) + np.float32(0.5), 0, 1)
    assert float(np.abs(Q.quantiles(x, QS, 0.5, 0.5, 0.0, 1.0) - np.quantile(y.astype(np.float64), QS, axis=1)).max()) <= 1e-6


@pytest.mark.parametrize('N', [3, 5, 33])
def test_restatement_median_of_odd_n_is_exact(N):
    x = np.random.default_rng(N + 100).standard_normal((2, N, 11)).astype(np.float32)
    got = Q.quantiles(x, (0.5,))[0]
    assert np.array_equal(got, np.sort(x, axis=1)[:, N // 2])
    assert np.array_equal(Q.quantiles(x, (0.0,))[0], x.min(1))


def test_restatement_nan_reaches_every_quantile():
    x = np.random.default_rng(5).standard_normal((2, 8, 6)).astype(np.float32)
    x[1, 3, 2] = np.nan
    got = Q.quantiles(x, QS)
    assert np.isnan(got[:, 1, 2]).all()
    keep = np.ones((2, 6), bool)
    keep[1, 2] = False
    assert np.isfinite(got[:, keep]).all()
    clean = np.array(x)
    clean[1, 3, 2] = 0.0
    assert np.array_equal(got[:, keep], Q.quantiles(clean, QS)[:, keep])


# ---------------------------------------------------------------------------------------------------
def test_file_name_rule():
    from mudiff_hip import ensemble as E
    assert [E.quantile_suffix(q) for q in (0.05, 0.5, 0.975, 0.0, 1.0)] == ['_q050', '_q500', '_q975', '_q000', '_q1000']


def _parsers():
    from mudiff_hip import cohort as CO
    from mudiff_hip import volume as V
    return ((lambda a: V.build_argparser(VS.cli_argv(*a)), '--gt_volume', ['--gt_volume', 'gt.nii.gz']),
            (lambda a: CO.build_argparser(VS.cli_argv('--manifest', 'm.tsv', *a)), '--score', ['--score']))


def test_flags_accept_the_valid_forms():
    from mudiff_hip import ensemble as E
    from mudiff_hip import volume as V
    for parse, _, scored in _parsers():
        a = parse(['--num_samples', '4', '--ensemble_quantiles', '0.05', '0.5', '0.95'])
        plan = E.quantile_plan(a)
        assert a.ensemble_quantiles == [0.05, 0.5, 0.95] and a.ensemble_center == 'mean' and a.coverage is None
        assert plan.computed == plan.written == (0.05, 0.5, 0.95) and plan.center == 'mean' and plan.coverage is None
        assert V._done_tail(a, 'auto') == ' | quantiles=0.05,0.5,0.95'
        b = parse(['--num_samples', '64', '--ensemble_center', 'median'])
        plan = E.quantile_plan(b)
        assert plan.computed == (0.5,) and plan.written == () and plan.center == 'median'      # computed, not written
        assert V._done_tail(b, 'auto') == ' | center=median'
        c = parse(['--num_samples', '8', '--coverage', '0.05', '0.95', '--ensemble_center', 'median', '--ensemble_quantiles', '0.25'] + scored)
        plan = E.quantile_plan(c)
        assert plan.computed == (0.05, 0.25, 0.5, 0.95) and plan.written == (0.05, 0.25, 0.95) and plan.coverage == (0.05, 0.95)
        assert V._done_tail(c, '16x1') == ' | prec_plan=16x1 | center=median | quantiles=0.05,0.25,0.95'
        d = parse(['--num_samples', '2', '--ensemble_quantiles', '0', '0.125', '0.25', '0.375', '0.5', '0.625', '0.75', '1'])
        assert len(E.quantile_plan(d).computed) == 8


BAD = [(['--ensemble_quantiles', '0.5'], '--ensemble_quantiles needs --num_samples'),
       (['--ensemble_center', 'median'], '--ensemble_center median needs --num_samples'),
       (['--num_samples', '65', '--ensemble_quantiles', '0.5'], '--ensemble_quantiles needs --num_samples <= 64'),
       (['--num_samples', '65', '--ensemble_center', 'median'], '--ensemble_center median needs --num_samples <= 64'),
       (['--num_samples', '4', '--ensemble_quantiles', '0.5', '1.5'], '--ensemble_quantiles takes 1 to 8 fractions in [0, 1]'),
       (['--num_samples', '4', '--ensemble_quantiles', '-0.1'], '--ensemble_quantiles takes 1 to 8 fractions in [0, 1]'),
       (['--num_samples', '4', '--ensemble_quantiles', 'nan'], '--ensemble_quantiles takes 1 to 8 fractions in [0, 1]'),
       (['--num_samples', '4', '--ensemble_quantiles'] + [str(i / 10) for i in range(9)], '--ensemble_quantiles takes 1 to 8 fractions'),
       (['--num_samples', '4', '--ensemble_quantiles', '0.5', '0.5'], '--ensemble_quantiles: the fractions must be strictly increasing'),
       (['--num_samples', '4', '--ensemble_quantiles', '0.9', '0.1'], '--ensemble_quantiles: the fractions must be strictly increasing'),
       (['--num_samples', '4', '--ensemble_center', 'mode'], '--ensemble_center'),
       (['--num_samples', '4', '--ensemble_quantiles', '0.0501', '0.0502'], 'round to one file name')]
BAD_SCORED = [(['--num_samples', '4', '--coverage', '0.95', '0.05'], '--coverage: Q_LO must be below Q_HI'),
              (['--num_samples', '4', '--coverage', '0.5', '0.5'], '--coverage: Q_LO must be below Q_HI'),
              (['--num_samples', '4', '--coverage', '0.05', '1.5'], '--coverage takes two fractions'),
              (['--num_samples', '65', '--coverage', '0.05', '0.95'], '--coverage needs --num_samples <= 64'),
              (['--coverage', '0.05', '0.95'], '--coverage needs --num_samples')]


def test_flags_refuse_bad_combinations(capsys):
    for parse, score_flag, scored in _parsers():
        cases = BAD + [(a + scored, msg) for a, msg in BAD_SCORED] + [(['--num_samples', '4', '--coverage', '0.05', '0.95'], '--coverage needs --gt_volume')]
        for argv, msg in cases:
            with pytest.raises(SystemExit) as e:
                parse(argv)
            err = capsys.readouterr().err
            assert e.value.code == 2 and msg in err, (argv, err[-300:])


def test_without_the_flags_nothing_changes():
    from mudiff_hip import ensemble as E
    from mudiff_hip import volume as V
    for argv in ([], ['--num_samples', '4']):
        a = V.build_argparser(VS.cli_argv(*argv))
        assert (a.ensemble_quantiles, a.ensemble_center, a.coverage) == (None, 'mean', None)
        assert E.quantile_plan(a) is None and V._done_tail(a, 'auto') == ''
        b = V.build_argparser(VS.cli_argv(*argv))
        for k in ('ensemble_quantiles', 'ensemble_center', 'coverage'):      # the namespace of the parser before the flags existed
            delattr(b, k)
        assert E.quantile_plan(b) is None and V._done_tail(b, 'auto') == ''
        assert {k: v for k, v in vars(a).items() if k in vars(b)} == vars(b)
    bare = argparse.Namespace(norm='percentile')
    assert E.quantile_plan(bare) is None and V._done_tail(bare, 'auto') == ''
    # the main option list and `late` stay what their tests pin: the new flags sit in a parser of their own
    p = V.make_parser()
    new = ['--ensemble_quantiles', '--ensemble_center', '--coverage']
    assert [o for a in p.lates[-1]._actions for o in a.option_strings] == new
    assert not any(o in new for late in [p] + p.lates[:-1] for a in late._actions for o in a.option_strings)


def test_sample_ensemble_refuses_quantiles_of_more_than_64_samples():
    from mudiff_hip import ensemble as E
    with pytest.raises(ValueError, match='64'):
        E.sample_ensemble(None, None, None, (None, None, None), 65, 1, quantiles=(0.5,))
    with pytest.raises(ValueError, match='fractions'):
        E.sample_ensemble(None, None, None, (None, None, None), 8, 1, quantiles=(1.5,))
    with pytest.raises(ValueError, match='fractions'):
        E.check_quantiles([0.1] * 9)
    assert E.check_quantiles([0, 0.5, 1]) == (0.0, 0.5, 1.0)


# ---------------------------------------------------------------------------------------------------
def _hand_made():
    """9 x 7 x 7 planes-first volumes: the interval is [0.25, 0.75] everywhere; plane z holds z voxels below it and 2 above (the
    first z and the last 2 of the plane's 49), the rest at 0.5; region bit 1 is the first 3 rows (21 voxels) of every plane."""
    lo, hi = np.full((9, 7, 7), 0.25, np.float32), np.full((9, 7, 7), 0.75, np.float32)
    gt = np.full((9, 49), 0.5, np.float32)
    for z in range(9):
        gt[z, :z] = 0.0
        gt[z, 47:] = 1.0
    region = np.ones((9, 7, 7), np.uint8)
    region[:, :3] |= 2
    return lo, hi, gt.reshape(9, 7, 7), region


def test_coverage_restatement_on_a_hand_made_case():
    lo, hi, gt, region = _hand_made()
    counts, sums, z0, z1 = C.coverage(lo, hi, gt, region, 2)
    assert (z0, z1) == (0, 8) and counts.shape == (9, 2, 5) and sums.shape == (9, 2, 2)
    for z in range(9):
        assert counts[z, 0].tolist() == [49, z, 2, 47 - z, 0]
        assert counts[z, 1].tolist() == [21, z, 0, 21 - z, 0]          # the first 21 voxels: the z below, none of the 2 above
        assert sums[z, 0].tolist() == [49 * 0.5, (47 - z) * 0.5] and sums[z, 1].tolist() == [21 * 0.5, (21 - z) * 0.5]
    # the boundary belongs to the interval; a NaN in any of the three is nonfinite and nothing else
    gt[4, 3, 3], lo[4, 3, 4], hi[4, 3, 5] = np.nan, np.nan, np.nan
    gt[5, 6, 0], gt[5, 6, 1] = 0.25, 0.75
    counts, sums, _, _ = C.coverage(lo, hi, gt, region, 2, 3, 20)
    assert counts.shape == (6, 2, 5)
    assert counts[1, 0].tolist() == [46, 4, 2, 40, 3] and sums[1, 0].tolist() == [46 * 0.5, 40 * 0.5]
    assert counts[2, 0].tolist() == [49, 5, 2, 42, 0]
    # without a region volume every voxel is in every region
    both = C.coverage(lo, hi, gt, None, 2)[0]
    assert np.array_equal(both[:, 0], both[:, 1]) and both[5, 0].tolist() == [49, 5, 2, 42, 0]


def test_coverage_report_from_the_sums():
    from mudiff_hip import volume_coverage as VC
    lo, hi, gt, region = _hand_made()
    gt[0, 6, 6] = np.nan
    counts, sums, z0, _ = C.coverage(lo, hi, gt, region, 2, 0, 7)
    counts = np.concatenate([counts, np.zeros((8, 1, 5), np.int64)], 1)        # an empty third region
    sums = np.concatenate([sums, np.zeros((8, 1, 2))], 1)
    rep = VC.summarize(counts, sums, ('slab', 'brain', 'tumor'), 3, nominal=0.9)
    assert rep['regions'] == ['slab', 'brain', 'tumor'] and rep['per_plane']['plane'] == list(range(3, 11))
    s = rep['coverage']['slab']
    below, above = sum(range(8)), 2 * 8 - 1
    n = 8 * 49 - 1
    assert (s['voxels'], s['nonfinite'], s['below_voxels'], s['above_voxels'], s['inside_voxels']) == (8 * 49, 1, below, above, n - below - above)
    assert s['empirical'] == (n - below - above) / n and s['below'] == below / n and s['above'] == above / n
    assert s['mean_width'] == 0.5 and s['mean_width_inside'] == 0.5 and s['nominal'] == 0.9
    assert rep['per_plane']['slab']['empirical'][0] == 47 / 48 and rep['per_plane']['brain']['empirical'][2] == 19 / 21
    t = rep['coverage']['tumor']
    assert t['voxels'] == 0 and all(t[k] is None for k in ('empirical', 'below', 'above', 'mean_width', 'mean_width_inside'))
    assert rep['per_plane']['tumor']['empirical'] == [None] * 8
    lines = VC.format_lines(dict(rep))
    assert len(lines) == 3 and lines[0].startswith('[coverage] slab: empirical ') and 'nominal 0.9' in lines[0] and 'nonfinite 1' in lines[0]
    assert 'n/a' in lines[2]
    with pytest.raises(ValueError):
        VC.summarize(counts, sums, ('slab',))
    assert 'nominal' in VC.__doc__ and 'guaranteed' in VC.__doc__


def test_cohort_aggregates_the_coverage_blocks():
    from mudiff_hip import cohort as CO
    rows = [dict(id='a', metrics={}, coverage=dict(slab=dict(empirical=0.5, mean_width=0.2), brain=dict(empirical=None, mean_width=None))),
            dict(id='b', metrics={}, coverage=dict(slab=dict(empirical=0.7, mean_width=0.4), brain=dict(empirical=0.25, mean_width=0.1))),
            dict(id='c', metrics={})]
    agg = CO.aggregate_coverage(rows)
    assert agg['slab']['empirical'] == dict(mean=pytest.approx(0.6), std=pytest.approx(0.1), count=2)
    assert agg['slab']['mean_width']['mean'] == pytest.approx(0.3) and agg['brain']['empirical'] == dict(mean=0.25, std=0.0, count=1)
    rep = dict(regions=['slab'], coverage=dict(slab=dict(empirical=0.5, mean_width=0.25, voxels=7)))
    assert CO.coverage_row(rep) == dict(slab=dict(empirical=0.5, mean_width=0.25))


def test_the_two_symbols_are_exported():
    import mudiff_hip
    assert {'mud_ensemble_quantiles', 'mud_volume_interval_coverage'} <= set(mudiff_hip.EXPORTED_SYMBOLS)
    if not os.path.isfile(mudiff_hip.lib_path()):
        import __graft_entry__
        __graft_entry__.build()
    lib = mudiff_hip.load()
    assert hasattr(lib, 'mud_ensemble_quantiles') and hasattr(lib, 'mud_volume_interval_coverage')
    # argument checks come before any launch: no GPU is needed to be refused
    import ctypes as C_
    q = (C_.c_double * 9)(*([0.5] * 9))
    one = C_.c_void_p(16)
    assert lib.mud_ensemble_quantiles(one, 1, 65, 4, 1.0, 0.0, 0.0, 1.0, q, 1, one, None) != 0 and b'[2, 64]' in lib.mud_last_error()
    assert lib.mud_ensemble_quantiles(one, 1, 4, 4, 1.0, 0.0, 0.0, 1.0, q, 9, one, None) != 0 and b'1 to 8' in lib.mud_last_error()
    q[0] = 1.5
    assert lib.mud_ensemble_quantiles(one, 1, 4, 4, 1.0, 0.0, 0.0, 1.0, q, 1, one, None) != 0 and b'not in [0, 1]' in lib.mud_last_error()
    q[0] = float('nan')
    assert lib.mud_ensemble_quantiles(one, 1, 4, 4, 1.0, 0.0, 0.0, 1.0, q, 1, one, None) != 0
    q[0] = 0.5
    assert lib.mud_ensemble_quantiles(None, 1, 4, 4, 1.0, 0.0, 0.0, 1.0, q, 1, one, None) != 0 and b'null' in lib.mud_last_error()
    assert lib.mud_ensemble_quantiles(one, 0, 4, 4, 1.0, 0.0, 0.0, 1.0, q, 1, one, None) == 0             # n == 0: nothing to do
    assert lib.mud_volume_interval_coverage(one, one, one, None, 9, 7, 7, 9, 0, 8, one, one, one, 1 << 20, None) != 0
    assert lib.mud_volume_interval_coverage(one, one, one, None, 9, 7, 7, 1, 3, 9, one, one, one, 1 << 20, None) != 0
    assert lib.mud_volume_interval_coverage(one, one, one, None, 9, 7, 7, 1, 0, 8, one, one, one, 8, None) != 0 and b'needs' in lib.mud_last_error()
