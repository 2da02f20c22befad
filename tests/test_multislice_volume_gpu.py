"""GPU: --known_multislice end to end on the tiny model (mudiff_hip.multislice through mudiff_hip.volume and mudiff_hip.cohort; DESIGN.md
section 5.28): 16 x 16 x 13 phantoms, S = 16, L = 3, G = 1 (slabs 0..2, 4..6, 8..10 and a cut one at 12), gauss, equispaced x2, every run
in one child process under MUD_DETERMINISTIC=1 (tests/volume_support.py)."""
import json
import os

import numpy as np
import pytest

import kspace_ref as KR
import multislice_ref as R
import thick_ref as TR
import volume_support as VS

pytestmark = pytest.mark.gpu
S, Z, L, G, ACCEL, SEED = 16, 13, 3, 1, 2, 31
MS = ['--known_multislice', 'equispaced', '--multislice_thick', str(L), '--multislice_gap', str(G), '--multislice_profile', 'gauss',
      '--multislice_accel', str(ACCEL)]
TH = ['--known_thick', str(L), '--thick_gap', str(G), '--thick_profile', 'gauss']
SLABS = [(0, 2), (4, 6), (8, 10), (12, 12)]
TAIL = f' | multislice={L}+{G} gauss equispaced x{ACCEL}'


def _phantom(shape, i):
    x, y, z = np.meshgrid(*(np.arange(float(n)) for n in shape), indexing='ij')
    return (120 + 60 * np.sin(x / (3 + i) + 0.3 * z) * np.cos(y / (4.5 - i) - 0.2 * z) + 4 * z).astype(np.float32)


@pytest.fixture(scope='module')
def runs(tmp_path_factory):
    from mudiff_hip import volume as V
    tmp = tmp_path_factory.mktemp('multislice')
    VS.write_tiny_model(tmp)
    p = {k: str(tmp / f'{k}.nii.gz') for k in ('flair', 't2', 't1', 'K')}
    for i, k in enumerate(p):
        V.write_nifti(p[k], _phantom((16, 16, Z), i), np.eye(4))
    inputs = ['--input_flair', p['flair'], '--input_t2', p['t2'], '--input_t1', p['t1']]
    known = inputs + ['--known_volume', p['K']]
    jobs = {'plain': (6, 7, inputs, {}), 'ms': (6, 7, known + MS, {}), 'ms_dev': (6, 7, known + MS + ['--device_intake'], {}),
            'ms_b4': (6, 4, known + MS, {}), 'th': (6, 7, known + TH, {}), 'drop': (6, 7, known + MS + ['--known_drop_slices', '5:5'], {}),
            'ens': (6, 7, known + MS + ['--num_samples', '2'], {}), 'ens_b4': (6, 4, known + MS + ['--num_samples', '2'], {}),
            'base': (6, 7, known + MS + ['--multislice_baseline', '--gt_volume', p['K'], '--through_plane'], {}),
            'small': (6, 2, known + MS, dict(raises=True))}
    steps = [VS.volume_step(k, VS.model_argv(tmp, hr, b) + a + ['--output_dir', str(tmp / k)], **o) for k, (hr, b, a, o) in jobs.items()]
    manifest = tmp / 'cohort.tsv'
    manifest.write_text('id\tt1\tt1ce\tt2\tflair\tknown\ns0\t' + '\t'.join([p['t1'], '', p['t2'], p['flair'], p['K']]) + '\n')
    steps.append(VS.cohort_step('cohort', VS.model_argv(tmp, 6, 7) + MS + ['--manifest', str(manifest), '--output_dir', str(tmp / 'cohort')]))
    log = VS.run_plan(tmp, steps, 900, ignore='RuntimeWarning')
    vol = lambda path: V.read_nifti(str(path))[0]             # noqa: E731
    return dict(tmp=tmp, log=log, p=p, vol=vol, pred=lambda k, suffix='': vol(tmp / k / f'predicted_t1ce{suffix}.nii.gz'),
                bytes=lambda k, suffix='': VS.payload(str(tmp / k / f'predicted_t1ce{suffix}.nii.gz')),
                report=lambda k: json.load(open(tmp / k / 'multislice_t1ce.json')))


def _residuals_under_the_rule(rep):
    """Every measured slab: |M_eff (F(A x) - y)| <= 3 rule(S) (|A |x_new|| + |y|) in L2 over the slab's coefficients, the rule
    test_multislice_gpu.py holds the clean step to."""
    worst = 0.0
    for s in rep['slabs']:
        assert (s['residual'] is None) == (not s['measured'])
        if s['measured']:
            assert s['y_norm'] > 0 and 0 <= s['residual'] * s['y_norm'] <= 3 * KR.rule(S) * (s['x_norm'] + s['y_norm']), s
            worst = max(worst, s['residual'])
    return worst


def _masks():
    from mudiff_hip import kspace as KS
    M = KS.build_mask(S, 'equispaced', ACCEL, KS.DEFAULT_CENTER, KS.DEFAULT_AXIS, SEED)
    return M, KR.symmetrise(M)


def test_report_and_residuals(runs):
    rep = runs['report']('ms')
    w32 = TR.profile(L, 'gauss').astype(np.float32)
    M, M_eff = _masks()
    assert (rep['L'], rep['gap'], rep['offset'], rep['profile'], rep['image_size'], rep['slab'], rep['resample']) == (L, G, 0, 'gauss', S, [0, Z - 1], 1)
    assert (rep['pattern'], rep['accel'], rep['center'], rep['axis'], rep['mask_file']) == ('equispaced', ACCEL, 0.08, 0, None)
    assert rep['weights'] == [float(v) for v in w32] and rep['sum_w2'] == float((w32.astype(np.float64) ** 2).sum())
    assert rep['given_fraction'] == float(M.mean()) and rep['effective_fraction'] == float(M_eff.mean()) and 0 < rep['given_fraction'] < 1
    assert [(s['first'], s['last'], s['measured']) for s in rep['slabs']] == [(a, b, b - a + 1 == L) for a, b in SLABS] and rep['measured_slabs'] == 3
    worst = _residuals_under_the_rule(rep)
    print(f'worst residual {worst:.3e}')
    assert rep['max_residual'] == worst
    pred = runs['pred']('ms')
    assert pred.shape == (16, 16, Z) and np.isfinite(pred).all()
    assert VS.done_line(runs['log']['ms']).endswith(TAIL + ' (3/4 slabs)')
    assert sorted(os.listdir(runs['tmp'] / 'ms')) == ['multislice_t1ce.json', 'predicted_t1ce.nii.gz']


def test_the_prediction_is_neither_the_plain_nor_the_thick_one(runs):
    ms, plain, th = runs['pred']('ms'), runs['pred']('plain'), runs['pred']('th')
    assert (ms != plain).any() and (ms != th).any()
    assert ' | multislice=' not in VS.done_line(runs['log']['plain']) and sorted(os.listdir(runs['tmp'] / 'plain')) == ['predicted_t1ce.nii.gz']
    assert ' | multislice=' not in VS.done_line(runs['log']['th'])


def test_intake_batch_size_and_cohort_give_the_same_bytes(runs):
    assert runs['bytes']('ms') == runs['bytes']('ms_dev')
    assert runs['bytes']('ms') == runs['bytes']('ms_b4')
    assert runs['bytes']('ms') == VS.payload(str(runs['tmp'] / 'cohort' / 's0' / 'predicted_t1ce.nii.gz'))
    assert json.load(open(runs['tmp'] / 'cohort' / 's0' / 'multislice_t1ce.json')) == runs['report']('ms') == runs['report']('ms_b4')
    assert VS.done_line(runs['log']['cohort']).endswith(VS.done_line(runs['log']['ms']).split(' | slices=')[1])
    small = runs['log']['small']                              # a slab of 3 thin slices does not fit a batch of 2
    assert '--batch_size 2 ' in small['error']


def test_a_dropped_slice_frees_its_whole_slab(runs):
    rep = runs['report']('drop')
    assert [s['measured'] for s in rep['slabs']] == [True, False, True, False] and rep['drop_slices'] == [[5, 5]] and rep['measured_slabs'] == 2
    assert rep['slabs'][1]['residual'] is None
    _residuals_under_the_rule(rep)
    drop, ms = runs['pred']('drop'), runs['pred']('ms')
    assert all((drop[:, :, z] != ms[:, :, z]).any() for z in (4, 5, 6))          # the whole slab is sampled freely ...
    keep = [0, 1, 2, 3, 7, 8, 9, 10, 11, 12]
    assert np.array_equal(drop[:, :, keep], ms[:, :, keep])                       # ... and no other slice notices


def test_ensemble(runs):
    tmp = runs['tmp']
    assert sorted(os.listdir(tmp / 'ens')) == ['multislice_t1ce.json', 'predicted_t1ce.nii.gz', 'predicted_t1ce_std.nii.gz']
    mean, std = runs['pred']('ens'), runs['pred']('ens', '_std')
    assert np.isfinite(mean).all() and np.isfinite(std).all() and std.any()
    rep = runs['report']('ens')
    assert rep['measured_slabs'] == 3
    _residuals_under_the_rule(rep)                             # the largest over both samples
    assert ' | 2 samples per slice' + TAIL + ' (3/4 slabs)' in VS.done_line(runs['log']['ens'])
    for suffix in ('', '_std'):                                # a (slab, sample) group travels whole whatever the batch size
        assert runs['bytes']('ens', suffix) == runs['bytes']('ens_b4', suffix)
    assert runs['report']('ens_b4') == rep


def test_the_zero_filled_interpolated_baseline(runs):
    tmp = runs['tmp']
    assert sorted(os.listdir(tmp / 'base')) == ['metrics_multislice_baseline_t1ce.json', 'metrics_t1ce.json', 'multislice_baseline_t1ce.nii.gz',
                                                'multislice_t1ce.json', 'predicted_t1ce.nii.gz', 'through_plane_multislice_baseline_t1ce.json',
                                                'through_plane_t1ce.json']
    assert runs['bytes']('base') == runs['bytes']('ms')
    got = runs['vol'](tmp / 'base' / 'multislice_baseline_t1ce.nii.gz')
    from mudiff_hip import volume as V
    k = np.moveaxis(np.asarray(V.normalise_volume(np.asarray(runs['vol'](runs['p']['K']), np.float64)), np.float32).astype(np.float64), 2, 0)
    w32 = TR.profile(L, 'gauss').astype(np.float32)
    starts = [a for a, b in SLABS[:3]]
    y = R.measure(k, [list(range(a, a + L)) for a in starts], w32, _masks()[1][None])
    want = np.clip(0.5 * R.baseline(y, starts, L, Z) + 0.5, 0, 1)
    assert np.abs(np.moveaxis(got, 2, 0) - want).max() <= 1e-5
    both = [json.load(open(tmp / 'base' / f)) for f in ('metrics_t1ce.json', 'metrics_multislice_baseline_t1ce.json')]
    assert both[0].keys() == both[1].keys()
    both = [json.load(open(tmp / 'base' / f)) for f in ('through_plane_t1ce.json', 'through_plane_multislice_baseline_t1ce.json')]
    assert both[0].keys() == both[1].keys()
    assert '[multislice-baseline] ' in runs['log']['base']
