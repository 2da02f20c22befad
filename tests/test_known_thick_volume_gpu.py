"""GPU: --known_thick_volume end to end on the tiny model (mudiff_hip.thick_volume through mudiff_hip.volume and mudiff_hip.cohort;
DESIGN.md section 5.29): 16 x 16 x 13 thin phantoms at 1 mm, S = 16, and a thick volume made from the thin target with
band_ref.weights - 4 mm slices every 2 mm (50 % overlap) from a fractional origin, 6 of them, the last reaching past the stack - written
with its own affine by the project's NIfTI writer.  Every run in one child process under MUD_DETERMINISTIC=1 (tests/volume_support.py).
(tests/test_thick_volume_gpu.py is --known_thick's, the retrospective mode.)"""
import json
import os

import numpy as np
import pytest

import band_ref as R
import volume_support as VS

pytestmark = pytest.mark.gpu
S, Z = 16, 13
C0, STEP, T, M_ALL = 1.75, 2.0, 4.0, 6                      # thick slice j is centred at thin index 1.75 + 2 j, 4 thin slices thick
Y_AFFINE = np.array([[1.0, 0, 0, 0], [0, 1.0, 0, 0], [0, 0, STEP, C0], [0, 0, 0, 1.0]])


def _phantom(shape, i):
    x, y, z = np.meshgrid(*(np.arange(float(n)) for n in shape), indexing='ij')
    return (120 + 60 * np.sin(x / (3 + i) + 0.3 * z) * np.cos(y / (4.5 - i) - 0.2 * z) + 4 * z).astype(np.float32)


def _thick_of(k, profile='box', width=T):
    """The thick volume of the thin volume k [X,Y,Z]: every slice j = 0..M_ALL-1, whether or not its support lies inside the stack."""
    rows = np.stack([R.row(Z, C0 + STEP * j, width, profile) for j in range(M_ALL)])
    return np.tensordot(k.astype(np.float64), rows, axes=(2, 1)).astype(np.float32)


@pytest.fixture(scope='module')
def runs(tmp_path_factory):
    from mudiff_hip import volume as V
    tmp = tmp_path_factory.mktemp('thick_volume')
    VS.write_tiny_model(tmp)
    p = {k: str(tmp / f'{k}.nii.gz') for k in ('flair', 't2', 't1', 'K')}
    for i, k in enumerate(p):
        V.write_nifti(p[k], _phantom((16, 16, Z), i), np.eye(4))
    K = _phantom((16, 16, Z), 3)
    p['Y'], p['Yg'], p['Ybad'] = (str(tmp / f'{k}.nii.gz') for k in ('Y', 'Yg', 'Ybad'))
    V.write_nifti(p['Y'], _thick_of(K), Y_AFFINE)
    V.write_nifti(p['Yg'], _thick_of(K, 'gauss', 3.0), Y_AFFINE)
    V.write_nifti(p['Ybad'], _thick_of(K)[:, :12], Y_AFFINE)
    inputs = ['--input_flair', p['flair'], '--input_t2', p['t2'], '--input_t1', p['t1']]
    tv = inputs + ['--known_thick_volume', p['Y'], '--thick_volume_thickness_mm', str(T)]
    jobs = {'plain': (7, inputs, {}), 'tv': (7, tv, {}), 'tv_b4': (4, tv, {}), 'tv_dev': (7, tv + ['--device_intake'], {}),
            'drop': (7, tv + ['--thick_volume_drop', '2:2'], {}),
            'base': (7, tv + ['--thick_volume_baseline', '--gt_volume', p['K'], '--through_plane'], {}),
            'ens': (7, tv + ['--num_samples', '2'], {}), 'ens_b4': (4, tv + ['--num_samples', '2'], {}),
            'gauss': (7, inputs + ['--known_thick_volume', p['Yg'], '--thick_volume_thickness_mm', '3', '--thick_volume_profile', 'gauss',
                                   '--known_resample', '2'], {}),
            'shape': (7, inputs + ['--known_thick_volume', p['Ybad']], dict(raises=True))}
    steps = [VS.volume_step(k, VS.model_argv(tmp, 6, b) + a + ['--output_dir', str(tmp / k)], **o) for k, (b, a, o) in jobs.items()]
    manifest = tmp / 'cohort.tsv'
    manifest.write_text('id\tt1\tt1ce\tt2\tflair\tknown\ns0\t' + '\t'.join([p['t1'], '', p['t2'], p['flair'], p['Y']]) + '\n')
    steps.append(VS.cohort_step('cohort', VS.model_argv(tmp, 6, 7) + ['--known_thick_volume', 'manifest', '--thick_volume_thickness_mm', str(T),
                                                                      '--manifest', str(manifest), '--output_dir', str(tmp / 'cohort')]))
    log = VS.run_plan(tmp, steps, 900, ignore='RuntimeWarning')
    vol = lambda path: V.read_nifti(str(path))[0]             # noqa: E731
    return dict(tmp=tmp, log=log, p=p, vol=vol, pred=lambda k, suffix='': vol(tmp / k / f'predicted_t1ce{suffix}.nii.gz'),
                bytes=lambda k, suffix='': VS.payload(str(tmp / k / f'predicted_t1ce{suffix}.nii.gz')),
                report=lambda k: json.load(open(tmp / k / 'thick_volume_t1ce.json')))


def _residuals_under_the_rule(rep, A):
    """Every measured thick slice: |A x - y| in L2 over its pixels is at most band_ref.bound_residual_norms of the recorded norms - the
    relative form of band_ref.bound_residual."""
    measured = [s for s in rep['slices'] if s['measured']]
    assert len(measured) == A.shape[0] == rep['measured_slices']
    bound = R.bound_residual_norms(rep['x_new_norm'], [s['y_norm'] for s in measured], A)
    worst = 0.0
    for s, b in zip(measured, bound):
        assert s['y_norm'] > 0 and 0 <= s['residual'] * s['y_norm'] <= b, (s, b)
        worst = max(worst, s['residual'])
    assert all(s['residual'] is None and s['y_norm'] is None for s in rep['slices'] if not s['measured'])
    print(f"worst residual {worst:.3e}, relative bound {max(b / s['y_norm'] for s, b in zip(measured, bound)):.3e}")
    assert rep['max_residual'] == worst
    return worst


def test_report_residuals_and_done_line(runs):
    rep = runs['report']('tv')
    A, centres, idx = R.weights(Z, C0, STEP, T, 'box', count=M_ALL)
    assert idx == [0, 1, 2, 3, 4]                                                        # the sixth reaches past the last thin slice
    assert (rep['T'], rep['thin_dz'], rep['thick_dz'], rep['c0'], rep['step'], rep['profile'], rep['image_size'], rep['slab'], rep['resample']) == \
        (T, 1.0, STEP, C0, STEP, 'box', S, [0, Z - 1], 1)
    assert [(s['centre'], s['measured']) for s in rep['slices']] == [(C0 + STEP * j, j < 5) for j in range(M_ALL)]
    assert rep['bandwidth'] == R.bandwidth(A) == 2 and rep['cond'] == pytest.approx(R.cond(A), rel=1e-9)
    assert _residuals_under_the_rule(rep, A) < 1e-5
    pred, plain = runs['pred']('tv'), runs['pred']('plain')
    assert pred.shape == (16, 16, Z) and np.isfinite(pred).all() and (pred != plain).any()
    assert VS.done_line(runs['log']['tv']).endswith(f" | thick_volume=4mm/1mm box (5/6 slices, bw {rep['bandwidth']})")
    assert sorted(os.listdir(runs['tmp'] / 'tv')) == ['predicted_t1ce.nii.gz', 'thick_volume_t1ce.json']


def test_batch_size_intake_and_cohort_give_the_same_bytes(runs):
    """Bitwise, as tests/test_thick_volume_gpu.py holds --known_thick at another --batch_size on this model."""
    assert runs['bytes']('tv') == runs['bytes']('tv_b4')
    assert runs['bytes']('tv') == runs['bytes']('tv_dev')
    assert runs['bytes']('tv') == VS.payload(str(runs['tmp'] / 'cohort' / 's0' / 'predicted_t1ce.nii.gz'))
    assert json.load(open(runs['tmp'] / 'cohort' / 's0' / 'thick_volume_t1ce.json')) == runs['report']('tv') == runs['report']('tv_b4')
    assert VS.done_line(runs['log']['cohort']).endswith(VS.done_line(runs['log']['tv']).split(' | slices=')[1])


def test_a_dropped_thick_slice_is_not_measured(runs):
    rep = runs['report']('drop')
    assert [s['measured'] for s in rep['slices']] == [True, True, False, True, True, False] and rep['drop'] == [[2, 2]]
    A, _, _ = R.weights(Z, C0, STEP, T, 'box', count=M_ALL)
    _residuals_under_the_rule(rep, A[[0, 1, 3, 4]])
    assert runs['bytes']('drop') != runs['bytes']('tv')


def test_baseline_is_written_and_scored(runs):
    out = runs['tmp'] / 'base'
    assert (out / 'thick_volume_interp_t1ce.nii.gz').is_file() and (out / 'metrics_thick_volume_interp_t1ce.json').is_file()
    assert (out / 'through_plane_thick_volume_interp_t1ce.json').is_file()
    base = runs['vol'](out / 'thick_volume_interp_t1ce.nii.gz')
    assert base.shape == (16, 16, Z) and np.isfinite(base).all() and base.min() >= 0 and base.max() <= 1
    assert np.array_equal(base[:, :, 0], base[:, :, 1]) and np.array_equal(base[:, :, 10], base[:, :, 12])      # constant beyond the centres
    assert runs['bytes']('base') == runs['bytes']('tv')
    assert '[thick-volume-interp] ' in runs['log']['base']


def test_ensemble_writes_mean_and_std(runs):
    assert runs['bytes']('ens') == runs['bytes']('ens_b4') and runs['bytes']('ens', '_std') == runs['bytes']('ens_b4', '_std')
    std = runs['pred']('ens', '_std')
    assert np.isfinite(std).all() and (std > 0).any() and runs['bytes']('ens') != runs['bytes']('tv')
    A, _, _ = R.weights(Z, C0, STEP, T, 'box', count=M_ALL)
    _residuals_under_the_rule(runs['report']('ens'), A)
    assert '2 samples per slice' in VS.done_line(runs['log']['ens'])


def test_gauss_profile_with_resampling(runs):
    rep = runs['report']('gauss')
    A, _, idx = R.weights(Z, C0, STEP, 3.0, 'gauss', count=M_ALL)
    assert rep['profile'] == 'gauss' and rep['resample'] == 2 and [j for j, s in enumerate(rep['slices']) if s['measured']] == idx
    _residuals_under_the_rule(rep, A)


def test_refusals_name_the_flag(runs, capsys):
    from mudiff_hip import volume as V
    err = runs['log']['shape']['error']
    assert '--known_thick_volume' in err and 'in-plane shape' in err and 'out of scope' in err
    with pytest.raises(SystemExit):
        V.build_argparser(VS.cli_argv('--known_thick_volume', runs['p']['Y'], '--known_volume', runs['p']['K']))
    assert '--known_thick_volume cannot be combined with --known_volume' in capsys.readouterr().err
