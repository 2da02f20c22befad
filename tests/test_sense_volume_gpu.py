"""GPU: --known_sense end to end on the tiny model (mudiff_hip.sense through mudiff_hip.volume and mudiff_hip.cohort; DESIGN.md section
5.32): 16 x 16 x 9 phantoms, S = 16, every run in one child process under MUD_DETERMINISTIC=1 (tests/volume_support.py)."""
import hashlib
import json
import os

import numpy as np
import pytest

import sense_ref as R
import volume_support as VS

pytestmark = pytest.mark.gpu
S, NC, LAM, ITERS = 16, 4, 8.0, 12
SN = ['--known_sense', 'equispaced', '--sense_accel', '2', '--sense_coils', str(NC)]


def _phantom(shape, i):
    x, y, z = np.meshgrid(*(np.arange(float(n)) for n in shape), indexing='ij')
    return (120 + 60 * np.sin(x / (3 + i) + 0.3 * z) * np.cos(y / (4.5 - i) - 0.2 * z) + 4 * z).astype(np.float32)


@pytest.fixture(scope='module')
def runs(tmp_path_factory):
    from mudiff_hip import volume as V
    tmp = tmp_path_factory.mktemp('sense')
    VS.write_tiny_model(tmp)
    p = {k: str(tmp / f'{k}.nii.gz') for k in ('flair', 't2', 't1', 'K')}
    for i, k in enumerate(p):
        V.write_nifti(p[k], _phantom((16, 16, 9), i), np.eye(4))
    inputs = ['--input_flair', p['flair'], '--input_t2', p['t2'], '--input_t1', p['t1']]
    known = inputs + ['--known_volume', p['K']]
    noisy = known + SN + ['--sense_noise', '0.05']
    jobs = {'plain': (5, inputs, {}), 'plain_old': (5, inputs, dict(strip=['known_sense', 'sense_'])),
            'sn': (5, known + SN, {}), 'sn_dev': (5, known + SN + ['--device_intake'], {}), 'sn_b2': (2, known + SN, {}),
            'drop': (5, known + SN + ['--known_drop_slices', '3:5'], {}), 'ens': (5, known + SN + ['--num_samples', '2'], {}),
            'base': (5, known + SN + ['--sense_baseline', '--gt_volume', p['K']], {}),
            'noise': (5, noisy, {}), 'noise_again': (2, noisy, {}), 'noise_seed': (5, noisy + ['--seed', '32'], {})}
    steps = [VS.volume_step(k, VS.model_argv(tmp, 4, b) + a + ['--output_dir', str(tmp / k)], **o) for k, (b, a, o) in jobs.items()]
    manifest = tmp / 'cohort.tsv'
    manifest.write_text('id\tt1\tt1ce\tt2\tflair\tknown\ns0\t' + '\t'.join([p['t1'], '', p['t2'], p['flair'], p['K']]) + '\n')
    steps.append(VS.cohort_step('cohort', VS.model_argv(tmp, 4, 5) + SN + ['--manifest', str(manifest), '--output_dir', str(tmp / 'cohort')]))
    log = VS.run_plan(tmp, steps, 900, ignore='RuntimeWarning')
    vol = lambda path: V.read_nifti(str(path))[0]             # noqa: E731
    return dict(tmp=tmp, log=log, p=p, vol=vol, pred=lambda k, suffix='': vol(tmp / k / f'predicted_t1ce{suffix}.nii.gz'),
                bytes=lambda k: VS.payload(str(tmp / k / 'predicted_t1ce.nii.gz')), report=lambda k: json.load(open(tmp / k / 'sense_t1ce.json')))


def _residuals_fall(rep):
    """Every measured slice: the step does not move away from the measurement, and the conjugate gradients ended finite."""
    for r, before, cg, m, yn in zip(rep['residual_per_slice'], rep['residual_before_per_slice'], rep['cg_residual_per_slice'],
                                    rep['measured_per_slice'], rep['y_norm_per_slice']):
        assert (r is None) == (before is None) == (cg is None) == (not m)
        if m:
            assert yn > 0 and 0 <= r <= before and 0 <= cg < 1, (r, before, cg)


def test_report_and_residuals(runs):
    from mudiff_hip import kspace as KS_
    rep = runs['report']('sn')
    M = KS_.build_mask(S, 'equispaced', 2, 0.08, 0, seed=31)
    assert (rep['pattern'], rep['accel'], rep['center'], rep['axis'], rep['image_size'], rep['slab']) == ('equispaced', 2, 0.08, 0, S, [0, 8])
    assert (rep['coils'], rep['maps'], rep['lambda'], rep['iters'], rep['noise']) == (NC, 'analytic', LAM, ITERS, 0.0)
    assert rep['sampling_fraction'] == float(M.mean()) and 0.5 <= rep['sampling_fraction'] < 1.0       # the pattern as given, not symmetrised
    assert rep['measured_slices'] == 9 and rep['unmeasured_slices'] == 0 and rep['measured_per_slice'] == [True] * 9 and rep['resample'] == 1
    assert 'noise_floor_per_slice' not in rep and len(rep['x_norm_per_slice']) == 9 and min(rep['x_norm_per_slice']) > 0
    _residuals_fall(rep)
    assert rep['max_residual'] == max(rep['residual_per_slice']) and rep['max_cg_residual'] == max(rep['cg_residual_per_slice'])
    print(f"residual {rep['max_residual']:.3e} (before the last step {rep['max_residual_before']:.3e}), CG {rep['max_cg_residual']:.3e}")
    pred, plain = runs['pred']('sn'), runs['pred']('plain')
    assert pred.shape == (16, 16, 9) and np.isfinite(pred).all() and (pred != plain).any()
    assert VS.done_line(runs['log']['sn']).endswith(f' | sense=equispaced x2 {NC} coils')
    assert sorted(os.listdir(runs['tmp'] / 'sn')) == ['predicted_t1ce.nii.gz', 'sense_t1ce.json']


def test_intake_batch_size_and_cohort_give_the_same_bytes(runs):
    assert runs['bytes']('sn') == runs['bytes']('sn_dev')
    assert runs['bytes']('sn') == runs['bytes']('sn_b2')
    assert runs['bytes']('sn') == VS.payload(str(runs['tmp'] / 'cohort' / 's0' / 'predicted_t1ce.nii.gz'))
    assert json.load(open(runs['tmp'] / 'cohort' / 's0' / 'sense_t1ce.json')) == runs['report']('sn') == runs['report']('sn_b2')
    assert VS.done_line(runs['log']['cohort']).endswith(VS.done_line(runs['log']['sn']).split(' | slices=')[1])


def test_without_the_flags_nothing_changes(runs):
    """The run without the flags writes the bytes the existing payload fixture records (tests/golden/kspace_parent_payloads.json: the
    same phantoms and model), a namespace as the parser left it before these flags existed gives the same, and those runs write nothing
    new."""
    from conftest import REPO
    with open(os.path.join(REPO, 'tests', 'golden', 'kspace_parent_payloads.json')) as f:
        recorded = json.load(f)
    assert hashlib.sha256(runs['bytes']('plain')).hexdigest() == recorded['plain']
    assert runs['bytes']('plain') == runs['bytes']('plain_old')
    assert ' | sense=' not in VS.done_line(runs['log']['plain']) and sorted(os.listdir(runs['tmp'] / 'plain')) == ['predicted_t1ce.nii.gz']


def test_dropped_slices_are_not_measured(runs):
    rep = runs['report']('drop')
    assert rep['measured_per_slice'] == [True] * 3 + [False] * 3 + [True] * 3 and rep['measured_slices'] == 6 and rep['unmeasured_slices'] == 3
    assert rep['drop_slices'] == [[3, 5]] and rep['residual_per_slice'][3:6] == [None] * 3
    _residuals_fall(rep)
    drop, sn = runs['pred']('drop'), runs['pred']('sn')
    assert (drop[:, :, 3:6] != sn[:, :, 3:6]).any()           # sampled freely there ...
    assert np.array_equal(drop[:, :, :3], sn[:, :, :3]) and np.array_equal(drop[:, :, 6:], sn[:, :, 6:])      # ... and the others do not notice


def test_ensemble_and_baseline(runs):
    tmp = runs['tmp']
    assert sorted(os.listdir(tmp / 'ens')) == ['predicted_t1ce.nii.gz', 'predicted_t1ce_std.nii.gz', 'sense_t1ce.json']
    mean, std = runs['pred']('ens'), runs['pred']('ens', '_std')
    assert np.isfinite(mean).all() and np.isfinite(std).all() and std.any()
    _residuals_fall(runs['report']('ens'))                     # the largest over both samples
    assert f' | 2 samples per slice | sense=equispaced x2 {NC} coils' in VS.done_line(runs['log']['ens'])
    assert sorted(os.listdir(tmp / 'base')) == ['metrics_sense_baseline_t1ce.json', 'metrics_t1ce.json', 'predicted_t1ce.nii.gz',
                                                'sense_baseline_t1ce.nii.gz', 'sense_t1ce.json']
    assert runs['bytes']('base') == runs['bytes']('sn')
    got = runs['vol'](tmp / 'base' / 'sense_baseline_t1ce.nii.gz')
    # against the restatement: lambda (I + lambda N)^-1 A^H y = the step, clean, from x_new = 0.  1e-5 on the [0,1] map: the bar the
    # zero-filled baseline of --known_kspace is held to; the kernel's error on these operands is of the order of 1e-6 per pixel
    from mudiff_hip import kspace as KS_, volume as V
    k = np.moveaxis(np.asarray(V.normalise_volume(np.asarray(runs['vol'](runs['p']['K']), np.float64)), np.float32).astype(np.float64), 2, 0)
    m = KS_.build_mask(S, 'equispaced', 2, 0.08, 0, seed=31)[None]
    maps = R.coil_maps(S, NC).astype(np.complex64)
    ahy = R.adjoint(R.measure(k, maps, m).astype(np.complex64), maps).astype(np.float32)
    want = np.clip(0.5 * R.constrain(np.zeros_like(k), ahy, maps, m, LAM, ITERS, None, None, 0, None, None, True) + 0.5, 0, 1)
    print(f'baseline against the restatement: {np.abs(np.moveaxis(got, 2, 0) - want).max():.3e}')
    assert np.abs(np.moveaxis(got, 2, 0) - want).max() <= 1e-5
    both = [json.load(open(tmp / 'base' / f)) for f in ('metrics_t1ce.json', 'metrics_sense_baseline_t1ce.json')]
    assert both[0].keys() == both[1].keys()


def test_measurement_noise_is_a_function_of_the_seed(runs):
    clean, noise, again, other = (runs['report'](k) for k in ('sn', 'noise', 'noise_again', 'noise_seed'))
    assert noise['noise'] == 0.05 and noise['y_norm_per_slice'] != clean['y_norm_per_slice']
    assert noise == again and runs['bytes']('noise') == runs['bytes']('noise_again')          # whatever the batch size
    assert other['y_norm_per_slice'] != noise['y_norm_per_slice']
    _residuals_fall(noise)
    # the floor sigma sqrt(2 * measured coefficients) / |y| is what the noise alone leaves of |A k - y| / |y|
    M = int(round(noise['sampling_fraction'] * S * S))
    for f, yn in zip(noise['noise_floor_per_slice'], noise['y_norm_per_slice']):
        assert f == pytest.approx(0.05 * np.sqrt(2 * M * NC) / yn, rel=1e-6)
