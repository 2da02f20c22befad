"""GPU: --known_kspace end to end on the tiny model (mudiff_hip.kspace through mudiff_hip.volume and mudiff_hip.cohort; DESIGN.md section
5.26): 16 x 16 x 9 phantoms, S = 16, every run in one child process under MUD_DETERMINISTIC=1 (tests/volume_support.py)."""
import json
import os

import numpy as np
import pytest

import kspace_ref as R
import volume_support as VS

pytestmark = pytest.mark.gpu
S = 16
KS = ['--known_kspace', 'equispaced', '--kspace_accel', '2']


def _phantom(shape, i):
    x, y, z = np.meshgrid(*(np.arange(float(n)) for n in shape), indexing='ij')
    return (120 + 60 * np.sin(x / (3 + i) + 0.3 * z) * np.cos(y / (4.5 - i) - 0.2 * z) + 4 * z).astype(np.float32)


@pytest.fixture(scope='module')
def runs(tmp_path_factory):
    from mudiff_hip import volume as V
    tmp = tmp_path_factory.mktemp('kspace')
    VS.write_tiny_model(tmp)
    p = {k: str(tmp / f'{k}.nii.gz') for k in ('flair', 't2', 't1', 'K')}
    for i, k in enumerate(p):
        V.write_nifti(p[k], _phantom((16, 16, 9), i), np.eye(4))
    inputs = ['--input_flair', p['flair'], '--input_t2', p['t2'], '--input_t1', p['t1']]
    known = inputs + ['--known_volume', p['K']]
    jobs = {'plain': (5, inputs, {}), 'plain_old': (5, inputs, dict(strip=['known_kspace', 'kspace_'])),
            'ks': (5, known + KS, {}), 'ks_dev': (5, known + KS + ['--device_intake'], {}), 'ks_b2': (2, known + KS, {}),
            'full': (5, known + ['--known_kspace', 'equispaced', '--kspace_accel', '1'], {}), 'known_all': (5, known, {}),
            'drop': (5, known + KS + ['--known_drop_slices', '3:5'], {}), 'ens': (5, known + KS + ['--num_samples', '2'], {}),
            'zf': (5, known + KS + ['--kspace_zero_filled', '--gt_volume', p['K']], {})}
    steps = [VS.volume_step(k, VS.model_argv(tmp, 4, b) + a + ['--output_dir', str(tmp / k)], **o) for k, (b, a, o) in jobs.items()]
    manifest = tmp / 'cohort.tsv'
    manifest.write_text('id\tt1\tt1ce\tt2\tflair\tknown\ns0\t' + '\t'.join([p['t1'], '', p['t2'], p['flair'], p['K']]) + '\n')
    steps.append(VS.cohort_step('cohort', VS.model_argv(tmp, 4, 5) + KS + ['--manifest', str(manifest), '--output_dir', str(tmp / 'cohort')]))
    log = VS.run_plan(tmp, steps, 900, ignore='RuntimeWarning')
    vol = lambda path: V.read_nifti(str(path))[0]             # noqa: E731
    return dict(tmp=tmp, log=log, p=p, vol=vol, pred=lambda k, suffix='': vol(tmp / k / f'predicted_t1ce{suffix}.nii.gz'),
                bytes=lambda k: VS.payload(str(tmp / k / 'predicted_t1ce.nii.gz')), report=lambda k: json.load(open(tmp / k / 'kspace_t1ce.json')))


def _residuals_under_the_rule(rep):
    """Every measured slice: |M_eff (F(x) - y)| / |y| <= 3 * rule * (|x| + |y|) / |y| (the constraint's two transforms and the check's)."""
    worst = 0.0
    for r, m, xn, yn in zip(rep['residual_per_slice'], rep['measured_per_slice'], rep['x_norm_per_slice'], rep['y_norm_per_slice']):
        assert (r is None) == (not m)
        if m:
            assert yn > 0 and 0 <= r <= 3 * R.rule(S) * (xn + yn) / yn, (r, xn, yn)
            worst = max(worst, r)
    return worst


def test_report_and_residuals(runs):
    from mudiff_hip import kspace as KS_
    rep = runs['report']('ks')
    M = KS_.build_mask(S, 'equispaced', 2, 0.08, 0, seed=31)
    assert (rep['pattern'], rep['accel'], rep['center'], rep['axis'], rep['image_size'], rep['slab']) == ('equispaced', 2, 0.08, 0, S, [0, 8])
    assert rep['given_fraction'] == float(M.mean()) and rep['effective_fraction'] == float(R.symmetrise(M).mean()) >= rep['given_fraction']
    assert 0.5 <= rep['given_fraction'] < 1.0
    assert rep['measured_slices'] == 9 and rep['unmeasured_slices'] == 0 and rep['measured_per_slice'] == [True] * 9 and rep['resample'] == 1
    worst = _residuals_under_the_rule(rep)
    print(f'worst residual {worst:.3e} (rule {R.rule(S):.3e})')
    assert rep['max_residual'] == worst
    pred, plain = runs['pred']('ks'), runs['pred']('plain')
    assert pred.shape == (16, 16, 9) and np.isfinite(pred).all() and (pred != plain).any()
    assert VS.done_line(runs['log']['ks']).endswith(f" | kspace=equispaced x2 ({rep['effective_fraction']:.3f})")
    assert sorted(os.listdir(runs['tmp'] / 'ks')) == ['kspace_t1ce.json', 'predicted_t1ce.nii.gz']


def test_intake_batch_size_and_cohort_give_the_same_bytes(runs):
    assert runs['bytes']('ks') == runs['bytes']('ks_dev')
    assert runs['bytes']('ks') == runs['bytes']('ks_b2')
    assert runs['bytes']('ks') == VS.payload(str(runs['tmp'] / 'cohort' / 's0' / 'predicted_t1ce.nii.gz'))
    assert json.load(open(runs['tmp'] / 'cohort' / 's0' / 'kspace_t1ce.json')) == runs['report']('ks') == runs['report']('ks_b2')
    assert VS.done_line(runs['log']['cohort']).endswith(VS.done_line(runs['log']['ks']).split(' | slices=')[1])


def test_without_the_flags_nothing_changes(runs):
    """The run without the flags writes the bytes the commit before them wrote (recorded: tests/golden/kspace_parent_payloads.json), a
    namespace as the parser left it before these flags existed gives the same, and those runs write nothing new."""
    import hashlib
    from conftest import REPO
    with open(os.path.join(REPO, 'tests', 'golden', 'kspace_parent_payloads.json')) as f:
        recorded = json.load(f)
    assert hashlib.sha256(runs['bytes']('plain')).hexdigest() == recorded['plain']
    assert runs['bytes']('plain') == runs['bytes']('plain_old')
    assert ' | kspace=' not in VS.done_line(runs['log']['plain']) and sorted(os.listdir(runs['tmp'] / 'plain')) == ['predicted_t1ce.nii.gz']
    assert sorted(os.listdir(runs['tmp'] / 'known_all')) == ['known_t1ce.json', 'predicted_t1ce.nii.gz']
    assert ' | kspace=' not in VS.done_line(runs['log']['known_all'])


def test_acceleration_one_returns_the_known_volume(runs):
    rep = runs['report']('full')
    assert rep['given_fraction'] == rep['effective_fraction'] == 1.0
    _residuals_under_the_rule(rep)
    a, b = runs['pred']('full').astype(np.float64), runs['pred']('known_all').astype(np.float64)      # b: K itself, pasted
    err = np.sqrt(((a - b) ** 2).sum((0, 1)))
    bound = 0.5 * 3 * R.rule(S) * (np.array(rep['x_norm_per_slice']) + np.array(rep['y_norm_per_slice'])) + S * 2.0 ** -23
    print(f'accel 1 against --known_volume: worst per-slice L2 {err.max():.3e} (bound {bound.min():.3e})')
    assert (err <= bound).all() and b.any()


def test_dropped_slices_are_not_measured(runs):
    rep = runs['report']('drop')
    assert rep['measured_per_slice'] == [True] * 3 + [False] * 3 + [True] * 3 and rep['measured_slices'] == 6 and rep['unmeasured_slices'] == 3
    assert rep['drop_slices'] == [[3, 5]] and rep['residual_per_slice'][3:6] == [None] * 3
    _residuals_under_the_rule(rep)
    drop, ks = runs['pred']('drop'), runs['pred']('ks')
    assert (drop[:, :, 3:6] != ks[:, :, 3:6]).any()           # sampled freely there ...
    assert np.array_equal(drop[:, :, :3], ks[:, :, :3]) and np.array_equal(drop[:, :, 6:], ks[:, :, 6:])      # ... and the others do not notice


def test_ensemble_and_zero_filled(runs):
    tmp = runs['tmp']
    assert sorted(os.listdir(tmp / 'ens')) == ['kspace_t1ce.json', 'predicted_t1ce.nii.gz', 'predicted_t1ce_std.nii.gz']
    mean, std = runs['pred']('ens'), runs['pred']('ens', '_std')
    assert np.isfinite(mean).all() and np.isfinite(std).all() and std.any()
    _residuals_under_the_rule(runs['report']('ens'))           # the largest over both samples
    assert ' | 2 samples per slice | kspace=equispaced x2 (' in VS.done_line(runs['log']['ens'])
    assert sorted(os.listdir(tmp / 'zf')) == ['kspace_t1ce.json', 'metrics_t1ce.json', 'metrics_zero_filled_t1ce.json', 'predicted_t1ce.nii.gz',
                                              'zero_filled_t1ce.nii.gz']
    assert runs['bytes']('zf') == runs['bytes']('ks')
    zf = runs['vol'](tmp / 'zf' / 'zero_filled_t1ce.nii.gz')
    from mudiff_hip import kspace as KS_, volume as V
    k = np.moveaxis(np.asarray(V.normalise_volume(np.asarray(runs['vol'](runs['p']['K']), np.float64)), np.float32).astype(np.float64), 2, 0)
    m = R.symmetrise(KS_.build_mask(S, 'equispaced', 2, 0.08, 0, seed=31))[None]
    want = np.clip(0.5 * R.fft2(R.measure(k, m), inverse=True).real + 0.5, 0, 1)
    assert np.abs(np.moveaxis(zf, 2, 0) - want).max() <= 1e-5
    both = [json.load(open(tmp / 'zf' / f)) for f in ('metrics_t1ce.json', 'metrics_zero_filled_t1ce.json')]
    assert both[0].keys() == both[1].keys()


def test_with_the_flags_the_bytes_are_those_of_the_separate_code_paths(runs):
    """The three modes share one constraint path (mudiff_hip.constraints): the runs with the flags write the bytes, and report the
    residuals, that the commit before it wrote (recorded there: tests/golden/constraint_parent_payloads.json)."""
    import hashlib
    from conftest import REPO
    with open(os.path.join(REPO, 'tests', 'golden', 'constraint_parent_payloads.json')) as f:
        recorded = json.load(f)['kspace']
    for job, suffix in (('ks', ''), ('ens', ''), ('ens', '_std')):
        got = VS.payload(str(runs['tmp'] / job / f'predicted_t1ce{suffix}.nii.gz'))
        assert hashlib.sha256(got).hexdigest() == recorded[job + suffix], job + suffix
    for job in ('ks', 'ens'):
        assert runs['report'](job)['max_residual'] == recorded[job + '_max_residual'], job
