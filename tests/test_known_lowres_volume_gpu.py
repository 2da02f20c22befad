"""GPU: --known_lowres_volume end to end on the tiny model (mudiff_hip.lowres_volume through mudiff_hip.volume and mudiff_hip.cohort;
DESIGN.md section 5.31): 16 x 16 x 9 thin phantoms at 1 mm, S = 16, and a Y made in the test from a smooth thin K by the dense
restatement of tests/lowres_ref.py - coarse voxels of 2 x 2 x 3 fine voxels, shifted by half a fine voxel on every axis (so every axis
has bandwidth 1), 8 x 8 x 3 of them, the last of each axis reaching past the grid - written with its own affine by the project's NIfTI
writer.  Every run in one child process under MUD_DETERMINISTIC=1 (tests/volume_support.py).
Measured on an MI355X: max_residual 1.26e-7 (single sample) against 1.27e-7 left by the fp32 emulation of the four passes on the same
Y from a random start; the rule is max_residual <= 4 x that."""
import json
import os

import numpy as np
import pytest

import band_ref
import lowres_ref as R
import volume_support as VS

pytestmark = pytest.mark.gpu
S, Z = 16, 9
Y_SHAPE = (8, 8, 3)
Y_AFFINE = np.array([[2.0, 0, 0, 1.0], [0, 2.0, 0, 1.0], [0, 0, 3.0, 1.5], [0, 0, 0, 1.0]])      # centres 1 + 2 j in-plane, 1.5 + 3 j along z


def _phantom(shape, i):
    x, y, z = np.meshgrid(*(np.arange(float(n)) for n in shape), indexing='ij')
    return (120 + 60 * np.sin(x / (3 + i) + 0.3 * z) * np.cos(y / (4.5 - i) - 0.2 * z) + 4 * z).astype(np.float32)


def _coarse_of(k):
    """Y of the thin volume k [X,Y,Z]: every coarse voxel, whether or not its support lies inside the grid."""
    rows = [np.stack([band_ref.row(n, Y_AFFINE[a, 3] + Y_AFFINE[a, a] * j, Y_AFFINE[a, a], 'box') for j in range(Y_SHAPE[a])])
            for a, n in enumerate((16, 16, Z))]
    return np.einsum('ax,by,cz,xyz->abc', rows[0], rows[1], rows[2], k.astype(np.float64)).astype(np.float32)


@pytest.fixture(scope='module')
def runs(tmp_path_factory):
    from mudiff_hip import volume as V
    tmp = tmp_path_factory.mktemp('lowres_volume')
    VS.write_tiny_model(tmp)
    p = {k: str(tmp / f'{k}.nii.gz') for k in ('flair', 't2', 't1', 'K')}
    for i, k in enumerate(p):
        V.write_nifti(p[k], _phantom((16, 16, Z), i), np.eye(4))
    Y = _coarse_of(_phantom((16, 16, Z), 3))
    p['Y'], p['Yrot'], p['regrid'] = (str(tmp / f'{k}.nii.gz') for k in ('Y', 'Yrot', 'Y_on_grid'))
    V.write_nifti(p['Y'], Y, Y_AFFINE)
    a = 0.2
    rot = np.array([[np.cos(a), -np.sin(a), 0, 0], [np.sin(a), np.cos(a), 0, 0], [0, 0, 1, 0], [0, 0, 0, 1.0]])
    V.write_nifti(p['Yrot'], Y, rot @ Y_AFFINE)
    inputs = ['--input_flair', p['flair'], '--input_t2', p['t2'], '--input_t1', p['t1']]
    lv = inputs + ['--known_lowres_volume', p['Y']]
    jobs = {'plain': (9, inputs, {}), 'lv': (9, lv, {}), 'lv_b4': (4, lv, {}), 'lv_dev': (9, lv + ['--device_intake'], {}),
            'base': (9, lv + ['--lowres_volume_baseline', '--gt_volume', p['K'], '--through_plane'], {}), 'ens': (9, lv + ['--num_samples', '2'], {}),
            'rot': (9, inputs + ['--known_lowres_volume', p['Yrot']], dict(raises=True))}
    steps = [VS.volume_step(k, VS.model_argv(tmp, 4, b) + a_ + ['--output_dir', str(tmp / k)], **o) for k, (b, a_, o) in jobs.items()]
    manifest = tmp / 'cohort.tsv'
    manifest.write_text('id\tt1\tt1ce\tt2\tflair\tknown\ns0\t' + '\t'.join([p['t1'], '', p['t2'], p['flair'], p['Y']]) + '\n')
    steps.append(VS.cohort_step('cohort', VS.model_argv(tmp, 4, 9) + ['--known_lowres_volume', 'manifest', '--manifest', str(manifest),
                                                                      '--output_dir', str(tmp / 'cohort')]))
    steps.append(VS.regrid_step(p['Y'], p['flair'], p['regrid']))
    log = VS.run_plan(tmp, steps, 900, ignore='RuntimeWarning')
    vol = lambda path: V.read_nifti(str(path))[0]             # noqa: E731
    return dict(tmp=tmp, log=log, p=p, vol=vol, Y=Y, pred=lambda k, suffix='': vol(tmp / k / f'predicted_t1ce{suffix}.nii.gz'),
                bytes=lambda k, suffix='': VS.payload(str(tmp / k / f'predicted_t1ce{suffix}.nii.gz')),
                report=lambda k: json.load(open(tmp / k / 'lowres_volume_t1ce.json')))


def _emulated_residual(Y):
    """The largest |A out - y| / |y| over the coarse slices that the fp32 emulation of the four passes leaves on this Y from a random
    start: what the arithmetic itself cannot go below."""
    import torch
    from mudiff_hip import lowres_volume as LV, ops
    geo = LV.voxel_geometry((16, 16, Z), np.eye(4), Y.shape, Y_AFFINE)
    opt = dict(volume='y', extent=None, profile='box', drop=[], baseline=False, resample=1)
    m = LV.measure(LV.LowresInputs(Y.astype(np.float64), geo, (16, 16, Z), opt, Y_AFFINE, np.eye(4), 'linear'), ((16, 16, Z), np.eye(4), None, 0, Z - 1),
                   S, 'percentile', torch.device('cpu'))
    tabs, y = ops.lowres_tables(*m.A), m.y.numpy()
    x = np.random.default_rng(11).standard_normal((Z, S, S)).astype(np.float32)
    d = R.measure_fp32(R.constrain_fp32(x, y, tabs), tabs) - y
    return max(float(np.linalg.norm(d[j]) / np.linalg.norm(y[j])) for j in range(y.shape[0])), m


def test_report_residual_and_done_line(runs):
    rep = runs['report']('lv')
    floor, m = _emulated_residual(runs['Y'])
    assert m.shape == (2, 7, 7)
    assert [rep['axes'][k]['measured'] for k in 'zyx'] == [2, 7, 7] and [rep['axes'][k]['coarse'] for k in 'zyx'] == [3, 8, 8]
    assert [(rep['axes'][k]['c0'], rep['axes'][k]['step'], rep['axes'][k]['width']) for k in 'zyx'] == [(1.5, 3.0, 3.0), (1.0, 2.0, 2.0), (1.0, 2.0, 2.0)]
    assert (rep['extent_mm'], rep['fine_mm'], rep['coarse_mm'], rep['profile'], rep['image_size'], rep['slab'], rep['resample']) == \
        ([2.0, 2.0, 3.0], [1.0, 1.0, 1.0], [2.0, 2.0, 3.0], 'box', S, [0, Z - 1], 1)
    assert [rep['axes'][k]['bandwidth'] for k in 'zyx'] == [1, 1, 1]
    assert rep['cond'] == pytest.approx(np.prod([rep['axes'][k]['cond'] for k in 'zyx'])) and rep['cond'] == pytest.approx(m.tables.cond, rel=1e-9)
    assert [s['measured'] for s in rep['slices']] == [True, True, False] and rep['slices'][2]['residual'] is None
    worst = max(s['residual'] for s in rep['slices'] if s['measured'])
    print(f'max_residual {rep["max_residual"]:.3e}; the fp32 emulation from a random start leaves {floor:.3e}')
    assert rep['max_residual'] == worst and all(s['y_norm'] > 0 for s in rep['slices'] if s['measured'])
    assert 0 <= rep['max_residual'] <= 4 * floor
    pred, plain = runs['pred']('lv'), runs['pred']('plain')
    assert pred.shape == (16, 16, Z) and np.isfinite(pred).all() and (pred != plain).any()
    assert VS.done_line(runs['log']['lv']).endswith(' | lowres_volume=2x2x3mm on 1x1x1mm box (2/3 slices, bw 1/1/1)')
    assert ' | lowres_volume=' not in VS.done_line(runs['log']['plain'])
    assert sorted(os.listdir(runs['tmp'] / 'lv')) == ['lowres_volume_t1ce.json', 'predicted_t1ce.nii.gz']


def test_batch_size_intake_and_cohort_give_the_same_bytes(runs):
    assert runs['bytes']('lv') == runs['bytes']('lv_b4')
    assert runs['bytes']('lv') == runs['bytes']('lv_dev')
    assert runs['bytes']('lv') == VS.payload(str(runs['tmp'] / 'cohort' / 's0' / 'predicted_t1ce.nii.gz'))
    assert json.load(open(runs['tmp'] / 'cohort' / 's0' / 'lowres_volume_t1ce.json')) == runs['report']('lv') == runs['report']('lv_b4')
    assert VS.done_line(runs['log']['cohort']).endswith(VS.done_line(runs['log']['lv']).split(' | slices=')[1])


def test_ensemble_writes_mean_and_std(runs):
    mean, std = runs['pred']('ens'), runs['pred']('ens', '_std')
    assert np.isfinite(mean).all() and np.isfinite(std).all() and (std > 0).any() and runs['bytes']('ens') != runs['bytes']('lv')
    floor, _ = _emulated_residual(runs['Y'])
    rep = runs['report']('ens')
    print(f'max_residual over two samples {rep["max_residual"]:.3e}; the fp32 emulation leaves {floor:.3e}')
    assert 0 <= rep['max_residual'] <= 4 * floor
    assert '2 samples per slice' in VS.done_line(runs['log']['ens'])


def test_baseline_is_the_regridded_scan(runs):
    out = runs['tmp'] / 'base'
    assert (out / 'lowres_volume_interp_t1ce.nii.gz').is_file() and (out / 'metrics_lowres_volume_interp_t1ce.json').is_file()
    assert (out / 'through_plane_lowres_volume_interp_t1ce.json').is_file()
    base, want = runs['vol'](out / 'lowres_volume_interp_t1ce.nii.gz'), runs['vol'](runs['p']['regrid'])
    assert base.shape == (16, 16, Z) and np.array_equal(base, want) and np.isfinite(base).all() and base.max() > 1
    assert runs['bytes']('base') == runs['bytes']('lv')
    assert '[lowres-volume-interp] ' in runs['log']['base']


def test_refusals_name_the_flag(runs, capsys):
    from mudiff_hip import volume as V
    err = runs['log']['rot']['error']
    assert '--known_lowres_volume' in err and 'not parallel' in err and 'out of scope' in err
    with pytest.raises(SystemExit):
        V.build_argparser(VS.cli_argv('--known_lowres_volume', runs['p']['Y'], '--known_volume', runs['p']['K']))
    assert '--known_lowres_volume cannot be combined with --known_volume' in capsys.readouterr().err
