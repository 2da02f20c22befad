"""GPU: whole-volume scoring (csrc/volume_metrics.hip, ops.volume_metrics, mudiff_hip.volume_metrics, the volume pipeline's
--gt_volume / --eval_mask) against the fp64 restatement in tests/volume_metrics_ref.py, plus exact identities and determinism."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import PKG, REPO
import volume_metrics_ref as R
import volume_support as VS

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
TOL_SSIM, TOL_PSNR, TOL_MAE, TOL_R = 1e-9, 1e-8, 1e-10, 1e-10
NAMES = ('slab', 'brain', 'tumor', 'healthy')


def _case(shape, seed):
    """[Z, X, Y] fp32 pred / gt in [0, 1] with a flat block, region bits of the four regions, and a std correlated with the error."""
    rng = np.random.default_rng(seed)
    g = rng.random(shape, dtype=np.float32)
    g[: shape[0] // 2, :9, :9] = 0.4                              # flat: sigma^2 << mu^2
    p = np.clip(g + 0.08 * rng.standard_normal(shape), 0, 1).astype(np.float32)
    brain, tumor = rng.random(shape) < 0.7, rng.random(shape) < 0.25
    region = (1 | brain.astype(np.uint8) << 1 | tumor.astype(np.uint8) << 2 | (brain & ~tumor).astype(np.uint8) << 3).astype(np.uint8)
    std = (0.02 * rng.random(shape) + 0.5 * np.abs(p - g)).astype(np.float32)
    return p, g, region, std


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _close(a, b, tol):
    if a is None or b is None:
        return a is None and b is None
    if math.isinf(a) or math.isinf(b):
        return a == b
    return abs(a - b) <= tol


def _check_against_ref(rep, ref, names, with_std):
    for name in names:
        m, r = rep['metrics'][name], ref[name]
        assert (m['voxels'], m['interior_voxels']) == (r['voxels'], r['interior_voxels']), name
        assert _close(m['ssim3d'], r['ssim3d'], TOL_SSIM), (name, m['ssim3d'], r['ssim3d'])
        assert _close(m['psnr'], r['psnr'], TOL_PSNR), (name, m['psnr'], r['psnr'])
        assert _close(m['mae'], r['mae'], TOL_MAE), (name, m['mae'], r['mae'])
        pp = rep['per_plane'][name]
        for key, tol in (('ssim3d', TOL_SSIM), ('psnr', TOL_PSNR), ('mae', TOL_MAE)):
            assert len(pp[key]) == len(r['per_plane'][key])
            for z, (a, b) in enumerate(zip(pp[key], r['per_plane'][key])):
                assert _close(a, b, tol), (name, key, z, a, b)
        if with_std:
            u = rep['uncertainty'][name]
            assert _close(u['mean_std'], r['mean_std'], TOL_MAE), (name, u, r['mean_std'])
            assert _close(u['pearson_r'], r['pearson_r'], TOL_R), (name, u, r['pearson_r'])


@pytest.mark.parametrize('shape,seed', [((19, 37, 45), 0), ((23, 64, 64), 1), ((40, 21, 133), 2)])
def test_matches_the_restatement(shape, seed):
    from mudiff_hip import volume_metrics as VM
    p, g, region, std = _case(shape, seed)
    rep = VM.score_volume(_dev(p), _dev(g), _dev(region), _dev(std), NAMES)
    _check_against_ref(rep, R.score(p, g, region, NAMES, std=std), NAMES, True)
    rep2 = VM.score_volume(_dev(p), _dev(g), _dev(region), None, NAMES[:2])
    assert 'uncertainty' not in rep2
    assert rep2['metrics'] == {k: rep['metrics'][k] for k in NAMES[:2]}


def test_identical_volumes_give_exactly_one():
    from mudiff_hip import volume_metrics as VM
    p, _, region, _ = _case((21, 30, 70), 4)
    rep = VM.score_volume(_dev(p), _dev(p), _dev(region), None, NAMES)
    for name in NAMES:
        m = rep['metrics'][name]
        assert m['voxels'] > 0 and m['ssim3d'] == 1.0 and m['psnr'] == math.inf and m['mae'] == 0.0, (name, m)
        assert all(v is None or v == 1.0 for v in rep['per_plane'][name]['ssim3d'])


def test_known_offset_on_one_region():
    from mudiff_hip import ops
    from mudiff_hip import volume_metrics as VM
    rng = np.random.default_rng(5)
    shape, c = (15, 20, 30), 0.125
    g = (rng.integers(0, 512, shape) / 1024.0).astype(np.float32)     # multiples of 2^-10 below 0.5: g + c is exact in fp32
    _, _, region, _ = _case(shape, 5)
    brain = (region >> 1) & 1 == 1
    p = np.where(brain, g + np.float32(c), g).astype(np.float32)
    rep = VM.score_volume(_dev(p), _dev(g), _dev(region), None, NAMES)
    b = rep['metrics']['brain']
    assert b['mae'] == c and abs(b['psnr'] - (-20 * math.log10(c))) <= 1e-12
    assert rep['metrics']['tumor']['voxels'] > 0
    sums = ops.volume_metrics(_dev(p), _dev(g), _dev(region), None, nreg=4).cpu().numpy()
    outside = ((region >> 1) & 1 == 0)
    assert sums[:, 0, ops.VM_N].sum() == p.size and sums[:, 1, ops.VM_N].sum() == brain.sum()
    assert not (p[outside] != g[outside]).any()


def test_region_identities():
    from mudiff_hip import volume_metrics as VM
    shape = (25, 50, 70)
    p, g, _, std = _case(shape, 6)
    rng = np.random.default_rng(6)
    brain = rng.random(shape) < 0.7
    tumor = brain & (rng.random(shape) < 0.3)                        # a segmentation inside the brain
    region = (1 | brain.astype(np.uint8) << 1 | tumor.astype(np.uint8) << 2 | (brain & ~tumor).astype(np.uint8) << 3).astype(np.uint8)
    m = VM.score_volume(_dev(p), _dev(g), _dev(region), _dev(std), NAMES)['metrics']
    b, t, h = m['brain'], m['tumor'], m['healthy']
    assert b['voxels'] == t['voxels'] + h['voxels'] and b['interior_voxels'] == t['interior_voxels'] + h['interior_voxels']
    for k in ('sse', 'sae'):
        assert abs(t[k] + h[k] - b[k]) <= 1e-12 * b[k], k


def test_two_runs_are_bit_identical():
    from mudiff_hip import ops
    p, g, region, std = _case((33, 47, 90), 7)
    a = ops.volume_metrics(_dev(p), _dev(g), _dev(region), _dev(std), nreg=4)
    b = ops.volume_metrics(_dev(p), _dev(g), _dev(region), _dev(std), nreg=4)
    assert torch.equal(a, b)


def test_slice2d_is_the_2d_driver_protocol():
    from mudiff_hip import metrics
    from mudiff_hip import volume_metrics as VM
    p, g, region, _ = _case((9, 40, 40), 8)
    rep = VM.score_volume(_dev(p), _dev(g), _dev(region), None, NAMES)
    d = metrics.score_device(_dev(p), _dev(g))
    assert rep['slice2d'] == {k: (int(d[k]) if k == 'count' else float(d[k])) for k in ('psnr', 'ssim', 'mae', 'count', 'global_min', 'global_max')}
    assert rep['slice2d']['count'] == 9


def test_bad_inputs_raise_value_error():
    from mudiff_hip import volume_metrics as VM
    p, g, region, _ = _case((9, 12, 12), 9)
    with pytest.raises(ValueError, match='one shape'):
        VM.score_volume(_dev(p), _dev(g[:, :11]), _dev(region), None, NAMES)
    with pytest.raises(ValueError, match='smaller than 7'):
        VM.score_volume(_dev(p[:6]), _dev(g[:6]), _dev(region[:6]), None, NAMES)
    p[4, 5, 6] = np.nan
    with pytest.raises(ValueError, match='NaN'):
        VM.score_volume(_dev(p), _dev(g), _dev(region), None, NAMES)


# ---------------------------------------------------------------------------------------------------
# the volume pipeline and the CLI
# ---------------------------------------------------------------------------------------------------
def _synthetic_case(tmp_path):
    from mudiff_hip import volume as V
    VS.write_tiny_model(tmp_path)
    rng = np.random.default_rng(0)
    aff = np.diag([1.0, 1.0, 2.5, 1.0])
    aff[:3, 3] = (-8, -8, 3)
    paths = {}
    for m in ('flair', 't2', 't1', 't1ce'):
        v = (100 + 50 * rng.random((16, 16, 9))) * (rng.random((16, 16, 9)) > 0.2)
        paths[m] = str(tmp_path / f'{m}.nii.gz')
        V.write_nifti(paths[m], v.astype(np.float32), aff)
    paths['seg'] = str(tmp_path / 'seg.nii.gz')
    V.write_nifti(paths['seg'], (rng.random((16, 16, 9)) < 0.3).astype(np.float32) * 4, aff)
    argv = VS.model_argv(tmp_path, 3, 4, '--input_flair', paths['flair'], '--input_t2', paths['t2'], '--input_t1', paths['t1'])
    return paths, argv


def test_predict_volume_scores_what_it_wrote(tmp_path):
    paths, argv = _synthetic_case(tmp_path)
    ev = ['--gt_volume', paths['t1ce'], '--eval_mask', paths['seg']]
    out = {k: str(tmp_path / k) for k in ('plain', 'eval', 'ens')}
    jobs = {'plain': argv, 'eval': argv + ev, 'ens': argv + ev + ['--num_samples', '3']}
    log = VS.run_plan(tmp_path, [VS.volume_step(k, a + ['--output_dir', out[k]]) for k, a in jobs.items()], 900)
    stdout = ''.join(log[k] for k in jobs)
    # the files scored once more, here (the scoring kernels need no MUD_DETERMINISTIC); through JSON like the reports they are compared with
    from mudiff_hip import volume_metrics as VM
    rescored = json.loads(json.dumps(dict(
        eval=VM.score_files(out['eval'] + '/predicted_t1ce.nii.gz', paths['t1ce'], paths['seg'], slice_half_range=3),
        ens=VM.score_files(out['ens'] + '/predicted_t1ce.nii.gz', paths['t1ce'], paths['seg'], out['ens'] + '/predicted_t1ce_std.nii.gz',
                           slice_half_range=3))))
    assert '[metrics] brain: PSNR ' in stdout and '[metrics] slice2d (8-bit, 7 planes)' in stdout
    lines = stdout.splitlines()
    done = [i for i, ln in enumerate(lines) if ln.startswith('[done] saved:')]
    assert len(done) == 3 and lines[done[1] + 1].startswith('[metrics] slab: ')
    with open(os.path.join(out['plain'], 'predicted_t1ce.nii.gz'), 'rb') as f1, open(os.path.join(out['eval'], 'predicted_t1ce.nii.gz'), 'rb') as f2:
        assert f1.read() == f2.read()                                          # scoring does not change the prediction
    assert not os.path.exists(os.path.join(out['plain'], 'metrics_t1ce.json'))
    got = json.load(open(os.path.join(out['eval'], 'metrics_t1ce.json')))
    assert got == rescored['eval']                                              # bit-identical: the same array, the same kernels
    assert got['slab'] == [1, 7] and got['regions'] == list(NAMES) and 'uncertainty' not in got
    ens = json.load(open(os.path.join(out['ens'], 'metrics_t1ce.json')))
    assert ens == rescored['ens'] and set(ens['uncertainty']) == set(NAMES)
    # against the restatement, from the written file
    from mudiff_hip import ops
    from mudiff_hip import volume as V
    for which, rep, std_name in (('eval', got, None), ('ens', ens, 'predicted_t1ce_std.nii.gz')):
        pred = VM.slab_planes(V.read_nifti(os.path.join(out[which], 'predicted_t1ce.nii.gz'))[0], 1, 7)
        raw = V.read_nifti(paths['t1ce'])[0]
        gt = ops.to_range_0_1(_dev(VM.slab_planes(V.robust_minmax_to_minus1_1(raw), 1, 7))).cpu().numpy()
        region, names = VM.region_mask(VM.slab_planes(raw, 1, 7, np.float64), VM.slab_planes(V.read_nifti(paths['seg'])[0], 1, 7, np.float64))
        std = None if std_name is None else VM.slab_planes(V.read_nifti(os.path.join(out[which], std_name))[0], 1, 7)
        _check_against_ref(rep, R.score(pred, gt, region, names, std=std), names, std is not None)


def test_cli(tmp_path):
    from mudiff_hip import volume as V
    rng = np.random.default_rng(11)
    gt = (100 * rng.random((20, 24, 15))) * (rng.random((20, 24, 15)) > 0.3)
    pred = rng.random((20, 24, 15)).astype(np.float32)
    V.write_nifti(str(tmp_path / 'gt.nii.gz'), gt.astype(np.float32), np.eye(4))
    V.write_nifti(str(tmp_path / 'pred.nii.gz'), pred, np.eye(4))
    V.write_nifti(str(tmp_path / 'bad.nii.gz'), pred[:, :, :14], np.eye(4))
    V.write_nifti(str(tmp_path / 'seg.nii.gz'), (rng.random((20, 24, 15)) < 0.2).astype(np.float32), np.eye(4))
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([REPO, PKG, os.environ.get('PYTHONPATH', '')]))
    cmd = [sys.executable, '-m', 'mudiff_hip.volume_metrics', '--gt', str(tmp_path / 'gt.nii.gz'), '--mask', str(tmp_path / 'seg.nii.gz'),
           '--slice_half_range', '5']
    ok = subprocess.run(cmd + ['--pred', str(tmp_path / 'pred.nii.gz'), '--json', str(tmp_path / 'm.json')], cwd=REPO, env=env,
                        stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert ok.returncode == 0, ok.stderr[-3000:]
    for name in NAMES:
        assert f'[metrics] {name}: PSNR ' in ok.stdout
    assert '[metrics] slice2d (8-bit, 11 planes)' in ok.stdout and json.load(open(tmp_path / 'm.json'))['slab'] == [2, 12]
    bad = subprocess.run(cmd + ['--pred', str(tmp_path / 'bad.nii.gz')], cwd=REPO, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                         text=True, timeout=600)
    assert bad.returncode != 0 and 'differ in shape' in bad.stderr
