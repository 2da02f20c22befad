"""CPU: the fp64 restatement of the volume scores (tests/volume_metrics_ref.py) against a brute-force loop, the volume pipeline's
evaluation flags (refused by predict_volume before any GPU work) and the report that mudiff_hip.volume_metrics builds from per-plane
sums."""
import json
import math

import numpy as np
import pytest

import volume_metrics_ref as R


def _volumes(shape, seed):
    rng = np.random.default_rng(seed)
    g = rng.random(shape)
    g[:, :2] = 0.25                                               # a flat band: sigma^2 far below mu^2
    p = np.clip(g + 0.1 * rng.standard_normal(shape), 0, 1)
    region = (1 | (rng.random(shape) < 0.6).astype(np.uint8) << 1).astype(np.uint8)
    return p, g, region, rng.random(shape) * 0.2


@pytest.mark.parametrize('shape,seed', [((9, 8, 7), 0), ((11, 10, 9), 1)])
def test_restatement_matches_brute_force(shape, seed):
    p, g, region, std = _volumes(shape, seed)
    fast, slow = R.ssim_map(p, g), R.ssim_map_brute(p, g)
    inner = R.interior(shape)
    assert np.isfinite(slow[inner]).all() and np.isnan(slow[~inner]).all()
    assert np.abs(fast[inner] - slow[inner]).max() <= 1e-12
    a = R.score(p, g, region, ('slab', 'brain'), std=std)
    b = R.score(p, g, region, ('slab', 'brain'), std=std, ssim=slow)
    for name in ('slab', 'brain'):
        sel = (region >> ('slab', 'brain').index(name)) & 1 == 1
        assert a[name]['voxels'] == int(sel.sum()) and a[name]['interior_voxels'] == int((sel & inner).sum())
        assert abs(a[name]['ssim3d'] - float(np.mean(slow[sel & inner]))) <= 1e-12
        assert abs(a[name]['ssim3d'] - b[name]['ssim3d']) <= 1e-12
        d = (p - g)[sel]
        assert a[name]['psnr'] == pytest.approx(-10 * math.log10(np.mean(d * d)), abs=1e-12)
        assert a[name]['mae'] == pytest.approx(np.mean(np.abs(d)), abs=1e-15)
        assert a[name]['pearson_r'] == pytest.approx(np.corrcoef(std[sel], np.abs(d))[0, 1], abs=1e-12)
        for z in range(shape[0]):                                   # per-plane SSIM3D only on planes 3..Z-4
            v = a[name]['per_plane']['ssim3d'][z]
            if 3 <= z < shape[0] - 3 and (sel[z] & inner[z]).any():
                assert abs(v - float(np.mean(slow[z][sel[z] & inner[z]]))) <= 1e-12
            else:
                assert v is None
    # for the whole slab the 3D SSIM is the plain mean of the cropped map (skimage's structural_similarity on 3D arrays)
    assert abs(a['slab']['ssim3d'] - float(slow[3:-3, 3:-3, 3:-3].mean())) <= 1e-12


def test_identical_volumes_score_exactly_one_in_the_restatement():
    p, _, region, _ = _volumes((9, 9, 9), 3)
    r = R.score(p, p, region, ('slab', 'brain'))
    assert r['slab']['psnr'] == math.inf and r['slab']['mae'] == 0.0
    assert abs(r['slab']['ssim3d'] - 1.0) <= 1e-15


# ---------------------------------------------------------------------------------------------------
# the volume pipeline's evaluation flags
# ---------------------------------------------------------------------------------------------------
def _nifti_inputs(tmp_path, shape=(16, 16, 9)):
    from mudiff_hip import volume as V
    rng = np.random.default_rng(0)
    paths = {}
    for m in ('flair', 't2', 't1'):
        paths[m] = str(tmp_path / f'{m}.nii.gz')
        V.write_nifti(paths[m], (100 + 50 * rng.random(shape)).astype(np.float32), np.eye(4))
    return paths


def _argv(tmp_path, paths, *extra, half_range='3'):
    return ['--target_modality', 'T1CE', '--exp', 'exp0', '--output_path', str(tmp_path / 'results'), '--image_size', '16',
            '--slice_half_range', half_range, '--input_flair', paths['flair'], '--input_t2', paths['t2'], '--input_t1', paths['t1'],
            '--output_dir', str(tmp_path / 'out'), *extra]


@pytest.fixture
def no_gpu_work(monkeypatch):
    """predict_volume must refuse bad evaluation inputs before it samples, loads a checkpoint or touches a device."""
    import torch
    from mudiff_hip import volume as V

    def touched(*a, **k):
        raise AssertionError('predict_volume went past its argument checks')
    monkeypatch.setattr(V, '_predict_volume', touched)
    monkeypatch.setattr(torch.cuda, 'set_device', touched)
    return V


def test_eval_mask_needs_gt_volume(tmp_path, no_gpu_work):
    V = no_gpu_work
    paths = _nifti_inputs(tmp_path)
    args = V.build_argparser(_argv(tmp_path, paths, '--eval_mask', paths['t1']))
    with pytest.raises(ValueError, match='--eval_mask needs --gt_volume'):
        V.predict_volume(args)


def test_gt_volume_of_another_shape_is_refused(tmp_path, no_gpu_work):
    V = no_gpu_work
    paths = _nifti_inputs(tmp_path)
    gt = str(tmp_path / 'gt.nii.gz')
    V.write_nifti(gt, np.ones((16, 15, 9), np.float32), np.eye(4))
    with pytest.raises(ValueError, match='differ in shape'):
        V.predict_volume(V.build_argparser(_argv(tmp_path, paths, '--gt_volume', gt)))
    mask = str(tmp_path / 'mask.nii.gz')
    V.write_nifti(mask, np.ones((16, 16, 8), np.float32), np.eye(4))
    with pytest.raises(ValueError, match='label mask'):
        V.predict_volume(V.build_argparser(_argv(tmp_path, paths, '--gt_volume', paths['t1'], '--eval_mask', mask)))


def test_slab_thinner_than_the_window_is_refused(tmp_path, no_gpu_work):
    V = no_gpu_work
    paths = _nifti_inputs(tmp_path)
    with pytest.raises(ValueError, match='at least 7'):
        V.predict_volume(V.build_argparser(_argv(tmp_path, paths, '--gt_volume', paths['t1'], half_range='2')))


def test_good_eval_inputs_reach_the_sampler(tmp_path, monkeypatch):
    from mudiff_hip import volume as V
    paths = _nifti_inputs(tmp_path)
    calls = []
    monkeypatch.setattr(V, '_predict_volume', lambda args, plan, evaluation=None: calls.append(evaluation))
    V.predict_volume(V.build_argparser(_argv(tmp_path, paths, '--gt_volume', paths['t1'], '--eval_mask', paths['t2'])))
    V.predict_volume(V.build_argparser(_argv(tmp_path, paths)))
    gt, label = calls[0]
    assert gt.shape == label.shape == (16, 16, 9) and calls[1] is None


def test_parser_defaults():
    from mudiff_hip import volume as V
    a = V.build_argparser(['--target_modality', 'T1CE', '--output_dir', 'o', '--exp', 'e'])
    assert a.gt_volume is None and a.eval_mask is None
    assert (a.num_channels_dae, a.slice_half_range, a.image_size, a.seed, a.num_timesteps, a.nz, a.batch_size, a.num_samples,
            a.resize_back) == (128, 80, 256, 1024, 4, 100, 32, None, False)
    from mudiff_hip import volume_metrics as VM
    c = VM.build_parser().parse_args(['--pred', 'p', '--gt', 'g'])
    assert (c.mask, c.std, c.json, c.slice_half_range) == (None, None, None, 80)


def test_slab_and_shape_checks():
    from mudiff_hip import volume as V
    from mudiff_hip import volume_metrics as VM
    for z in (7, 9, 155):
        for hr in (3, 4, 80):
            vol = np.zeros((1, 1, z))
            _, s0, s1 = V.extract_center_slices(vol, hr)
            assert VM.slab_range(z, hr) == (s0, s1)
    assert VM.check_shapes((8, 8, 9), (8, 8, 9), None, 3) == (1, 7)
    with pytest.raises(ValueError, match='in-plane'):
        VM.check_shapes((6, 8, 9), (6, 8, 9), None, 3)
    with pytest.raises(ValueError, match='std volume'):
        VM.check_shapes((8, 8, 9), (8, 8, 9), None, 3, std_shape=(8, 8, 8))


def test_region_mask_bits():
    from mudiff_hip import volume_metrics as VM
    gt = np.array([0.0, 1.0, 2.0, 0.0])
    m, names = VM.region_mask(gt)
    assert names == ('slab', 'brain') and m.tolist() == [1, 3, 3, 1]
    m, names = VM.region_mask(gt, np.array([0, 0, 4, 1]))
    assert names == ('slab', 'brain', 'tumor', 'healthy') and m.tolist() == [1, 1 | 2 | 8, 1 | 2 | 4, 1 | 4]


# ---------------------------------------------------------------------------------------------------
# report from fixed sums
# ---------------------------------------------------------------------------------------------------
def _fixed_sums():
    from mudiff_hip import ops
    s = np.zeros((3, 2, ops.VM_NQ))
    # region 0: plane 0 has no interior voxel, plane 1 is perfect, plane 2 has errors; region 1 is empty on plane 0
    s[0, 0, [ops.VM_N, ops.VM_SSE, ops.VM_SAE]] = (100, 1.0, 5.0)
    s[1, 0, [ops.VM_N, ops.VM_N_INT, ops.VM_SSIM]] = (100, 10, 10.0)
    s[2, 0, [ops.VM_N, ops.VM_SSE, ops.VM_SAE, ops.VM_N_INT, ops.VM_SSIM]] = (100, 0.01, 1.0, 10, 9.0)
    # region 1: s = 1, 2, 3, 4 and e = 2, 4, 6, 8 on plane 1 (r = 1); plane 2: constant std (r undefined on its own)
    s[1, 1, [ops.VM_N, ops.VM_SSE, ops.VM_SAE, ops.VM_SS, ops.VM_SS2, ops.VM_SSE_STD]] = (4, 120.0, 20.0, 10.0, 30.0, 60.0)
    return s


def test_report_from_fixed_sums(tmp_path):
    from mudiff_hip import volume_metrics as VM
    rep = VM.summarize(_fixed_sums(), ('slab', 'brain'), first_plane=5, has_std=True)
    assert rep['regions'] == ['slab', 'brain'] and rep['per_plane']['plane'] == [5, 6, 7]
    m = rep['metrics']['slab']
    assert (m['voxels'], m['interior_voxels']) == (300, 20)
    assert m['psnr'] == pytest.approx(10 * math.log10(300 / 1.01), abs=1e-12)
    assert m['ssim3d'] == pytest.approx(19.0 / 20, abs=1e-15) and m['mae'] == pytest.approx(6.0 / 300, abs=1e-15)
    pp = rep['per_plane']['slab']
    assert pp['psnr'][0] == pytest.approx(20.0) and pp['psnr'][1] == math.inf and pp['psnr'][2] == pytest.approx(40.0)
    assert pp['ssim3d'] == [None, 1.0, 0.9] and pp['mae'] == [0.05, 0.0, 0.01]
    b = rep['metrics']['brain']
    assert b['voxels'] == 4 and b['interior_voxels'] == 0 and b['ssim3d'] is None
    assert rep['per_plane']['brain']['psnr'][0] is None and rep['per_plane']['brain']['mae'][0] is None
    u = rep['uncertainty']
    assert u['brain']['mean_std'] == 2.5 and u['brain']['pearson_r'] == pytest.approx(1.0, abs=1e-12)
    assert u['slab']['mean_std'] == 0.0 and u['slab']['pearson_r'] is None          # std identically 0: no correlation
    assert 'slice2d' not in rep and 'uncertainty' not in VM.summarize(_fixed_sums(), ('slab', 'brain'))
    rep['slice2d'] = dict(psnr=30.0, ssim=0.9, mae=0.01, count=3, global_min=0.0, global_max=1.0)
    path = VM.write_json(rep, str(tmp_path / 'm.json'))
    back = json.load(open(path))
    assert back == rep                                                               # Infinity and null round-trip
    lines = VM.format_lines(rep)
    assert lines[0] == '[metrics] slab: PSNR 24.7280 dB | SSIM3D 0.950000 | MAE 0.020000 | voxels 300'
    assert lines[1] == '[metrics] brain: PSNR -14.7712 dB | SSIM3D n/a | MAE 5.000000 | voxels 4'
    assert lines[2] == '[metrics] slice2d (8-bit, 3 planes): PSNR 30.0000 dB | SSIM 0.9000 | MAE 0.010000'
    assert lines[3].startswith('[metrics] uncertainty slab: mean std 0.000000 | r(std, |err|) n/a')
    with pytest.raises(ValueError):
        VM.summarize(_fixed_sums(), ('slab',))
