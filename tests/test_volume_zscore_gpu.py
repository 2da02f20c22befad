"""GPU: --norm zscore.  mud_volume_slab_zscore against the host function, `python -m mudiff_hip.volume --norm
zscore` with and without --device_intake, `python -m mudiff_hip.cohort --norm zscore`, and the scoring of a ground truth mapped by
the same rule.  Every comparison is exact."""
import json
import os

import numpy as np
import pytest
import torch

import volume_intake_ref as R
import volume_support as VS

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _host_stack(vol, scale, half):
    from mudiff_hip import volume as V
    host64 = vol.astype(np.float64)
    if R.is_scaled(*scale):
        host64 = host64 * float(np.float32(scale[0])) + float(np.float32(scale[1]))
    with np.errstate(invalid='ignore'):
        slices, s0, s1 = V.extract_center_slices(V.zscore_to_minus1_1(host64), half)
    return torch.from_numpy(np.stack(slices, 0))[:, None], s0, s1


def _same(got, want):
    """torch.equal, with NaN equal to NaN at the same places."""
    got = got.cpu()
    return got.dtype == want.dtype and got.shape == want.shape and torch.equal(torch.isnan(got), torch.isnan(want)) and \
        torch.equal(torch.nan_to_num(got, nan=7.0), torch.nan_to_num(want, nan=7.0))


def _check_slab(vol, scale, half):
    from mudiff_hip import volume_intake as VI
    want, s0, s1 = _host_stack(vol, scale, half)
    raw = VS.raw_volume(vol, scale)
    slope, inter = (raw.slope, raw.inter) if raw.scaled else (1.0, 0.0)
    with np.errstate(invalid='ignore'):
        mean, std = VI.zscore_moments(raw)
    t = VI.slab_zscore(VI.upload(raw, DEV), raw.code, vol.shape, slope, inter, mean, std, s0, s1)
    assert tuple(t.shape) == (s1 - s0 + 1, 1) + vol.shape[:2] and _same(t, want)
    if vol.shape[0] == vol.shape[1]:
        with np.errstate(invalid='ignore'):
            assert _same(VI.condition_from_raw(raw, half, vol.shape[0], DEV, norm='zscore'), want)
    return mean, std, want


@pytest.mark.parametrize('dtype', ['u1', 'i2', 'u2', 'i4', 'f4'])
@pytest.mark.parametrize('scale', [(1.0, 0.0), (0.0123, -5.5)], ids=['unscaled', 'scaled'])
@pytest.mark.parametrize('shape,half', [((37, 29, 11), 3), ((130, 65, 7), 20), ((64, 70, 9), 2), ((48, 48, 9), 2)])
def test_slab_zscore_is_the_host_function(dtype, scale, shape, half):
    """zscore_moments -> slab z-score == zscore_to_minus1_1 + extract_center_slices + stack: sizes that are not multiples of the 64 x 64
    tile, slabs shorter than the volume and the whole volume."""
    mean, std, want = _check_slab(R.synthetic(shape, 'noise' if dtype == 'f4' else 'ties', dtype, seed=21), scale, half)
    assert std != 1.0 and float(want.min()) < 0 < float(want.max())


def test_slab_zscore_clamps_both_tails():
    vol = R.synthetic((70, 66, 9), 'noise', 'f4', seed=22)
    vol[5, 5, 4], vol[60, 65, 5] = 1.0e6, -1.0e6
    _, _, want = _check_slab(vol, (1.0, 0.0), 3)
    assert float(want.max()) == 1.0 and float(want.min()) == -1.0


@pytest.mark.parametrize('kind', ['zeros', 'constant'])
def test_slab_zscore_std_fallbacks(kind):
    """No non-zero voxel: mean 0, std 1 (zeros out); a flat volume: std 0 -> 1 (0 inside, the background clamped to -1)."""
    vol = R.synthetic((37, 29, 11), 'zeros' if kind == 'zeros' else 'ties', 'i2', seed=23)
    if kind == 'constant':
        vol = np.asfortranarray(np.where(vol != 0, 7, 0).astype(np.int16))
    mean, std, want = _check_slab(vol, (1.0, 0.0), 4)
    assert std == 1.0 and mean == (0.0 if kind == 'zeros' else 7.0)
    assert set(np.unique(want.numpy()).tolist()) == ({0.0} if kind == 'zeros' else {-1.0, 0.0})


def test_slab_zscore_keeps_nan():
    """A NaN voxel makes the host's moments NaN and with them every voxel; with finite moments forced, only the NaN voxel stays NaN
    (the clamp must not turn it into a bound)."""
    from mudiff_hip import volume_intake as VI
    vol = R.synthetic((37, 29, 11), 'noise', 'f4', seed=24)
    vol[3, 4, 5] = np.nan
    mean, std, want = _check_slab(vol, (1.0, 0.0), 4)
    assert np.isnan(mean) and np.isnan(std) and bool(torch.isnan(want).all())
    m, s = np.float32(12.5), np.float32(800.0)
    t = VI.slab_zscore(VI.upload(VS.raw_volume(vol), DEV), R.CODES['f4'], vol.shape, 1.0, 0.0, m, s, 1, 9).cpu()
    ref = torch.clamp(torch.from_numpy(np.ascontiguousarray(np.moveaxis((vol - m) / s, 2, 0)[1:10])), -3.0, 3.0) / 3.0
    assert _same(t[:, 0], ref) and int(torch.isnan(t).sum()) == 1 and bool(torch.isnan(t[4, 0, 3, 4]))


def test_c_abi_rejects_bad_arguments_without_launching():
    import mudiff_hip
    lib = mudiff_hip.load()
    vol = torch.zeros(16 * 16 * 4, dtype=torch.int16, device=DEV)
    out = torch.full((4, 16, 16), 5.0, device=DEV)
    z = lambda v, code, s0, s1, std=1.0, o=out: lib.mud_volume_slab_zscore(v, code, 16, 16, 4, 1.0, 0.0, 0.0, std, s0, s1,          # noqa: E731
                                                                           None if o is None else o.data_ptr(), None)
    assert z(vol.data_ptr(), 4, 1, 4) == 1 and b'slab' in lib.mud_last_error()
    assert z(vol.data_ptr(), 4, 2, 1) == 1 and z(vol.data_ptr(), 4, -1, 2) == 1
    assert z(vol.data_ptr(), 64, 0, 3) == 1 and b'datatype' in lib.mud_last_error()
    assert z(None, 4, 0, 3) == 1 and z(vol.data_ptr(), 4, 0, 3, o=None) == 1 and z(vol.data_ptr() + 2, 4, 0, 3) == 1
    assert z(vol.data_ptr(), 4, 0, 3, std=0.0) == 1 and b'std' in lib.mud_last_error()
    torch.cuda.synchronize()
    assert float(out.min()) == 5.0 and float(out.max()) == 5.0                                  # nothing was launched
    assert z(vol.data_ptr(), 4, 1, 2) == 0                                                      # the library still works afterwards
    torch.cuda.synchronize()
    assert not out[:2].any() and float(out[2:].min()) == 5.0


# ---------------------------------------------------------------------------------------------------
# scoring: the ground truth goes through the same rule
# ---------------------------------------------------------------------------------------------------
def test_a_prediction_equal_to_the_mapped_ground_truth_scores_perfectly_only_in_its_own_mode(tmp_path):
    from mudiff_hip import ops
    from mudiff_hip import volume as V
    from mudiff_hip import volume_metrics as VM
    gt = R.synthetic((37, 29, 15), 'ties', 'i2', seed=25)
    gt_path = R.write_nifti_typed(tmp_path / 'gt.nii.gz', gt)
    mapped = V.zscore_to_minus1_1(V.read_nifti(gt_path)[0])
    pred = ops.to_range_0_1(torch.from_numpy(np.ascontiguousarray(mapped)).to(DEV)).cpu().numpy()
    V.write_nifti(str(tmp_path / 'pred.nii.gz'), pred, np.eye(4))
    reps = {}
    for norm in ('zscore', 'percentile'):
        js = str(tmp_path / f'{norm}.json')
        assert VM.main(['--pred', str(tmp_path / 'pred.nii.gz'), '--gt', gt_path, '--slice_half_range', '5', '--json', js] +
                       (['--norm', norm] if norm == 'zscore' else [])) == 0
        reps[norm] = json.load(open(js))
    assert reps['zscore']['norm'] == 'zscore' and 'norm' not in reps['percentile']
    assert list(reps['percentile']) == ['shape', 'slab', 'regions', 'metrics', 'per_plane', 'slice2d']          # the keys it had
    for region in ('slab', 'brain'):
        m = reps['zscore']['metrics'][region]
        print(region, 'zscore', m['ssim3d'], m['mae'], 'percentile', reps['percentile']['metrics'][region]['ssim3d'],
              reps['percentile']['metrics'][region]['mae'])
        assert m['ssim3d'] == 1.0 and m['mae'] == 0.0 and m['psnr'] == float('inf')
        d = reps['percentile']['metrics'][region]
        assert d['ssim3d'] < 1.0 and d['mae'] > 0.0


# ---------------------------------------------------------------------------------------------------
# end to end: the volume CLI with and without --device_intake, then the cohort
# ---------------------------------------------------------------------------------------------------
def _subject(root, sid, shape, seed, dtype='i2', scale=(0.0, 0.0)):
    rng = np.random.default_rng(seed)
    os.makedirs(root / sid)
    aff = np.diag([1.0, 1.0, 2.5, 1.0])
    paths = {}
    for m in ('t1', 't1ce', 't2', 'flair'):
        v = (rng.integers(100, 150, shape) * (rng.random(shape) > 0.2)).astype(dtype)
        paths[m] = R.write_nifti_typed(root / sid / f'{sid}_{m}.nii.gz', np.asfortranarray(v), '<', *scale, affine=aff)
    seg = ((rng.random(shape) < 0.3) * 4).astype('u1')
    paths['seg'] = R.write_nifti_typed(root / sid / f'{sid}_seg.nii.gz', np.asfortranarray(seg), affine=aff)
    return paths


def test_zscore_runs_write_the_same_files_through_every_path(tmp_path):
    VS.write_tiny_model(tmp_path)
    model = VS.model_argv(tmp_path, 3, 4, '--resize_back', '--norm', 'zscore')
    data = tmp_path / 'brats'
    subjects = {'s_a': _subject(data, 's_a', (16, 16, 9), 1), 's_b': _subject(data, 's_b', (20, 12, 11), 2, scale=(0.5, 3.0))}
    (tmp_path / 'test.list').write_text('s_a\ns_b\n')
    single = {}
    for sid in ('s_a', 's_b'):
        p = subjects[sid]
        inputs = ['--input_flair', p['flair'], '--input_t2', p['t2'], '--input_t1', p['t1'], '--gt_volume', p['t1ce'], '--eval_mask', p['seg']]
        host, dev = str(tmp_path / f'{sid}_host'), str(tmp_path / f'{sid}_dev')
        a = VS.run_module('mudiff_hip.volume', model + inputs + ['--output_dir', host])
        b = VS.run_module('mudiff_hip.volume', model + inputs + ['--output_dir', dev, '--device_intake'])
        assert VS.payload(host + '/predicted_t1ce.nii.gz') == VS.payload(dev + '/predicted_t1ce.nii.gz')
        rep = json.load(open(host + '/metrics_t1ce.json'))
        assert rep == json.load(open(dev + '/metrics_t1ce.json')) and rep['norm'] == 'zscore'
        assert a.stdout.replace(host, 'OUT') == b.stdout.replace(dev, 'OUT')      # the same lines, too
        done = [ln for ln in a.stdout.splitlines() if ln.startswith('[done]')]
        assert len(done) == 1 and done[0].endswith(' | norm=zscore')
        single[sid] = host
    # the mode changes the prediction: the default run of the same subject writes another file, and says nothing about a mode
    p = subjects['s_a']
    d = VS.run_module('mudiff_hip.volume', [m for m in model if m not in ('--norm', 'zscore')] +
             ['--input_flair', p['flair'], '--input_t2', p['t2'], '--input_t1', p['t1'], '--output_dir', str(tmp_path / 'default')])
    assert VS.payload(str(tmp_path / 'default' / 'predicted_t1ce.nii.gz')) != VS.payload(single['s_a'] + '/predicted_t1ce.nii.gz')
    assert 'norm=' not in d.stdout
    # an ensemble through both paths (mean and std volumes)
    p = subjects['s_b']
    inputs = ['--input_flair', p['flair'], '--input_t2', p['t2'], '--input_t1', p['t1'], '--num_samples', '2']
    e = VS.run_module('mudiff_hip.volume', model + inputs + ['--output_dir', str(tmp_path / 'ens_host')])
    VS.run_module('mudiff_hip.volume', model + inputs + ['--output_dir', str(tmp_path / 'ens_dev'), '--device_intake'])
    for name in ('predicted_t1ce.nii.gz', 'predicted_t1ce_std.nii.gz'):
        assert VS.payload(str(tmp_path / 'ens_host' / name)) == VS.payload(str(tmp_path / 'ens_dev' / name))
    assert [ln for ln in e.stdout.splitlines() if ln.startswith('[done]')][0].endswith(' | norm=zscore')
    # the cohort: both subjects, moments on the prefetch thread
    out = tmp_path / 'cohort'
    c = VS.run_module('mudiff_hip.cohort', model + ['--brats_root', str(data), '--subjects', str(tmp_path / 'test.list'), '--score', '--output_dir',
                                           str(out), '--io_threads', '2'])
    assert c.stdout.count(' | norm=zscore') == 2
    for sid in ('s_a', 's_b'):
        assert VS.payload(str(out / sid / 'predicted_t1ce.nii.gz')) == VS.payload(single[sid] + '/predicted_t1ce.nii.gz')
        assert json.load(open(out / sid / 'metrics_t1ce.json')) == json.load(open(single[sid] + '/metrics_t1ce.json'))
    rep = json.load(open(out / 'cohort_t1ce.json'))
    assert rep['norm'] == 'zscore' and [r['id'] for r in rep['subjects']] == ['s_a', 's_b'] and rep['timing']['moments'] > 0
