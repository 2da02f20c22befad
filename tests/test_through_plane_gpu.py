"""GPU: the through-plane measure (csrc/volume_through_plane.hip, ops.volume_through_plane, mudiff_hip.volume_through_plane) against the
fp64 restatement in tests/slice_coupling_ref.py, its null entries, clipped slab ranges and the command line.  DESIGN.md section 5.23."""
import json

import numpy as np
import pytest
import torch

import slice_coupling_ref as R
import volume_support as VS

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
TOL = 1e-10                 # tests/test_volume_metrics_gpu.py: means of fp64 plane sums of values in [0, 1]
KEYS = ('mean_dz', 'mean_dzz', 'mean_dx', 'mean_dy', 'anisotropy')


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _close(a, b, tol=TOL):
    return (a is None and b is None) if a is None or b is None else abs(a - b) <= tol


def _check(rep, want):
    for k in KEYS:
        assert _close(rep[k], want[k], TOL if k != 'anisotropy' else 1e-9), (k, rep[k], want[k])
    assert len(rep['dz']) == len(want['dz']) and all(_close(a, b) for a, b in zip(rep['dz'], want['dz'])), (rep['dz'], want['dz'])


# 9 x 7 x 5: less than a wave per plane; 33 x 17 x 8: odd sizes; 5 x 70 x 67: more voxels per plane than one pass of the plane's workgroups
@pytest.mark.parametrize('shape,seed', [((9, 7, 5), 0), ((33, 17, 8), 1), ((5, 70, 67), 2)])
@pytest.mark.parametrize('masked', [False, True])
def test_matches_the_restatement(shape, seed, masked):
    from mudiff_hip import ops
    from mudiff_hip import volume_through_plane as TP
    rng = np.random.default_rng(seed)
    vol = rng.random(shape, dtype=np.float32)
    mask = (rng.random(shape) < 0.7).astype(np.uint8) * rng.integers(1, 255, shape).astype(np.uint8) if masked else None
    sums, z0, z1 = ops.volume_through_plane(_dev(vol), None if mask is None else _dev(mask))
    want = R.through_plane_sums(vol, mask)
    got = sums.cpu().numpy()
    assert (z0, z1) == (0, shape[0] - 1) and got.shape == want.shape
    assert np.array_equal(got[:, 0::2], want[:, 0::2])                               # the counts are exact
    assert np.abs(got[:, 1::2] - want[:, 1::2]).max() <= TOL * max(1.0, want[:, 0::2].max())
    _check(TP.measure_volume(_dev(vol), None if mask is None else _dev(mask)), R.through_plane(vol, mask))
    again, _, _ = ops.volume_through_plane(_dev(vol), None if mask is None else _dev(mask))
    assert torch.equal(again, sums)                                                  # no atomics: the same bits


def test_an_emptied_plane_gives_null_entries():
    from mudiff_hip import volume_through_plane as TP
    rng = np.random.default_rng(3)
    vol = rng.random((9, 7, 5), dtype=np.float32)
    mask = np.ones(vol.shape, np.uint8)
    mask[4] = 0
    rep = TP.measure_volume(_dev(vol), _dev(mask))
    assert rep['dz'][3] is None and rep['dz'][4] is None and None not in rep['dz'][:3] + rep['dz'][5:]
    _check(rep, R.through_plane(vol, mask))
    none = TP.measure_volume(_dev(vol), _dev(np.zeros(vol.shape, np.uint8)))
    assert all(none[k] is None for k in KEYS) and none['dz'] == [None] * 8 and none['pairs_dz'] == 0
    one = TP.measure_volume(_dev(vol), None, 2, 2)                                    # a single plane: no pair along z
    assert one['mean_dz'] is None and one['mean_dzz'] is None and one['anisotropy'] is None and one['dz'] == [] and one['mean_dx'] is not None


@pytest.mark.parametrize('z0,z1,planes', [(-5, 3, (0, 3)), (2, 99, (2, 8)), (3, 6, (3, 6)), (-1, None, (0, 8))])
def test_slab_ranges_clip(z0, z1, planes):
    from mudiff_hip import MudiffHipError, ops
    from mudiff_hip import volume_through_plane as TP
    rng = np.random.default_rng(4)
    vol = rng.random((9, 11, 6), dtype=np.float32)
    vol[:planes[0]] = np.nan                                                         # planes outside the range are never read
    vol[planes[1] + 1:] = np.nan
    mask = (rng.random(vol.shape) < 0.8).astype(np.uint8)
    rep = TP.measure_volume(_dev(vol), _dev(mask), z0, z1)
    assert rep['planes'] == list(planes)
    _check(rep, R.through_plane(vol, mask, planes[0], planes[1]))
    with pytest.raises(MudiffHipError):
        ops.volume_through_plane(_dev(vol), None, 9, 12)


def test_measure_arrays_and_the_command_line(tmp_path, capsys):
    from mudiff_hip import volume as V
    from mudiff_hip import volume_through_plane as TP
    rng = np.random.default_rng(5)
    pred = rng.random((12, 10, 9)).astype(np.float32)                                # [X, Y, Z]
    gt = (200 * rng.random(pred.shape) * (rng.random(pred.shape) < 0.8)).astype(np.float32)
    seg = (rng.random(pred.shape) < 0.5).astype(np.uint8)
    paths = {k: str(tmp_path / f'{k}.nii.gz') for k in ('pred', 'gt', 'seg')}
    for k, v in (('pred', pred), ('gt', gt), ('seg', seg.astype(np.float32))):
        V.write_nifti(paths[k], v, np.eye(4))
    zxy = lambda a: np.moveaxis(a, 2, 0)      # noqa: E731
    # half range 3 of 9 planes: the slab 1..7
    rep = TP.measure_arrays(pred, None, None, 3, DEV)
    assert rep['slab'] == [1, 7] and rep['mask'] == 'slab' and 'ground_truth' not in rep
    _check(rep['prediction'], R.through_plane(zxy(pred), None, 1, 7))
    out = tmp_path / 'tp.json'
    p = VS.run_module('mudiff_hip.volume_through_plane', ['--pred', paths['pred'], '--gt', paths['gt'], '--slice_half_range', '3', '--json', str(out)])
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith('[through-plane]')]
    assert len(lines) == 2 and lines[0].startswith('[through-plane] slab 1..7 (gt != 0): mean|dz| ') and lines[1] == f'[through-plane] wrote {out}'
    rep = json.load(open(out))
    assert rep['shape'] == [12, 10, 9] and rep['slab'] == [1, 7] and rep['mask'] == 'gt != 0'
    inside = zxy(gt != 0)
    _check(rep['prediction'], R.through_plane(zxy(pred), inside, 1, 7))
    gt01 = np.clip((V.robust_minmax_to_minus1_1(gt) + 1) / 2, 0, 1).astype(np.float32)
    want_gt = R.through_plane(zxy(gt01), inside, 1, 7)
    for k in KEYS:
        assert _close(rep['ground_truth'][k], want_gt[k], 1e-6), k               # (the GT's own fp32 normalisation: not the kernel's sums)
    assert _close(rep['dz_ratio'], rep['prediction']['mean_dz'] / rep['ground_truth']['mean_dz'], 1e-12)
    # --mask wins over GT != 0; a shape mismatch leaves with status 2 (in this process: one child is enough for the round trip)
    assert TP.main(['--pred', paths['pred'], '--gt', paths['gt'], '--mask', paths['seg'], '--slice_half_range', '3']) == 0
    assert ' (mask): ' in capsys.readouterr().out
    _check(TP.measure_files(paths['pred'], None, paths['seg'], 3, DEV)['prediction'], R.through_plane(zxy(pred), zxy(seg), 1, 7))
    V.write_nifti(str(tmp_path / 'small.nii.gz'), pred[:, :, :5], np.eye(4))
    assert TP.main(['--pred', paths['pred'], '--gt', str(tmp_path / 'small.nii.gz')]) == 2
    assert 'differ in shape' in capsys.readouterr().err
