"""GPU: the interval-coverage counts (csrc/volume_coverage.hip, ops.volume_interval_coverage, mudiff_hip.volume_coverage) against the
restatement in tests/volume_coverage_ref.py: exact counts, width sums within 1e-10 relative, null entries, clipped slab ranges, NaN
handling and the command line.  DESIGN.md section 5.24."""
import json

import numpy as np
import pytest
import torch

import volume_coverage_ref as R
import volume_support as VS

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
TOL = 1e-10                 # relative: fp64 sums of at most 2^13 fp64 differences of fp32 values, in another order than numpy's


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _case(shape, seed, masked, nreg=4):
    """An interval around 0.5 of varying width and a ground truth that leaves it on both sides; exact ties on both bounds."""
    rng = np.random.default_rng(seed)
    lo = (0.5 - 0.4 * rng.random(shape)).astype(np.float32)
    hi = (0.5 + 0.4 * rng.random(shape)).astype(np.float32)
    gt = rng.random(shape, dtype=np.float32)
    tie = rng.random(shape)
    gt = np.where(tie < 0.05, lo, np.where(tie > 0.95, hi, gt))
    region = rng.integers(0, 1 << nreg, shape).astype(np.uint8) if masked else None
    return lo, hi, gt, region


def _run(lo, hi, gt, region, nreg, z0=0, z1=None):
    from mudiff_hip import ops
    counts, sums, a, b = ops.volume_interval_coverage(_dev(lo), _dev(hi), _dev(gt), _dev(region), nreg, z0, z1)
    assert counts.dtype == torch.int64 and sums.dtype == torch.float64
    return counts.cpu().numpy(), sums.cpu().numpy(), a, b


def _same(got, want):
    assert got[2:] == want[2:] and got[0].shape == want[0].shape and got[1].shape == want[1].shape
    assert np.array_equal(got[0], want[0])                                           # the counts are exact
    assert np.abs(got[1] - want[1]).max() <= TOL * max(1.0, np.abs(want[1]).max())


# the sizes of tests/test_through_plane_gpu.py: less than a wave per plane, odd sizes, more voxels per plane than one pass of its workgroups
@pytest.mark.parametrize('shape,seed', [((9, 7, 5), 0), ((33, 17, 8), 1), ((5, 70, 67), 2)])
@pytest.mark.parametrize('masked', [False, True])
def test_matches_the_restatement(shape, seed, masked):
    nreg = 4 if masked else 1
    lo, hi, gt, region = _case(shape, seed, masked)
    got = _run(lo, hi, gt, region, nreg)
    _same(got, R.coverage(lo, hi, gt, region, nreg))
    c = got[0]
    assert (c[..., R.N] == c[..., R.BELOW] + c[..., R.ABOVE] + c[..., R.INSIDE]).all() and not c[..., R.NONFINITE].any()
    assert c[..., R.BELOW].sum() and c[..., R.ABOVE].sum() and (got[1][..., R.WIDTH_INSIDE] <= got[1][..., R.WIDTH]).all()
    again = _run(lo, hi, gt, region, nreg)
    assert np.array_equal(again[0], c) and np.array_equal(again[1], got[1])          # no atomics: the same bits
    if not masked:                                                                   # without a region volume every region is the slab
        two = _run(lo, hi, gt, None, 3)
        assert all(np.array_equal(two[0][:, k], c[:, 0]) and np.array_equal(two[1][:, k], got[1][:, 0]) for k in range(3))


def test_a_region_emptied_on_one_plane_reports_null():
    from mudiff_hip import ops
    from mudiff_hip import volume_coverage as VC
    lo, hi, gt, region = _case((9, 7, 5), 3, True, nreg=2)
    region |= 1
    region[4] &= 1                                                                   # region 1 has no voxel on plane 4
    counts, sums, z0, _ = ops.volume_interval_coverage(_dev(lo), _dev(hi), _dev(gt), _dev(region), 2)
    rep = VC.summarize(counts.cpu().numpy(), sums.cpu().numpy(), ('slab', 'brain'), z0, nominal=0.9)
    curve = rep['per_plane']['brain']['empirical']
    assert curve[4] is None and None not in curve[:4] + curve[5:] and None not in rep['per_plane']['slab']['empirical']
    want = R.coverage(lo, hi, gt, region, 2)[0]
    assert rep['coverage']['brain']['inside_voxels'] == int(want[:, 1, R.INSIDE].sum())
    assert rep['coverage']['brain']['empirical'] == want[:, 1, R.INSIDE].sum() / want[:, 1, R.N].sum()
    region[:] = 1                                                                    # region 1 empty everywhere
    counts, sums, z0, _ = ops.volume_interval_coverage(_dev(lo), _dev(hi), _dev(gt), _dev(region), 2)
    none = VC.summarize(counts.cpu().numpy(), sums.cpu().numpy(), ('slab', 'brain'), z0)['coverage']['brain']
    assert none['voxels'] == 0 and all(none[k] is None for k in ('empirical', 'below', 'above', 'mean_width', 'mean_width_inside', 'nominal'))


@pytest.mark.parametrize('z0,z1,planes', [(-5, 3, (0, 3)), (2, 99, (2, 8)), (3, 6, (3, 6)), (-1, None, (0, 8))])
def test_slab_ranges_clip_and_nan_outside_changes_nothing(z0, z1, planes):
    from mudiff_hip import MudiffHipError, ops
    lo, hi, gt, region = _case((9, 11, 6), 4, True)
    want = R.coverage(lo, hi, gt, region, 4, z0, z1)
    for a in (lo, hi, gt):                                                           # planes outside the range are never read
        a[:planes[0]] = np.nan
        a[planes[1] + 1:] = np.nan
    got = _run(lo, hi, gt, region, 4, z0, z1)
    assert got[2:] == planes
    _same(got, want)
    assert not got[0][..., R.NONFINITE].any()
    with pytest.raises(MudiffHipError):
        ops.volume_interval_coverage(_dev(lo), _dev(hi), _dev(gt), None, 1, 9, 12)
    with pytest.raises(MudiffHipError):
        ops.volume_interval_coverage(_dev(lo), _dev(hi), _dev(gt), _dev(region), 9)
    with pytest.raises(MudiffHipError):
        ops.volume_interval_coverage(_dev(lo), _dev(hi[:8]), _dev(gt), None, 1)


def test_nan_inside_the_slab_lands_in_nonfinite_only():
    lo, hi, gt, region = _case((9, 7, 5), 5, True, nreg=2)
    region |= 1
    clean = _run(lo, hi, gt, region, 2)
    spots = {'gt': (gt, (2, 3, 1)), 'lo': (lo, (2, 6, 4)), 'hi': (hi, (7, 0, 0))}
    state = {}
    for k, (a, at) in spots.items():
        state[k] = [int(c) for c in (gt[at] < lo[at], gt[at] > hi[at])]
        a[at] = np.nan
    got = _run(lo, hi, gt, region, 2)
    _same(got, R.coverage(lo, hi, gt, region, 2))
    diff = clean[0][:, 0] - got[0][:, 0]                                             # region 0 holds every voxel
    assert diff[:, R.NONFINITE].tolist() == [0, 0, -2, 0, 0, 0, 0, -1, 0] and diff[:, R.N].tolist() == [0, 0, 2, 0, 0, 0, 0, 1, 0]
    below, above = (sum(state[k][i] for k in spots) for i in (0, 1))
    assert diff[:, R.BELOW].sum() == below and diff[:, R.ABOVE].sum() == above and diff[:, R.INSIDE].sum() == 3 - below - above
    assert not diff[[0, 1, 3, 4, 5, 6, 8]].any()


def test_measure_arrays_and_the_command_line(tmp_path, capsys):
    """A 16 x 16 x 9 case through mudiff_hip.volume_coverage: the report against the restatement on the same normalised ground truth, and
    the stand-alone command line on files."""
    from mudiff_hip import ops
    from mudiff_hip import volume as V
    from mudiff_hip import volume_coverage as VC
    from mudiff_hip.volume_metrics import region_mask
    rng = np.random.default_rng(6)
    shape = (16, 16, 9)
    gt_raw = (rng.random(shape) * 900).astype(np.float32) * (rng.random(shape) < 0.8)
    label = (rng.random(shape) < 0.2).astype(np.uint8)
    lo, hi = (0.5 - 0.45 * rng.random(shape)).astype(np.float32), (0.5 + 0.45 * rng.random(shape)).astype(np.float32)
    rep = VC.measure_arrays(lo, hi, gt_raw, label, 3, DEV, nominal=0.9)
    assert rep['shape'] == [16, 16, 9] and rep['slab'] == [1, 7] and rep['regions'] == ['slab', 'brain', 'tumor', 'healthy'] and rep['nominal'] == 0.9
    assert rep['per_plane']['plane'] == list(range(1, 8)) and 'norm' not in rep
    pf = lambda a, dt: np.ascontiguousarray(np.moveaxis(np.asarray(a), 2, 0), dtype=dt)      # noqa: E731
    gt = ops.to_range_0_1(_dev(pf(V.normalise_volume(gt_raw, 'percentile'), np.float32))).cpu().numpy()
    m, names = region_mask(pf(gt_raw, np.float64), pf(label, np.float64))
    counts, sums, _, _ = R.coverage(pf(lo, np.float32), pf(hi, np.float32), gt, m, 4, 1, 7)
    for k, name in enumerate(names):
        c, s, b = counts[:, k].sum(0), sums[:, k].sum(0), rep['coverage'][name]
        assert (b['voxels'], b['inside_voxels'], b['below_voxels'], b['above_voxels'], b['nonfinite']) == (c[R.N], c[R.INSIDE], c[R.BELOW], c[R.ABOVE], 0)
        assert b['empirical'] == c[R.INSIDE] / c[R.N] and abs(b['mean_width'] - s[R.WIDTH] / c[R.N]) <= TOL and b['nominal'] == 0.9
        assert abs(b['mean_width_inside'] - s[R.WIDTH_INSIDE] / c[R.INSIDE]) <= TOL
        assert rep['per_plane'][name]['empirical'] == [ci[R.INSIDE] / ci[R.N] if ci[R.N] else None for ci in counts[:, k]]
    assert rep['coverage']['slab']['voxels'] == 16 * 16 * 7 and 0 < rep['coverage']['slab']['empirical'] < 1
    paths = {k: str(tmp_path / f'{k}.nii.gz') for k in ('lo', 'hi', 'gt', 'seg')}
    for k, a in (('lo', lo), ('hi', hi), ('gt', gt_raw), ('seg', label)):
        V.write_nifti(paths[k], a, np.eye(4))
    out = str(tmp_path / 'coverage.json')
    capsys.readouterr()
    assert VC.main(['--lo', paths['lo'], '--hi', paths['hi'], '--gt', paths['gt'], '--mask', paths['seg'], '--nominal', '0.9',
                    '--slice_half_range', '3', '--json', out]) == 0
    lines = capsys.readouterr().out.splitlines()
    assert [ln.split(':')[0] for ln in lines[:4]] == [f'[coverage] {n}' for n in names] and lines[4] == f'[coverage] wrote {out}'
    assert json.load(open(out)) == json.loads(json.dumps(rep))
    assert VC.main(['--lo', paths['lo'], '--hi', paths['hi'], '--gt', str(tmp_path / 'lo.nii.gz'), '--slice_half_range', '3']) == 0
    V.write_nifti(str(tmp_path / 'small.nii.gz'), lo[:8], np.eye(4))
    assert VC.main(['--lo', str(tmp_path / 'small.nii.gz'), '--hi', paths['hi'], '--gt', paths['gt']]) == 2
