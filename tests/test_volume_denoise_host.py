"""CPU: the host side of --denoise (mudiff_hip.volume_denoise) and its numpy restatement
(tests/volume_denoise_ref.py): what the definition passes through, the radix-select median, the flags, the place of the stage in
volume_prepare.prepare_inputs, the [done] suffix and the report file, and the recovery of a noisy slab by the restatement alone."""
import json
import os

import numpy as np
import pytest

import volume_denoise_ref as D
import volume_intake_ref as R
from volume_support import cli_argv

SHAPE = (13, 11, 9)


def _noisy(seed=5):
    return (500.0 + np.random.default_rng(seed).standard_normal(SHAPE) * 20.0).astype(np.float32)


def test_zeros_stay_zero_and_invalid_voxels_pass_through_and_stay_out_of_patches():
    v = _noisy()
    v[2:5, 3:6, 1:4] = 0.0
    v[8, 5, 4], v[10, 9, 7], v[1, 1, 7] = np.nan, np.inf, -np.inf
    for rician in (False, True):
        out = D.nlm(v, 20.0, rician=rician)
        assert out.dtype == np.float32 and out.shape == SHAPE
        special = ~np.isfinite(v) | (v == 0)
        assert np.array_equal(out[special].view(np.uint32), v[special].view(np.uint32))
        assert np.isfinite(out[~special]).all() and np.abs(out[~special] - v[~special]).max() > 1.0
        # an invalid voxel is not in anybody's patch or window: any other invalid value there gives the same bits everywhere else
        w = v.copy()
        w[8, 5, 4], w[10, 9, 7], w[1, 1, 7] = np.inf, np.nan, np.nan
        other = D.nlm(w, 20.0, rician=rician)
        assert np.array_equal(other[~special].view(np.uint32), out[~special].view(np.uint32))
    # but a zero is a valid voxel: its neighbours see it
    assert not np.array_equal(D.nlm(np.where(v == 0, np.float32(500), v), 20.0)[~special], D.nlm(v, 20.0)[~special])


@pytest.mark.parametrize('sigma', [0.01, 3.0, 1e4])
def test_a_constant_volume_and_a_single_valid_voxel_come_back_unchanged(sigma):
    const = np.full(SHAPE, 321.25, np.float32)
    lone = np.full(SHAPE, np.nan, np.float32)
    lone[6, 5, 4] = 77.5                                                               # no candidate: the centre's weight is 1
    for window in ((2, 1), (1, 1), (3, 2)):
        assert np.array_equal(D.nlm(const, sigma, *window), const)
        assert np.array_equal(D.nlm(lone, sigma, *window).view(np.uint32), lone.view(np.uint32))
    assert np.array_equal(D.nlm(lone, sigma, rician=True).view(np.uint32), np.where(np.isnan(lone), lone, np.float32(
        np.sqrt(max(77.5 ** 2 - 2.0 * sigma * sigma, 0.0)))).view(np.uint32))


@pytest.mark.parametrize('n', [1, 2, 7, 8, 1001, 4096])
def test_radix_select_is_the_lower_median(n):
    """numpy histograms standing in for the device: the key found equals np.sort(...)[(n - 1) // 2] exactly, ties included."""
    from mudiff_hip import volume_denoise as VD
    rng = np.random.default_rng(n)
    for trial in range(4):
        eps = np.abs(rng.standard_normal(n) * 10.0 ** rng.integers(-3, 4)).astype(np.float32)
        if trial % 2:
            eps = np.round(eps, 1).astype(np.float32)                                  # heavy ties
        if trial == 3:
            eps[:] = eps[0]
        keys = np.concatenate([eps.view(np.uint32), np.full(5, D.SKIP, np.uint32)])    # (skipped keys do not count)
        rng.shuffle(keys)
        key, count = VD.select_lower_median(lambda prefix, which: D.select_hist(keys, prefix, which))
        want = np.sort(eps)[(n - 1) // 2]
        assert count == n and key == int(want.view(np.uint32)) and VD.sigma_of_key(key) == 1.4826 * float(want)
    assert VD.select_lower_median(lambda prefix, which: np.zeros(256, np.int64)) == (None, 0)
    assert VD.select_lower_median(lambda prefix, which: D.select_hist(np.full(9, D.SKIP, np.uint32), prefix, which)) == (None, 0)


def test_residual_keys_cover_the_interior_positive_voxels_only():
    v = _noisy()
    v[0, 0, 0], v[6, 5, 4], v[3, 3, 3], v[9, 8, 6] = 0.0, np.nan, -4.0, 0.0
    keys = D.residual_keys(v)
    inner = np.zeros(SHAPE, bool)
    inner[1:-1, 1:-1, 1:-1] = True
    bad = ~np.isfinite(v) | ~(v > 0)
    near = bad.copy()
    for axis in range(3):
        near |= np.roll(bad, 1, axis) | np.roll(bad, -1, axis)
    assert np.array_equal(keys != D.SKIP, inner & ~near) and (keys[keys != D.SKIP] < 0x7F800000).all()
    assert D.sigma_by_sorting(v)[1] == int((inner & ~near).sum())
    assert D.sigma_by_sorting(np.zeros(SHAPE, np.float32)) == (0.0, 0) and D.sigma_by_sorting(np.ones((5, 2, 5), np.float32)) == (0.0, 0)


def test_flags_defaults_and_refusals(capsys):
    from mudiff_hip import volume as V
    from mudiff_hip import volume_denoise as VD
    from mudiff_hip.volume_prepare import IntakeOptions
    args = V.build_argparser(cli_argv())
    assert args.denoise is False and args.denoise_sigma is None and args.denoise_rician is False
    assert IntakeOptions.from_args(args).denoise is None and IntakeOptions.from_args(args) == IntakeOptions('percentile', False, None, None, 80)
    assert IntakeOptions._fields[-1] == 'denoise' and IntakeOptions().denoise is None
    assert IntakeOptions.from_args(V.build_argparser(cli_argv('--denoise'))).denoise == VD.DEFAULTS == dict(sigma=None, search=2, patch=1, beta=1.0,
                                                                                                         rician=False)
    args = V.build_argparser(cli_argv('--denoise', '--denoise_sigma', '12.5', '--denoise_search', '3', '--denoise_patch', '2', '--denoise_beta', '0.5',
                                   '--denoise_rician'))
    assert IntakeOptions.from_args(args).denoise == dict(sigma=12.5, search=3, patch=2, beta=0.5, rician=True)
    for bad, word in ((['--denoise_sigma', '0'], 'denoise_sigma'), (['--denoise_sigma', 'nan'], 'denoise_sigma'), (['--denoise_sigma', '-1'], 'denoise_sigma'),
                      (['--denoise_search', '0'], 'denoise_search'), (['--denoise_search', '6'], 'denoise_search'), (['--denoise_patch', '0'], 'denoise_patch'),
                      (['--denoise_patch', '3'], 'denoise_patch'), (['--denoise_beta', '0'], 'denoise_beta'), (['--denoise_beta', 'inf'], 'denoise_beta')):
        with pytest.raises(SystemExit):
            V.build_argparser(cli_argv('--denoise', *bad))
        assert word in capsys.readouterr().err
    with pytest.raises(ValueError, match='--denoise_search'):
        VD.check_options(search=9)
    from mudiff_hip import cohort
    assert cohort.build_argparser(cli_argv('--manifest', 'm.tsv', '--denoise', '--denoise_search', '3')).denoise_search == 3


def test_denoise_suffix_and_reports(tmp_path):
    from mudiff_hip import volume_denoise as VD
    from mudiff_hip.volume_prepare import IntakeReport
    assert VD.denoise_suffix([]) == '' and VD.denoise_suffix(None) == ''
    reports = [('FLAIR', dict(sigma=31.5, estimated=True, samples=1200, zeroed=0)), ('T2', dict(sigma=0.0, estimated=True, samples=0, zeroed=0))]
    assert VD.denoise_suffix(reports) == ' | denoise=FLAIR,T2'
    path = VD.write_reports(reports, str(tmp_path / 'o'), 'T1CE')
    assert os.path.basename(path) == 'denoise_t1ce.json' and json.load(open(path)) == dict(reports)
    report = IntakeReport()
    assert report.denoise == [] and report.suffix() == ''
    report.denoise += reports
    report.bias.append(('FLAIR', dict(iterations=[1]), None))
    assert report.suffix() == ' | bias=FLAIR | denoise=FLAIR,T2'
    report.write(str(tmp_path / 'p'), 'T1CE', np.eye(4), None)
    assert sorted(os.listdir(tmp_path / 'p')) == ['bias_t1ce.json', 'denoise_t1ce.json']


class StandIn:
    def __init__(self, stage, source):
        self.stage, self.source = stage, source
        self.shape, self.affine, self.header = source.shape, source.affine, source.header


def test_prepare_inputs_denoises_every_input_first(tmp_path, monkeypatch):
    """denoise is called for every input before coregister sees any; `ref` is the first input's geometry; the first (denoised) input is
    still the one that is never registered or resampled."""
    from mudiff_hip import volume_bias as VB, volume_coreg as VC, volume_denoise as VD, volume_intake as VI, volume_regrid as VR
    from mudiff_hip.volume_prepare import IntakeOptions, prepare_inputs
    rng = np.random.default_rng(4)
    names = ['FLAIR', 'T2', 'T1']
    raws = [VI.read_nifti_raw(R.write_nifti_typed(tmp_path / f'{m}.nii.gz', rng.integers(0, 50, (8, 8, 9)).astype(np.int16))) for m in names]
    calls = []

    def denoise(raw, device, **kw):
        calls.append(('denoise', raw, kw))
        return StandIn('denoised', raw), dict(sigma=float(len(calls)))

    def coregister(fixed, moving, device, **kw):
        calls.append(('coregister', fixed, moving))
        return np.eye(4), dict(params=[0.0] * 6, accepted=True)

    def regrid_to(raw, ref_shape, ref_affine, device, mode='linear', header=None, world=None):
        calls.append(('regrid_to', raw))
        return StandIn('regridded', raw)

    def correct(raw, device, **kw):
        calls.append(('correct', raw))
        return StandIn('corrected', raw), dict(iterations=[1])

    monkeypatch.setattr(VD, 'denoise', denoise)
    monkeypatch.setattr(VC, 'coregister', coregister)
    monkeypatch.setattr(VR, 'regrid_to', regrid_to)
    monkeypatch.setattr(VB, 'correct', correct)
    options = IntakeOptions(regrid=True, coreg=dict(strides=(4,)), bias=dict(VB.DEFAULTS, field=False), half_range=2, denoise=dict(VD.DEFAULTS))
    prepared, ref, report = prepare_inputs(list(zip(names, raws)), options, 'the device')
    assert [c[0] for c in calls] == ['denoise'] * 3 + ['correct', 'coregister', 'regrid_to', 'correct', 'coregister', 'regrid_to', 'correct']
    assert [c[1] for c in calls[:3]] == raws and all(c[2] == VD.DEFAULTS for c in calls[:3])
    assert ref[0] == raws[0].shape and ref[1] is raws[0].affine and ref[2] is raws[0].header and ref[3:] == (2, 6)
    assert calls[3][1].stage == 'denoised' and calls[3][1].source is raws[0]           # the first input: denoised, then corrected only
    for k, raw in ((4, raws[1]), (7, raws[2])):
        co, re, bi = calls[k:k + 3]
        assert co[1].source is raws[0] and co[1].stage == 'denoised' and co[2].source is raw and co[2].stage == 'denoised'
        assert re[1] is co[2] and bi[1].stage == 'regridded'
    assert [n for n, _ in report.denoise] == names and [r['sigma'] for _, r in report.denoise] == [1.0, 2.0, 3.0]
    assert report.suffix().endswith(' | bias=FLAIR,T2,T1 | denoise=FLAIR,T2,T1') and report.regridded == ['T2', 'T1']
    # the flag alone: the denoised volumes come back in order, nothing else runs
    del calls[:]
    prepared, ref, report = prepare_inputs(list(zip(names, raws)), IntakeOptions(half_range=2, denoise=dict(VD.DEFAULTS)), None)
    assert [c[0] for c in calls] == ['denoise'] * 3 and [v.source for v in prepared] == raws and report.suffix() == ' | denoise=FLAIR,T2,T1'
    # one file given for two inputs: only the first position is the reference
    del calls[:]
    monkeypatch.setattr(VD, 'denoise', lambda raw, device, **kw: (raw, dict(sigma=0.0)))      # (untouched: sigma 0)
    prepare_inputs([('FLAIR', raws[0]), ('T2', raws[0]), ('T1', raws[2])], options, None)
    assert [c[0] for c in calls] == ['correct', 'coregister', 'regrid_to', 'correct', 'coregister', 'regrid_to', 'correct']


def test_the_restatement_recovers_a_noisy_slab():
    """RMSE(denoised - clean) / RMSE(noisy - clean) on the 24 x 20 x 18 slab at the true sigma 30 and the defaults
    is RECORDED_RATIO = 0.12777 with this restatement; the estimator gives RECORDED_SIGMA = 32.237 there (the slab's one edge plane
    inflates it) and 30.379 on a flat 20^3 volume.  Bars: 1.5 x the recorded ratio, the estimate within 20 % of 30."""
    noisy, clean = D.slab()
    assert noisy.shape == D.SLAB_SHAPE == (24, 20, 18) and clean[11, 0, 0] == 400.0 and clean[12, 0, 0] == 700.0
    ratio = D.recovery_ratio(D.nlm(noisy, D.SLAB_SIGMA), noisy, clean)
    sigma, n = D.sigma_by_sorting(noisy)
    flat = (500.0 + np.random.default_rng(1).standard_normal((20, 20, 20)) * D.SLAB_SIGMA).astype(np.float32)
    flat_sigma = D.sigma_by_sorting(flat)[0]
    print('ratio', ratio, 'bar', D.BAR, 'sigma', sigma, 'samples', n, 'flat sigma', flat_sigma)
    assert ratio <= D.BAR and D.BAR == 1.5 * D.RECORDED_RATIO
    assert abs(sigma - D.SLAB_SIGMA) <= 0.2 * D.SLAB_SIGMA and abs(D.RECORDED_SIGMA - D.SLAB_SIGMA) <= 0.2 * D.SLAB_SIGMA
    assert abs(flat_sigma - D.SLAB_SIGMA) <= 0.2 * D.SLAB_SIGMA and n == 22 * 18 * 16
