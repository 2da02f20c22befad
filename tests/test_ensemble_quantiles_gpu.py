"""GPU: the per-pixel quantiles of an ensemble (csrc/ensemble.hip: mud_ensemble_quantiles, ops.ensemble_quantiles,
ensemble.sample_ensemble(quantiles=), the volume pipeline's --ensemble_quantiles / --ensemble_center / --coverage) against the numpy
restatements in tests/ensemble_quantile_ref.py and tests/volume_coverage_ref.py, bit for bit.  DESIGN.md section 5.24."""
import json
import os

import numpy as np
import pytest
import torch

import ensemble_quantile_ref as R
import volume_coverage_ref as C
import volume_support as VS

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
Q8 = (0.0, 0.05, 0.25, 0.5, 0.7, 0.95, 0.999, 1.0)                         # K = 8, with q = 0, 0.5 and 1
PREMAPS = ((1.0, 0.0, -np.inf, np.inf), (0.5, 0.5, 0.0, 1.0))              # the identity and ops.to_range_0_1's


def _same(got, want):
    """np.array_equal with NaN == NaN (+-0 compare equal: the sign of a zero is not specified)."""
    return got.shape == want.shape and np.array_equal(got, want, equal_nan=True)


def _data(kind, n, N, hw, seed):
    rng = np.random.default_rng(seed)
    if kind == 'normal':                       # spills over [-1, 1]: the [0, 1] pre-map clamps a share of the samples onto a bound
        return rng.standard_normal((n, N, hw)).astype(np.float32)
    if kind == 'levels':                       # 8 levels: ties and clamped runs dominate
        return (rng.integers(0, 8, (n, N, hw)).astype(np.float32) - 3.5) / 3.0
    x = rng.standard_normal((n, 1, hw)).astype(np.float32)                  # constant pixels
    return np.repeat(x, N, axis=1)


# every NP instantiation (2, 4, 8, 16, 32, 64) at its full size and at one past the size below it
@pytest.mark.parametrize('N', [2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64])
def test_quantiles_are_the_restatement_bit_for_bit(N):
    from mudiff_hip import ops
    for hw in (4, 10, 100):                    # the vector path alone, the ragged path, and (100: 25 whole blocks) the vector path again
        for n in (1, 3):
            for kind in ('normal', 'levels', 'constant'):
                x = _data(kind, n, N, hw, 1000 * N + hw + n)
                xd = torch.from_numpy(x).to(DEV)
                for pre in PREMAPS:
                    for qs in (Q8, (0.5,)):
                        want = R.quantiles(x, qs, *pre)
                        got = ops.ensemble_quantiles(xd, qs, *pre).cpu().numpy()
                        assert _same(got, want), (N, hw, n, kind, pre, len(qs), int((got != want).sum()))
                    got8 = ops.ensemble_quantiles(xd, Q8, *pre).cpu().numpy()
                    y = R.premap(x, *pre)
                    assert np.array_equal(got8[0], y.min(1)) and np.array_equal(got8[-1], y.max(1))      # q = 0 and q = 1
                    assert (np.diff(got8, axis=0) >= 0).all()                                            # non-decreasing in q
                    if pre[2] == 0.0:
                        assert got8.min() >= 0.0 and got8.max() <= 1.0


@pytest.mark.parametrize('N', [3, 16, 33])
def test_offset_pointers_take_the_scalar_path(N):
    from mudiff_hip import ops
    n, hw = 3, 100
    x = _data('normal', n, N, hw, N)
    want = R.quantiles(x, Q8, *PREMAPS[1])
    big = torch.full((n * N * hw + 2,), 9.0, device=DEV)
    big[1:-1] = torch.from_numpy(x).to(DEV).reshape(-1)
    shifted = big[1:-1].view(n, N, hw)                                      # the samples start one float past a 16-byte boundary
    assert shifted.data_ptr() % 16 == 4
    assert _same(ops.ensemble_quantiles(shifted, Q8, *PREMAPS[1]).cpu().numpy(), want)
    out = torch.full((8 * n * hw + 2,), 7.0, device=DEV)                    # and so does the output
    ops.ensemble_quantiles(torch.from_numpy(x).to(DEV), Q8, *PREMAPS[1], out=out[1:-1])
    assert _same(out[1:-1].cpu().numpy().reshape(8, n, hw), want) and float(out[0]) == 7.0 and float(out[-1]) == 7.0
    whole = torch.full((8 * n * hw + 8,), 7.0, device=DEV)                  # the vector path writes nothing past its planes either
    ops.ensemble_quantiles(torch.from_numpy(x).to(DEV), Q8, *PREMAPS[1], out=whole[4:-4])
    assert _same(whole[4:-4].cpu().numpy().reshape(8, n, hw), want) and (whole[:4] == 7.0).all() and (whole[-4:] == 7.0).all()


@pytest.mark.parametrize('N,hw', [(2, 8), (5, 10), (16, 8), (32, 12), (64, 9)])
def test_a_nan_sample_reaches_every_quantile_of_its_pixel_only(N, hw):
    from mudiff_hip import ops
    x = _data('normal', 2, N, hw, 7 * N)
    clean = ops.ensemble_quantiles(torch.from_numpy(x).to(DEV), Q8).cpu().numpy()
    x[1, N // 2, 5] = np.nan
    for pre in PREMAPS:
        got = ops.ensemble_quantiles(torch.from_numpy(x).to(DEV), Q8, *pre).cpu().numpy()
        assert _same(got, R.quantiles(x, Q8, *pre))
        assert np.isnan(got[:, 1, 5]).all() and int(np.isnan(got).sum()) == 8
    got = ops.ensemble_quantiles(torch.from_numpy(x).to(DEV), Q8).cpu().numpy()
    keep = ~np.isnan(got)
    assert np.array_equal(got[keep], clean[keep])                           # its neighbours are untouched


def test_bad_arguments_are_refused():
    from mudiff_hip import MudiffHipError, ops
    x = torch.zeros(2, 65, 8, device=DEV)
    with pytest.raises(MudiffHipError, match=r'\[2, 64\]'):
        ops.ensemble_quantiles(x, (0.5,))
    with pytest.raises(MudiffHipError, match='1 to 8'):
        ops.ensemble_quantiles(x[:, :8].contiguous(), [0.1 * k for k in range(9)])
    for qs in ((), (1.5,), (-0.1,), (float('nan'),)):
        with pytest.raises(MudiffHipError):
            ops.ensemble_quantiles(x[:, :8].contiguous(), qs)
    with pytest.raises(MudiffHipError):
        ops.ensemble_quantiles(x[:, :1].contiguous(), (0.5,))
    with pytest.raises(MudiffHipError):
        ops.ensemble_quantiles(x[:, :8].contiguous(), (0.5,), out=torch.zeros(5, device=DEV))
    assert ops.ensemble_quantiles(x[:0, :8].contiguous(), (0.5, 0.9)).shape == (2, 0, 8)


# ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def runs(tmp_path_factory):
    """16 x 16 x 9 inputs (and 16 x 12 x 9 ones for --resize_back), the tiny model, every run in one child process."""
    from mudiff_hip import volume as V
    tmp = tmp_path_factory.mktemp('quantiles')
    VS.write_tiny_model(tmp)
    x, y, z = np.meshgrid(np.arange(16.0), np.arange(16.0), np.arange(9.0), indexing='ij')
    p = {k: str(tmp / f'{k}.nii.gz') for k in ('flair', 't2', 't1', 'gt', 'seg')}
    for i, k in enumerate(('flair', 't2', 't1', 'gt')):
        vol = (120 + 60 * np.sin(x / (3 + i) + 0.3 * z) * np.cos(y / (4 - 0.5 * i) - 0.2 * z) + 4 * z) * ((x - 8) ** 2 + (y - 8) ** 2 < 49)
        V.write_nifti(p[k], vol.astype(np.float32), np.eye(4))
    V.write_nifti(p['seg'], ((x - 6) ** 2 + (y - 9) ** 2 < 9).astype(np.float32), np.eye(4))
    small = {k: str(tmp / f'{k}_small.nii.gz') for k in ('flair', 't2', 't1')}
    for k in small:
        V.write_nifti(small[k], V.read_nifti(p[k])[0][:, 2:14].astype(np.float32), np.eye(4))
    inputs = ['--input_flair', p['flair'], '--input_t2', p['t2'], '--input_t1', p['t1']]
    ens, q3 = ['--num_samples', '4'], ['--ensemble_quantiles', '0.05', '0.5', '0.95']
    scored = ['--gt_volume', p['gt'], '--eval_mask', p['seg']]
    jobs = {'plain': ens, 'q3': ens + q3, 'q3_dev': ens + q3 + ['--device_intake'], 'q500': ens + ['--ensemble_quantiles', '0.5'],
            'median': ens + ['--ensemble_center', 'median'], 'scored': ens + scored,
            'cover': ens + scored + ['--coverage', '0.05', '0.95'],
            'resize': ens + q3 + ['--resize_back', '--input_flair', small['flair'], '--input_t2', small['t2'], '--input_t1', small['t1']]}
    steps = [VS.volume_step(k, VS.model_argv(tmp, 4, 8) + inputs + a + ['--output_dir', str(tmp / k)]) for k, a in jobs.items()]
    manifest = tmp / 'cohort.tsv'
    manifest.write_text('id\tt1\tt1ce\tt2\tflair\tgt\tmask\ns0\t' + '\t'.join([p['t1'], '', p['t2'], p['flair'], p['gt'], p['seg']]) + '\n')
    steps.append(VS.cohort_step('cohort', VS.model_argv(tmp, 4, 8) + ens + q3 + ['--score', '--coverage', '0.05', '0.95', '--manifest', str(manifest),
                                                                                 '--output_dir', str(tmp / 'cohort')]))
    log = VS.run_plan(tmp, steps, 900, ignore='RuntimeWarning')
    return dict(tmp=tmp, log=log, gz=lambda k, name: VS.payload(str(tmp / k / name)))


def _volume(path):
    from mudiff_hip import volume as V
    return V.read_nifti(str(path))


NAMES = ('predicted_t1ce_q050.nii.gz', 'predicted_t1ce_q500.nii.gz', 'predicted_t1ce_q950.nii.gz')


def test_quantile_maps_end_to_end(runs):
    tmp, log, gz = runs['tmp'], runs['log'], runs['gz']
    mean, aff, _ = _volume(tmp / 'q3' / 'predicted_t1ce.nii.gz')
    maps = [_volume(tmp / 'q3' / name) for name in NAMES]
    for vol, a, _ in maps:
        assert vol.shape == mean.shape == (16, 16, 9) and np.array_equal(a, aff)
        assert vol.min() >= 0.0 and vol.max() <= 1.0
    lo, med, hi = (m[0] for m in maps)
    assert (lo <= med).all() and (med <= hi).all() and (lo < hi).any()
    # the mean and the std are those of the run without the flag, byte for byte; so is its [done] line up to the new tail
    for name in ('predicted_t1ce.nii.gz', 'predicted_t1ce_std.nii.gz'):
        assert gz('q3', name) == gz('plain', name)
    assert sorted(os.listdir(tmp / 'plain')) == ['predicted_t1ce.nii.gz', 'predicted_t1ce_std.nii.gz']
    assert sorted(os.listdir(tmp / 'q3')) == sorted(NAMES + ('predicted_t1ce.nii.gz', 'predicted_t1ce_std.nii.gz'))
    done = VS.done_line(log['q3'])
    assert done.endswith(' | 4 samples per slice | quantiles=0.05,0.5,0.95')
    assert VS.done_line(log['plain']).replace(str(tmp / 'plain'), str(tmp / 'q3')) + ' | quantiles=0.05,0.5,0.95' == done
    # host intake, device intake and a one-subject cohort write the same quantile bytes
    for name in NAMES:
        assert gz('q3', name) == gz('q3_dev', name) == VS.payload(str(tmp / 'cohort' / 's0' / name))


def test_the_median_as_the_centre(runs):
    tmp, log, gz = runs['tmp'], runs['log'], runs['gz']
    assert gz('median', 'predicted_t1ce.nii.gz') == gz('q500', 'predicted_t1ce_q500.nii.gz') == gz('q3', NAMES[1])
    assert gz('median', 'predicted_t1ce_std.nii.gz') == gz('plain', 'predicted_t1ce_std.nii.gz')          # the std about the mean
    assert gz('median', 'predicted_t1ce.nii.gz') != gz('plain', 'predicted_t1ce.nii.gz')
    assert sorted(os.listdir(tmp / 'median')) == ['predicted_t1ce.nii.gz', 'predicted_t1ce_std.nii.gz']   # computed, not written
    assert VS.done_line(log['median']).endswith(' | 4 samples per slice | center=median')
    assert VS.done_line(log['q500']).endswith(' | quantiles=0.5')


def test_the_ordering_survives_resize_back(runs):
    tmp = runs['tmp']
    lo, med, hi = (_volume(tmp / 'resize' / name)[0] for name in NAMES)
    assert lo.shape == (16, 12, 9) and (lo <= med).all() and (med <= hi).all() and lo.min() >= 0.0 and hi.max() <= 1.0 and (lo < hi).any()


def test_coverage_end_to_end(runs):
    from mudiff_hip import ops
    from mudiff_hip import volume as V
    from mudiff_hip.volume_metrics import region_mask
    tmp, log, gz = runs['tmp'], runs['log'], runs['gz']
    assert open(tmp / 'cover' / 'metrics_t1ce.json', 'rb').read() == open(tmp / 'scored' / 'metrics_t1ce.json', 'rb').read()
    assert not os.path.exists(tmp / 'scored' / 'coverage_t1ce.json') and not os.path.exists(tmp / 'q3' / 'coverage_t1ce.json')
    for name in (NAMES[0], NAMES[2]):                                       # the two fractions joined the written set
        assert gz('cover', name) == gz('q3', name)
    assert not os.path.exists(tmp / 'cover' / NAMES[1])
    assert VS.done_line(log['cover']).endswith(' | quantiles=0.05,0.95')
    rep = json.load(open(tmp / 'cover' / 'coverage_t1ce.json'))
    assert rep['regions'] == ['slab', 'brain', 'tumor', 'healthy'] and rep['slab'] == [0, 8] and rep['quantiles'] == [0.05, 0.95]
    assert abs(rep['nominal'] - 0.9) < 1e-12
    lines = [ln for ln in log['cover'].splitlines() if ln.startswith('[coverage]')]
    assert [ln.split(':')[0] for ln in lines[:4]] == [f'[coverage] {n}' for n in rep['regions']] and lines[4].startswith('[coverage] wrote ')
    assert log['cover'].index('[metrics] wrote') < log['cover'].index('[coverage] slab')               # after the scores
    # the counts are the restatement's on the written files
    pf = lambda a, dt: np.ascontiguousarray(np.moveaxis(np.asarray(a), 2, 0), dtype=dt)      # noqa: E731
    lo, hi = (_volume(tmp / 'cover' / name)[0] for name in (NAMES[0], NAMES[2]))
    gt_raw, seg = V.read_nifti(str(tmp / 'gt.nii.gz'))[0], V.read_nifti(str(tmp / 'seg.nii.gz'))[0]
    gt = ops.to_range_0_1(torch.from_numpy(pf(V.normalise_volume(gt_raw, 'percentile'), np.float32)).to(DEV)).cpu().numpy()
    m, names = region_mask(pf(gt_raw, np.float64), pf(seg, np.float64))
    counts, sums, _, _ = C.coverage(pf(lo, np.float32), pf(hi, np.float32), gt, m, 4)
    for k, name in enumerate(names):
        c, b = counts[:, k].sum(0), rep['coverage'][name]
        assert (b['voxels'], b['inside_voxels'], b['below_voxels'], b['above_voxels'], b['nonfinite']) == (c[C.N], c[C.INSIDE], c[C.BELOW], c[C.ABOVE], 0)
        assert b['empirical'] == c[C.INSIDE] / c[C.N] and abs(b['mean_width'] - sums[:, k, C.WIDTH].sum() / c[C.N]) <= 1e-10
    assert rep['coverage']['slab']['voxels'] == 16 * 16 * 9 and 0 < rep['coverage']['tumor']['voxels'] < rep['coverage']['brain']['voxels']
    # the cohort: the subject's files, and the block of the cohort's report
    assert json.load(open(tmp / 'cohort' / 's0' / 'coverage_t1ce.json')) == rep
    cohort = json.load(open(tmp / 'cohort' / 'cohort_t1ce.json'))
    assert cohort['subjects'][0]['coverage']['slab'] == dict(empirical=rep['coverage']['slab']['empirical'], mean_width=rep['coverage']['slab']['mean_width'])
    assert cohort['coverage']['slab']['empirical'] == dict(mean=rep['coverage']['slab']['empirical'], std=0.0, count=1)


def test_sample_ensemble_returns_the_quantiles_of_its_samples():
    """sample_ensemble(return_samples=True, quantiles=...) on the tiny model, in chunks of 2 slices: the maps are the restatement's on the
    returned samples, and the other results are what the call without quantiles returns."""
    from oracle import mudiff_oracle as O
    from backbones.ncsnpp_generator_adagn_feat import NCSNpp, NCSNpp_adaptive
    from mudiff_hip import ensemble as E
    cfg = O.default_config(**VS.TINY_MODEL)
    g1, g2 = NCSNpp(cfg), NCSNpp_adaptive(cfg)
    g1.load_state_dict(O.make_state_dict(cfg, 'g1', 9))
    g2.load_state_dict(O.make_state_dict(cfg, 'g2', 9))
    g1, g2 = g1.to(DEV).eval(), g2.to(DEV).eval()
    size = cfg.image_size
    g = torch.Generator().manual_seed(4)
    conds = [torch.tanh(torch.randn(3, 1, size, size, generator=g)).to(DEV) for _ in range(3)]
    qs = (0.05, 0.5, 0.95)
    mean, std, every, maps = E.sample_ensemble(cfg, g1, g2, conds, 5, 31, batch_size=4, chunk=2, map_0_1=True, return_samples=True, quantiles=qs)
    assert maps.shape == (3, 3, size, size) and every.shape == (3, 5, size, size)
    assert _same(maps.cpu().numpy(), R.quantiles(every.cpu().numpy(), qs, 0.5, 0.5, 0.0, 1.0))
    assert (maps[0] <= maps[1]).all() and (maps[1] <= maps[2]).all() and float(maps.min()) >= 0.0 and float(maps.max()) <= 1.0
    from mudiff_hip import ops
    m2, s2 = ops.ensemble_stats(every, 0.5, 0.5, 0.0, 1.0)
    assert torch.equal(m2, mean) and torch.equal(s2, std)
    with pytest.raises(ValueError, match='64'):
        E.sample_ensemble(cfg, g1, g2, conds, 65, 31, quantiles=qs)
