"""GPU: --denoise.  The kernels of csrc/volume_denoise.hip against the numpy restatement
(tests/volume_denoise_ref.py) on a 37 x 29 x 23 volume (nothing a multiple of the 32 x 8 x 4 tile, several workgroups per axis, halos
that cross the volume's faces) and a 5 x 4 x 3 one (smaller than the search window on every axis), stored as int16 with slope / inter
and as fp32 with a NaN, an inf and a block of zeros: the keys of the pseudo-residuals, the four radix-select histograms and the
estimated sigma equal to the restatement's; the estimate within the derived bound at every voxel in both modes; the recovery of a
noisy slab; the C ABI's refusals; `predict_volume --denoise` end to end."""
import json
import os

import numpy as np
import pytest
import torch

import volume_denoise_ref as D
import volume_intake_ref as R
import volume_support as VS

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SHAPES = ((37, 29, 23), (5, 4, 3))
WINDOWS = ((2, 1), (1, 1), (3, 2))
I2_SCALE = (0.25, -3.0)


def _stored(shape, kind):
    """-> (stored volume, (slope, inter)): the phantom as int16 behind a slope and an intercept, or as fp32 with the specials."""
    p = D.phantom(shape, seed=81 + shape[0], head=shape[0] > 8)
    if kind == 'i2':
        vol = np.asfortranarray(np.rint((p - I2_SCALE[1]) / I2_SCALE[0]).astype('<i2'))
        vol[p == 0] = int(round(-I2_SCALE[1] / I2_SCALE[0]))                       # (stored 12 -> value 0 exactly)
        if shape[0] <= 8:
            vol[0, 0, 0] = int(round(-I2_SCALE[1] / I2_SCALE[0]))
        return vol, I2_SCALE
    vol = np.asfortranarray(p.astype('<f4'))
    if shape[0] > 8:
        vol[20, 14, 11], vol[9, 20, 7], vol[30, 10, 15] = np.nan, np.inf, -np.inf
        vol[14:18, 8:12, 9:13] = 0.0
        vol[12, 13, 12] = -0.0
    else:
        vol[2, 1, 1], vol[4, 3, 2], vol[0, 0, 0] = np.nan, np.inf, 0.0
    return vol, (1.0, 0.0)


CASES = [(shape, kind) for shape in SHAPES for kind in ('i2', 'f4')]


@pytest.fixture(scope='module')
def volumes():
    """{(shape, kind): (raw, fp32 values [X,Y,Z], sigma of the restatement, samples)} - computed once."""
    out = {}
    for shape, kind in CASES:
        vol, scale = _stored(shape, kind)
        values = np.asfortranarray(R.values_float32(vol, *scale))
        out[shape, kind] = (VS.raw_volume(vol, scale), values) + D.sigma_by_sorting(values)
    return out


@pytest.fixture(scope='module')
def references(volumes):
    """The restatement's estimates, computed once and shared: {(shape, kind, s, r, rician): (out, m)}."""
    ref = {}
    for (shape, kind), (_, values, sigma, _) in volumes.items():
        for s, r in WINDOWS:
            for rician, found in D.nlm_modes(values, sigma, s, r).items():
                ref[shape, kind, s, r, rician] = found
    return ref


@pytest.mark.parametrize('shape,kind', CASES)
def test_keys_histograms_and_sigma_are_the_restatement(volumes, shape, kind):
    from mudiff_hip import ops, volume_denoise as VD, volume_intake as VI
    raw, values, want_sigma, want_n = volumes[shape, kind]
    assert (values == 0).any()
    keys = ops.volume_denoise_residual(VI.upload(raw, DEV), raw.code, raw.shape, *raw.scaling)
    got = VS.to_host_xyz(keys).view(np.uint32)
    want = D.residual_keys(values)
    assert got.shape == want.shape and np.array_equal(got, want)
    assert int((want != D.SKIP).sum()) == want_n and want_n >= 2
    seen = []

    def device_hist(prefix, which):
        h = ops.volume_denoise_select_hist(keys, prefix, which).cpu().numpy().view(np.uint32)
        assert np.array_equal(h.astype(np.int64), D.select_hist(want, prefix, which))
        seen.append(int(h.sum()))
        return h

    key, n = VD.select_lower_median(device_hist)
    assert len(seen) == 4 and seen[0] == want_n == n and all(a >= b >= 1 for a, b in zip(seen, seen[1:]))
    assert VD.sigma_of_key(key) == want_sigma
    sigma, samples = VD.estimate_sigma(raw, DEV)
    print(shape, kind, 'sigma', sigma, 'samples', samples)
    assert (sigma, samples) == (want_sigma, want_n) and sigma > 0


@pytest.mark.parametrize('s,r', WINDOWS)
@pytest.mark.parametrize('shape,kind', CASES)
def test_nlm_is_the_restatement_at_every_voxel(volumes, references, shape, kind, s, r):
    """Gaussian mode: |device - restatement| <= 1e-6 (max - min of the valid voxels): the output is a convex combination of window values,
    d2 is bit-defined, expf differs from numpy's by at most 2 ulp (2.4e-7 relative), so the combination moves by at most 2 * 2.4e-7 of the
    range, plus the final fp32 rounding.  Rician mode: the same for v^2, |device^2 - restatement^2| <= 1e-6 max^2; the count of zeroed
    voxels may differ only where the restatement's m - 2 sigma^2 is within that bound of 0.  Zeros and invalid voxels: the input's bits."""
    from mudiff_hip import volume_denoise as VD
    raw, values, sigma, _ = volumes[shape, kind]
    valid = np.isfinite(values)
    special = ~valid | (values == 0)
    assert special.any() and (~special).any()
    lo, hi = float(values[valid].min()), float(values[valid].max())
    for rician in (False, True):
        want, m = references[shape, kind, s, r, rician]
        out, rep = VD.denoise(raw, DEV, sigma=sigma, search=s, patch=r, rician=rician)
        got = out.values_float32()
        assert isinstance(out, VD.DenoisedVolume) and got.shape == shape and got.dtype == np.float32 and out.shape == shape
        assert np.array_equal(got[special].view(np.uint32), values[special].view(np.uint32))
        assert np.isfinite(got[~special]).all() and np.isfinite(want[~special]).all()
        g, w = got[~special].astype(np.float64), want[~special].astype(np.float64)
        if rician:
            err, bound = np.abs(g * g - w * w).max(), 1e-6 * max(abs(lo), abs(hi)) ** 2
            near = int((np.abs(m[~special]) <= bound).sum())
            zeroed = int((w == 0).sum())
            print(shape, kind, s, r, 'rician: zeroed', rep['zeroed'], 'restatement', zeroed, 'near 0', near)
            assert abs(rep['zeroed'] - zeroed) <= near and rep['zeroed'] == int((g == 0).sum())
            if shape[0] > 8:
                assert zeroed > 0                                                  # (the background planes)
        else:
            err, bound = np.abs(g - w).max(), 1e-6 * (hi - lo)
            assert rep['zeroed'] == 0 and np.abs(g - values[~special]).max() > 100 * bound      # and something was denoised
        print(shape, kind, s, r, 'rician' if rician else 'gaussian', 'max error', err, 'bound', bound)
        assert err <= bound
        assert rep['sigma'] == sigma and rep['estimated'] is False and rep['samples'] == 0 and (rep['search'], rep['patch']) == (s, r)
        again = VD.denoise(raw, DEV, sigma=sigma, search=s, patch=r, rician=rician)[0].values_float32()
        assert np.array_equal(again.view(np.uint32), got.view(np.uint32))          # two runs: identical bits


def test_estimated_sigma_flat_input_and_geometry(volumes):
    from mudiff_hip import volume_denoise as VD
    import copy
    raw, values, sigma, n = volumes[(37, 29, 23), 'i2']
    raw = copy.copy(raw)
    raw.affine, raw.header = np.diag([2.0, 2.0, 3.0, 1.0]), 'the header'
    out, rep = VD.denoise(raw, DEV)
    assert rep == dict(sigma=sigma, estimated=True, samples=n, zeroed=0, search=2, patch=1, beta=1.0, rician=False)
    assert out.affine is raw.affine and out.header == 'the header' and out.code == 16 and not out.scaled and out.dev.shape == (23, 29, 37)
    # nothing to estimate from (no voxel with six positive neighbours) and a noise-free volume: returned untouched
    for vol in (np.zeros((9, 8, 7), np.int16, order='F'), np.full((9, 8, 7), 5, np.int16, order='F')):
        flat = VS.raw_volume(vol)
        same, rep = VD.denoise(flat, DEV)
        assert same is flat and rep['sigma'] == 0.0 and rep['estimated'] is True and rep['samples'] == (0 if not vol.any() else 7 * 6 * 5)
    # a constant volume and a single valid voxel come back unchanged for a given sigma
    const = VD.denoise(VS.raw_volume(np.full((9, 8, 7), 5, np.int16, order='F')), DEV, sigma=3.0)[0].values_float32()
    assert np.array_equal(const, np.full((9, 8, 7), 5, np.float32))
    lone = np.full((9, 8, 7), np.nan, '<f4', order='F')
    lone[4, 4, 3] = 123.5
    got = VD.denoise(VS.raw_volume(lone), DEV, sigma=3.0)[0].values_float32()
    assert np.array_equal(got.view(np.uint32), lone.view(np.uint32))


def test_device_recovery_meets_the_bar():
    """The slab's ratio on the device is within 1e-3 relative of the restatement's recorded one (volume_denoise_ref.RECORDED_RATIO, DESIGN.md
    section 5.15) and below the host test's bar of 1.5 x it."""
    from mudiff_hip import volume_denoise as VD
    noisy, clean = D.slab()
    out, rep = VD.denoise(VS.raw_volume(noisy), DEV, sigma=D.SLAB_SIGMA)
    ratio = D.recovery_ratio(out.values_float32(), noisy, clean)
    sigma = VD.estimate_sigma(VS.raw_volume(noisy), DEV)[0]
    print('device recovery', ratio, 'recorded', D.RECORDED_RATIO, 'bar', D.BAR, 'estimated sigma', sigma)
    assert abs(ratio - D.RECORDED_RATIO) <= 1e-3 * D.RECORDED_RATIO and ratio <= D.BAR
    assert abs(sigma - D.RECORDED_SIGMA) <= 1e-3 * D.RECORDED_SIGMA and abs(sigma - D.SLAB_SIGMA) <= 0.2 * D.SLAB_SIGMA


def test_c_abi_rejects_bad_arguments_without_launching():
    import mudiff_hip
    lib = mudiff_hip.load()
    X, Y, Z = 16, 8, 4
    vol = torch.full((X * Y * Z,), 7, dtype=torch.int16, device=DEV)
    keys = torch.full((X * Y * Z,), 5, dtype=torch.int32, device=DEV)
    hist = torch.full((256,), 5, dtype=torch.int32, device=DEV)
    out = torch.full((X * Y * Z,), 5.0, dtype=torch.float32, device=DEV)
    zeroed = torch.full((1,), 5, dtype=torch.int32, device=DEV)
    p = lambda t: None if t is None else t.data_ptr()      # noqa: E731

    def residual(v=vol, dt=4, dims=(X, Y, Z), k=keys):
        return lib.mud_volume_denoise_residual(p(v), dt, *dims, 1.0, 0.0, p(k), None)

    def select(k=keys, n=X * Y * Z, prefix=0, which=0, h=hist):
        return lib.mud_volume_denoise_select_hist(p(k), n, prefix, which, p(h), None)

    def nlm(v=vol, dt=4, dims=(X, Y, Z), s=2, r=1, sigma=3.0, beta=1.0, o=out, z=zeroed):
        return lib.mud_volume_denoise_nlm(p(v), dt, *dims, 1.0, 0.0, s, r, sigma, beta, 0, p(o), p(z), None)

    for kw in (dict(v=None), dict(k=None), dict(dt=64), dict(dims=(0, Y, Z)), dict(dims=(X, Y, -1))):
        assert residual(**kw) == 1, kw
    for kw in (dict(k=None), dict(h=None), dict(n=0), dict(which=-1), dict(which=4), dict(prefix=1), dict(prefix=256, which=1)):
        assert select(**kw) == 1, kw
    for kw in (dict(v=None), dict(o=None), dict(z=None), dict(dt=3), dict(dims=(X, 0, Z)), dict(s=0), dict(r=0), dict(sigma=0.0),
               dict(sigma=float('nan')), dict(sigma=float('inf')), dict(beta=0.0), dict(beta=-1.0), dict(sigma=1e-30)):
        assert nlm(**kw) == 1, kw
    assert nlm(s=6) == 1 and b'search radius 6' in lib.mud_last_error()
    assert nlm(r=3) == 1 and b'patch radius 3' in lib.mud_last_error()
    torch.cuda.synchronize()
    assert int(keys.min()) == 5 and int(hist.max()) == 5 and float(out.min()) == 5.0 and int(zeroed[0]) == 5      # nothing launched or cleared
    assert residual() == 0 and select() == 0 and nlm(s=5, r=2) == 0                # the largest halo fits; the library still works
    torch.cuda.synchronize()
    assert int(hist.sum()) == (X - 2) * (Y - 2) * (Z - 2) and float(out.min()) == 7.0 and float(out.max()) == 7.0 and int(zeroed[0]) == 0


# ---------------------------------------------------------------------------------------------------
# end to end: the tiny model of the other volume tests, three noisy inputs on one grid
# ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def runs(tmp_path_factory):
    from mudiff_hip import volume as V
    tmp = tmp_path_factory.mktemp('noisy')
    VS.write_tiny_model(tmp)
    p = {k: str(tmp / f'{k}.nii.gz') for k in ('flair', 't2', 't1')}
    for seed, k in enumerate(p):
        V.write_nifti(p[k], np.asfortranarray(D.phantom(SHAPES[0], 91 + seed).astype(np.float32)), np.eye(4))
    model = VS.model_argv(tmp, 2, 5, '--resize_back')
    inputs = ['--input_flair', p['flair'], '--input_t2', p['t2'], '--input_t1', p['t1']]
    jobs = {'den_host': ['--denoise'], 'den_dev': ['--denoise', '--device_intake'], 'den_host_z': ['--denoise', '--norm', 'zscore'],
            'den_dev_z': ['--denoise', '--norm', 'zscore', '--device_intake'], 'plain_host': [], 'plain_dev': ['--device_intake']}
    jobs = {k: model + inputs + a + ['--output_dir', str(tmp / k)] for k, a in jobs.items()}
    manifest = tmp / 'cohort.tsv'
    manifest.write_text('id\tt1\tt1ce\tt2\tflair\ns0\t' + '\t'.join([p['t1'], '', p['t2'], p['flair']]) + '\n')
    cohort = model + ['--denoise', '--manifest', str(manifest), '--output_dir', str(tmp / 'den_cohort')]
    steps = [VS.cohort_step('den_cohort', cohort)] + [VS.volume_step(k, argv) for k, argv in jobs.items()]
    log = VS.run_plan(tmp, steps, 900, ignore='RuntimeWarning')
    return dict(tmp=tmp, log=log, pred=lambda k: VS.payload(str(tmp / k / 'predicted_t1ce.nii.gz')))


def test_predict_volume_denoise_end_to_end(runs):
    tmp = runs['tmp']
    where = {k: tmp / k for k in ('den_host', 'den_dev', 'den_host_z', 'den_dev_z')}
    where['den_cohort'] = tmp / 'den_cohort' / 's0'
    reports = {}
    for name, d in where.items():
        rep = reports[name] = json.load(open(d / 'denoise_t1ce.json'))
        assert list(rep) == ['FLAIR', 'T2', 'T1']
        for r in rep.values():
            assert r['estimated'] is True and 15.0 < r['sigma'] < 60.0 and r['samples'] > 1000 and r['zeroed'] == 0      # (noise of sigma 30)
            assert (r['search'], r['patch'], r['beta'], r['rician']) == (2, 1, 1.0, False)
        assert VS.done_line(runs['log'][name]).endswith(' | denoise=FLAIR,T2,T1')
    assert all(r == reports['den_host'] for r in reports.values())
    assert runs['pred']('den_host') == runs['pred']('den_dev') == VS.payload(str(where['den_cohort'] / 'predicted_t1ce.nii.gz'))
    assert runs['pred']('den_host_z') == runs['pred']('den_dev_z')                 # host file == device file in both --norm modes
    assert runs['pred']('den_host') != runs['pred']('plain_host')                  # and the denoised inputs reached the sampler
    assert VS.done_line(runs['log']['den_host']).replace(str(where['den_host']), 'OUT') == VS.done_line(runs['log']['den_dev']).replace(str(where['den_dev']), 'OUT')


def test_without_the_flag_nothing_changes(runs):
    tmp = runs['tmp']
    assert runs['pred']('plain_dev') == runs['pred']('plain_host')
    for name in ('plain_host', 'plain_dev'):
        assert 'denoise' not in runs['log'][name] and VS.done_line(runs['log'][name]).endswith('| slices=9..13')
        assert sorted(os.listdir(tmp / name)) == ['predicted_t1ce.nii.gz']
