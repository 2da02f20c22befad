"""GPU: --bias_correct.  The kernels of csrc/volume_bias.hip against the fp64 numpy restatement
(tests/volume_bias_ref.py) on a 37 x 29 x 23 volume (nothing a multiple of 64, x crosses a wave, several workgroups), shrink 1 / 2 / 3,
1 to 3 levels: the log image within 2 ulp, the corrected log image, its extremes, its largest change, its histogram and the integer sums
of the fit equal to the restatement's; the applied correction within 1 ulp; the whole loop equal to the restatement driven from the
device's log image; the recovery of a known field; the C ABI's argument checks; `predict_volume --bias_correct` end to end."""
import json
import os

import numpy as np
import pytest
import torch

import volume_bias_ref as B
import volume_intake_ref as R
import volume_support as VS

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SHAPE = (37, 29, 23)
SHRINKS, LEVELS = (1, 2, 3), (1, 2, 3)


def _engine(vol, shrink, scale=(1.0, 0.0)):
    from mudiff_hip import volume_bias as VB
    from mudiff_hip import volume_intake as VI
    raw = VS.raw_volume(vol, scale)
    return VB.DeviceEngine(VI.upload(raw, DEV), (raw.code, raw.shape) + ((raw.slope, raw.inter) if raw.scaled else (1.0, 0.0)), shrink)


def _lattices(levels, seed, amp=0.2):
    rng = np.random.default_rng(seed)
    return [rng.standard_normal(((1 << l) + 3,) * 3) * amp for l in range(levels)]


@pytest.fixture(scope='module')
def tissue():
    """Positive int16 intensities inside an ellipsoid, zero outside (volume_intake_ref's 'ties')."""
    return R.synthetic(SHAPE, 'ties', 'i2', seed=71)


@pytest.mark.parametrize('dtype,scale', [('u1', (1.0, 0.0)), ('i2', (1.0, 0.0)), ('u2', (1.0, 0.0)), ('i4', (1.0, 0.0)), ('f4', (1.0, 0.0)),
                                         ('i2', (0.0123, -5.5))])
def test_log_image(dtype, scale):
    """|dev - np.log(float32)| <= 2 ulp (one each for the device's logf and numpy's); NaN exactly where the mask is false."""
    vol = R.synthetic(SHAPE, 'noise', dtype, seed=72).copy(order='F')
    if dtype == 'f4':
        vol[3, 4, 5], vol[6, 4, 5], vol[9, 4, 5], vol[12, 4, 6] = np.nan, np.inf, -np.inf, 1e-42      # (a subnormal is > 0)
    values = R.values_float32(vol, *scale)
    for shrink in SHRINKS:
        want = B.log_image(values, shrink)
        got = VS.to_host_xyz(_engine(vol, shrink, scale).u)
        assert got.shape == want.shape and got.dtype == np.float32
        assert np.array_equal(np.isnan(got), np.isnan(want))
        ok = ~np.isnan(want)
        assert 0 < ok.sum() < ok.size
        ulps = np.abs(got[ok].astype(np.float64) - want[ok].astype(np.float64)) / np.spacing(np.abs(want[ok])).astype(np.float64)
        print(dtype, scale, shrink, 'masked in', int(ok.sum()), 'of', ok.size, 'max ulp', ulps.max())
        assert ulps.max() <= 2.0


@pytest.mark.parametrize('shrink', SHRINKS)
def test_corrected_histogram_and_fit_are_the_restatement(tissue, shrink):
    from mudiff_hip import volume_bias as VB
    for levels in LEVELS:
        eng = _engine(tissue, shrink)
        u = VS.to_host_xyz(eng.u)
        lat = _lattices(levels, 100 + levels)
        lo, hi, dmax = eng.corrected(lat)
        c, wlo, whi, wdmax = B.corrected(u, lat, SHAPE, shrink)
        got_c = VS.to_host_xyz(eng.c[0])
        assert np.array_equal(got_c, c, equal_nan=True) and np.isfinite(c).sum() > 100
        assert (lo, hi, dmax) == (wlo, whi, wdmax) and dmax > 0
        # a second pass against the first: dmax is measured from the previous corrected image
        lat2 = _lattices(levels, 200 + levels, amp=0.05)
        lo2, hi2, dmax2 = eng.corrected(lat2)
        c2, wlo2, whi2, wdmax2 = B.corrected(u, lat2, SHAPE, shrink, c)
        assert np.array_equal(VS.to_host_xyz(eng.c[0]), c2, equal_nan=True) and (lo2, hi2, dmax2) == (wlo2, whi2, wdmax2)
        for bins in (200, 64):
            scale = bins / (hi2 - lo2)
            h = eng.hist(lo2, scale, bins)
            assert h.dtype == np.int64 and np.array_equal(h, B.hist(c2, lo2, scale, bins)) and h.sum() == np.isfinite(c2).sum()
        scale = 200 / (hi2 - lo2)
        table = VB.sharpen(B.hist(c2, lo2, scale, 200), lo2, hi2)
        level = levels - 1
        for k in (20, VB.choose_k(eng.n_samples, lo2, hi2)):
            delta, omega = eng.fit(level, table, lo2, scale, k)
            wd, wo = B.fit(c2, table, lo2, scale, level, SHAPE, shrink, k)
            assert delta.dtype == np.int64 and delta.shape == wd.shape
            assert np.array_equal(delta, wd) and np.array_equal(omega, wo) and np.count_nonzero(wd) > 8 and (wo >= 0).all()
            again = eng.fit(level, table, lo2, scale, k)                       # determinism: integer sums, any order of arrival
            assert np.array_equal(again[0], delta) and np.array_equal(again[1], omega)


def test_corner_cases():
    from mudiff_hip import volume_bias as VB
    # nothing masked in: NaN everywhere, no extremes, zero sums, no fault
    eng = _engine(np.zeros(SHAPE, np.int16, order='F'), 2)
    assert np.isnan(VS.to_host_xyz(eng.u)).all()
    assert eng.corrected(_lattices(2, 5)) == (None, None, 0.0) and np.isnan(VS.to_host_xyz(eng.c[0])).all()
    assert not eng.hist(0.0, 0.0, 200).any()
    delta, omega = eng.fit(1, VB.bin_centres(0.0, 0.0, 200), 0.0, 0.0, 30)
    assert delta.shape == (5, 5, 5) and not delta.any() and not omega.any()
    lattices, iterations, dmax = VB.loop(eng, levels=2, iters=3)
    assert iterations == [0, 0] and dmax == 0.0 and not any(L.any() for L in lattices)
    # one plane
    vol = R.synthetic((37, 29, 1), 'ties', 'i2', seed=73)
    vol[vol == 0] = 7
    for shrink in (1, 2):
        eng = _engine(vol, shrink)
        lat = _lattices(3, 6)
        lo, hi, dmax = eng.corrected(lat)
        c, wlo, whi, wdmax = B.corrected(VS.to_host_xyz(eng.u), lat, vol.shape, shrink)
        assert np.array_equal(VS.to_host_xyz(eng.c[0]), c) and (lo, hi, dmax) == (wlo, whi, wdmax)
        scale = 200 / (hi - lo)
        table = VB.sharpen(eng.hist(lo, scale, 200), lo, hi)
        delta, omega = eng.fit(2, table, lo, scale, 40)
        wd, wo = B.fit(c, table, lo, scale, 2, vol.shape, shrink, 40)
        assert np.array_equal(delta, wd) and np.array_equal(omega, wo) and wd.any()


@pytest.mark.parametrize('dtype,scale', [('i2', (1.0, 0.0)), ('f4', (1.0, 0.0)), ('u1', (0.5, -1.0))])
def test_apply(dtype, scale):
    """|dev - ref| <= 1 ulp of fp32: the device's fp64 exp is within 1 ulp of fp64 before the single rounding to fp32.  Zeros stay zero, a
    non-finite voxel is unchanged, and with every lattice at 0 the output is the stored value bit for bit."""
    vol = R.synthetic(SHAPE, 'noise', dtype, seed=74).copy(order='F')
    if dtype == 'f4':
        vol[3, 4, 5], vol[6, 4, 5], vol[9, 4, 5], vol[1, 1, 1] = np.nan, np.inf, -np.inf, -0.0
    values = np.asfortranarray(R.values_float32(vol, *scale))
    for levels in LEVELS:
        eng = _engine(vol, 2, scale)
        lat = _lattices(levels, 300 + levels, amp=0.3)
        got = eng.apply(lat).cpu().numpy().transpose(2, 1, 0)
        want = B.apply(values, lat)
        assert got.dtype == np.float32 and got.shape == SHAPE
        special = ~np.isfinite(values) | (values == 0)
        assert special.any() and np.array_equal(got[special].view(np.uint32), values[special].view(np.uint32))
        ok = ~special
        ulps = np.abs(got[ok].astype(np.float64) - want[ok].astype(np.float64)) / np.spacing(np.abs(want[ok])).astype(np.float64)
        print(dtype, levels, 'max ulp', ulps.max(), 'voxels', int(ok.sum()))
        assert ulps.max() <= 1.0 and np.abs(got[ok] / values[ok] - 1).max() > 0.05
        field = eng.apply(lat, field=True).cpu().numpy().transpose(2, 1, 0)
        wf = np.exp(B.field(lat, SHAPE, 1)).astype(np.float32)
        assert (np.abs(field.astype(np.float64) - wf) <= np.spacing(wf)).all()
        same = eng.apply([np.zeros_like(L) for L in lat]).cpu().numpy().transpose(2, 1, 0)
        assert np.array_equal(same.view(np.uint32), values.view(np.uint32))


# ---------------------------------------------------------------------------------------------------
# the whole loop and the recovery of a known field
# ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def head():
    vol, true_field, mask = B.shaded_head()
    return dict(vol=vol, field=true_field, mask=mask)


def test_whole_loop_equals_the_restatement_driven_from_the_device_log_image(head):
    from mudiff_hip import volume_bias as VB
    eng = _engine(head['vol'], 2)
    opts = dict(levels=3, iters=8, tol=1e-3, bins=200, fwhm=0.15, wiener=0.01)
    lattices, iterations, dmax = VB.loop(eng, **opts)
    want, want_iterations, want_dmax = VB.loop(B.Engine(VS.to_host_xyz(eng.u), B.HEAD_SHAPE, 2), **opts)
    print('iterations', iterations, want_iterations, 'dmax', dmax, want_dmax)
    assert iterations == want_iterations and dmax == want_dmax and sum(iterations) >= 3
    for a, b in zip(lattices, want):
        assert np.array_equal(a, b) and a.any()
    again, it2, d2 = VB.loop(_engine(head['vol'], 2), **opts)                      # two runs: identical bits
    assert it2 == iterations and d2 == dmax and all(np.array_equal(a, b) for a, b in zip(again, lattices))


def test_device_recovery_meets_the_bar(head):
    """The bar is 1.5 x the ratio the restatement alone reaches (volume_bias_ref.RECORDED_RATIO)."""
    from mudiff_hip import volume_bias as VB
    from mudiff_hip import volume_regrid as VR
    out, rep = VB.correct(VS.raw_volume(head['vol']), DEV, **B.RECOVERY, field=True)
    ratio = B.recovery_ratio(out.lattices, head['field'], head['mask'])
    print('device recovery', ratio, 'bar', B.BAR, rep)
    assert ratio < 0.5 and ratio <= B.BAR
    assert isinstance(out, VR.RegriddedVolume) and out.code == 16 and out.shape == B.HEAD_SHAPE and not out.scaled
    assert len(rep['iterations']) == 4 and rep['masked'] == int((head['vol'][::2, ::2, ::2] > 0).sum()) and rep['samples'] == 22 * 20 * 18
    assert rep['field_min'] < rep['field_mean'] < rep['field_max']
    got = out.values_float32()
    want = B.apply(head['vol'], out.lattices)
    assert np.array_equal(got == 0, head['vol'] == 0)
    assert (np.abs(got.astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.abs(want))).all()
    assert out.field.shape == B.HEAD_SHAPE and np.abs(np.log(out.field) - B.field(out.lattices, B.HEAD_SHAPE, 1)).max() <= 1e-6


def test_c_abi_rejects_bad_arguments_without_launching():
    import mudiff_hip
    lib = mudiff_hip.load()
    X, Y, Z = 16, 8, 4
    vol = torch.ones(X * Y * Z, dtype=torch.int16, device=DEV)
    u = torch.full((X * Y * Z,), 5.0, dtype=torch.float32, device=DEV)
    c0, c1 = u.clone(), u.clone()
    lat = torch.zeros(64 + 125, dtype=torch.float64, device=DEV)
    stats = torch.full((3,), 5, dtype=torch.int64, device=DEV)
    hist = torch.full((200,), 5, dtype=torch.int32, device=DEV)
    table = torch.zeros(200, dtype=torch.float64, device=DEV)
    sums = torch.full((2 * 125,), 5, dtype=torch.int64, device=DEV)
    out = torch.full((X * Y * Z,), 5.0, dtype=torch.float32, device=DEV)
    p = lambda t: None if t is None else t.data_ptr()      # noqa: E731
    nan, inf = float('nan'), float('inf')

    def log(v=vol, dt=4, dims=(X, Y, Z), shrink=1, o=u):
        return lib.mud_volume_bias_log(p(v), dt, *dims, 1.0, 0.0, shrink, p(o), None)

    def corrected(a=u, b=c0, c=c1, l=lat, levels=2, dims=(X, Y, Z), shrink=1, s=stats):
        return lib.mud_volume_bias_corrected(p(a), p(b), p(c), p(l), levels, *dims, shrink, p(s), None)

    def histogram(c=c0, n=X * Y * Z, lo=0.0, scale=1.0, bins=200, h=hist):
        return lib.mud_volume_bias_hist(p(c), n, lo, scale, bins, p(h), None)

    def fit(c=c0, t=table, bins=200, lo=0.0, scale=1.0, level=1, dims=(X, Y, Z), shrink=1, k=30, s=sums):
        return lib.mud_volume_bias_fit(p(c), p(t), bins, lo, scale, level, *dims, shrink, k, p(s), None)

    def apply(v=vol, dt=4, dims=(X, Y, Z), l=lat, levels=2, o=out):
        return lib.mud_volume_bias_apply(p(v), dt, *dims, 1.0, 0.0, p(l), levels, 0, p(o), None)

    assert log(v=None) == 1 and b'null' in lib.mud_last_error()
    assert log(o=None) == 1 and log(dims=(0, Y, Z)) == 1 and log(dims=(X, Y, -1)) == 1
    assert log(shrink=0) == 1 and b'shrink' in lib.mud_last_error()
    assert log(dt=64) == 1 and b'datatype' in lib.mud_last_error()
    for kw in (dict(a=None), dict(b=None), dict(c=None), dict(l=None), dict(s=None), dict(dims=(X, 0, Z)), dict(shrink=-1), dict(levels=0),
               dict(levels=6), dict(c=c0), dict(c=u)):
        assert corrected(**kw) == 1, kw
    for kw in (dict(c=None), dict(h=None), dict(n=0), dict(n=-3), dict(bins=1), dict(bins=1025), dict(lo=nan), dict(scale=inf)):
        assert histogram(**kw) == 1, kw
    for kw in (dict(c=None), dict(t=None), dict(s=None), dict(bins=1), dict(bins=1025), dict(lo=inf), dict(scale=nan), dict(level=-1),
               dict(dims=(X, Y, 0)), dict(shrink=0), dict(k=-1), dict(k=63)):
        assert fit(**kw) == 1, kw
    assert fit(level=5) == 1 and b'LDS' in lib.mud_last_error()                    # 32 spans per axis: refused
    for kw in (dict(v=None), dict(l=None), dict(o=None), dict(dt=3), dict(dims=(X, Y, 0)), dict(levels=0), dict(levels=6)):
        assert apply(**kw) == 1, kw
    torch.cuda.synchronize()
    for t in (stats, hist, sums):
        assert int(t.min()) == 5 and int(t.max()) == 5                             # nothing was launched, nothing cleared
    assert float(out.min()) == 5.0 and float(c1.max()) == 5.0
    assert log() == 0 and corrected() == 0 and histogram() == 0 and fit() == 0 and apply() == 0      # the library still works afterwards
    torch.cuda.synchronize()
    assert float(u.abs().max()) == 0.0 and float(c1.abs().max()) == 0.0 and int(hist.sum()) == X * Y * Z and float(out.min()) == 1.0
    assert int(sums[:125].sum()) > 0 and int(sums[125:].sum()) > 0                 # r = 5 - table = 5 at every sample


# ---------------------------------------------------------------------------------------------------
# end to end: the tiny model of the other volume tests, three shaded inputs on one grid
# ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def runs(tmp_path_factory, head):
    from mudiff_hip import volume as V
    tmp = tmp_path_factory.mktemp('shaded')
    VS.write_tiny_model(tmp)
    p = {k: str(tmp / f'{k}.nii.gz') for k in ('flair', 't2', 't1')}
    V.write_nifti(p['flair'], head['vol'], np.eye(4))
    t2 = B.shaded_head(noise_seed=22)[0][::-1].copy(order='F') * np.float32(0.5)
    V.write_nifti(p['t2'], t2, np.eye(4))
    shifted = np.eye(4)
    shifted[:3, 3] = (1.5, -1.0, 0.5)
    p['t2_grid'] = str(tmp / 't2_grid.nii.gz')                                     # the same head on another grid: moved, one plane fewer
    V.write_nifti(p['t2_grid'], t2[:, :, :-1].copy(order='F'), shifted)
    V.write_nifti(p['t1'], B.shaded_head(noise_seed=23)[0][:, ::-1].copy(order='F') * np.float32(2.0), np.eye(4))
    model = VS.model_argv(tmp, 2, 5, '--resize_back', '--input_flair', p['flair'], '--input_t2', p['t2'], '--input_t1', p['t1'])
    bias = ['--bias_correct', '--bias_shrink', '2', '--bias_levels', '3']
    jobs = {'bias_host': bias, 'bias_dev': bias + ['--device_intake', '--bias_field_out'], 'bias_host_z': bias + ['--norm', 'zscore'],
            'bias_dev_z': bias + ['--norm', 'zscore', '--device_intake'], 'bias_coreg': bias + ['--coregister', '--coregister_strides', '4'],
            'plain_host': [], 'plain_dev': ['--device_intake'], 'plain_host_z': ['--norm', 'zscore']}
    jobs = {k: model + a + ['--output_dir', str(tmp / k)] for k, a in jobs.items()}
    every = ['--regrid', '--coregister', '--coregister_strides', '4'] + bias       # the three flags together, T2 on its own grid
    on_grid = model[:model.index('--input_flair')]
    jobs.update({k: on_grid + ['--input_flair', p['flair'], '--input_t2', p['t2_grid'], '--input_t1', p['t1']] + every + a +
                 ['--output_dir', str(tmp / k)] for k, a in (('all_host', []), ('all_dev', ['--device_intake']))})
    manifest = tmp / 'cohort.tsv'
    manifest.write_text('id\tt1\tt1ce\tt2\tflair\ns0\t' + '\t'.join([p['t1'], '', p['t2_grid'], p['flair']]) + '\n')
    cohort = on_grid + every + ['--manifest', str(manifest), '--output_dir', str(tmp / 'all_cohort')]
    steps = [VS.cohort_step('all_cohort', cohort)] + [VS.volume_step(k, argv) for k, argv in jobs.items()]
    log = VS.run_plan(tmp, steps, 900, ignore='RuntimeWarning')
    return dict(tmp=tmp, log=log, pred=lambda k: VS.payload(str(tmp / k / 'predicted_t1ce.nii.gz')))


def test_predict_volume_bias_correct_end_to_end(runs):
    tmp = runs['tmp']
    reports = {}
    for name in ('bias_host', 'bias_dev', 'bias_host_z', 'bias_dev_z', 'bias_coreg'):
        rep = reports[name] = json.load(open(tmp / name / 'bias_t1ce.json'))
        assert list(rep) == ['FLAIR', 'T2', 'T1']
        for r in rep.values():
            assert len(r['iterations']) == 3 and all(1 <= i <= 50 for i in r['iterations']) and r['shrink'] == 2
            assert r['field_min'] < r['field_mean'] < r['field_max'] and r['field_max'] - r['field_min'] > 0.2      # (the shading is +-0.3)
        assert VS.done_line(runs['log'][name]).endswith(' | bias=FLAIR,T2,T1')
    assert reports['bias_host'] == reports['bias_dev'] == reports['bias_host_z'] == reports['bias_dev_z']
    assert runs['pred']('bias_host') == runs['pred']('bias_dev')                   # host file == device file, byte for byte
    assert runs['pred']('bias_host_z') == runs['pred']('bias_dev_z')               # in both --norm modes
    assert runs['pred']('bias_host') != runs['pred']('plain_host')                 # and the correction reached the sampler
    assert runs['pred']('bias_host_z') != runs['pred']('plain_host_z')
    assert ' | coreg=T2:' in VS.done_line(runs['log']['bias_coreg']) and os.path.exists(tmp / 'bias_coreg' / 'coreg_t1ce.json')
    fields = sorted(f for f in os.listdir(tmp / 'bias_dev') if f.startswith('bias_field_'))
    assert fields == ['bias_field_flair_t1ce.nii.gz', 'bias_field_t1_t1ce.nii.gz', 'bias_field_t2_t1ce.nii.gz']
    from mudiff_hip import volume as V
    f = V.read_nifti(str(tmp / 'bias_dev' / fields[0]))[0]
    assert f.shape == B.HEAD_SHAPE and np.isfinite(f).all() and f.min() > 0 and f.max() / f.min() > 1.2      # (the shading spans exp(0.6))
    assert not any(f.startswith('bias_field_') for f in os.listdir(tmp / 'bias_host'))


def test_the_three_flags_together_agree_on_every_entry_point(runs):
    """--regrid --coregister --bias_correct with T2 on another grid: the host path, --device_intake and a one-subject cohort write the
    same prediction and the same reports and print the same [done] line."""
    import re
    tmp = runs['tmp']
    where = {'all_host': tmp / 'all_host', 'all_dev': tmp / 'all_dev', 'all_cohort': tmp / 'all_cohort' / 's0'}
    payloads = {k: VS.payload(str(d / 'predicted_t1ce.nii.gz')) for k, d in where.items()}
    assert payloads['all_host'] == payloads['all_dev'] == payloads['all_cohort']
    assert payloads['all_host'] != runs['pred']('bias_coreg')                      # (T2 really came from the other grid)
    for report, keys in (('coreg_t1ce.json', ['T2', 'T1']), ('bias_t1ce.json', ['FLAIR', 'T2', 'T1'])):
        reps = [json.load(open(d / report)) for d in where.values()]
        assert reps[0] == reps[1] == reps[2] and list(reps[0]) == keys
    lines = {k: VS.done_line(runs['log'][k]).replace(str(d), 'OUT') for k, d in where.items()}
    print(lines['all_host'])
    assert lines['all_host'] == lines['all_dev'] == lines['all_cohort']
    assert re.search(r' \| regrid=T2[^|]* \| coreg=[^|]+ \| bias=FLAIR,T2,T1$', lines['all_host'])


def test_without_the_flag_nothing_changes(runs):
    tmp = runs['tmp']
    assert runs['pred']('plain_dev') == runs['pred']('plain_host')
    for name in ('plain_host', 'plain_dev', 'plain_host_z'):
        assert ' | bias=' not in VS.done_line(runs['log'][name]) and ' | regrid=' not in VS.done_line(runs['log'][name]) and 'bias' not in runs['log'][name]
        assert sorted(os.listdir(tmp / name)) == ['predicted_t1ce.nii.gz']
    assert VS.done_line(runs['log']['plain_host']).endswith('| slices=16..20')
    assert VS.done_line(runs['log']['plain_host_z']).endswith('| slices=16..20 | norm=zscore')
