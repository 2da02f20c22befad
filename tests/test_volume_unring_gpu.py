"""GPU: --unring.  The kernels of csrc/volume_unring.hip against the fp64 restatement
(tests/volume_unring_ref.py) on seeded cumulative-sum noise: the line pass alone, then the whole stage, on lines of even and odd length,
lengths that are no multiple of the 4-voxel blocks, the shortest legal lines on strided axes, the longest (512), the largest shift bank
and window, int16 storage behind a slope and an intercept, and an input with a NaN and an inf; then the C ABI's refusals and
`predict_volume --unring` end to end.

The bar, for both: max |device - fp64| <= 1e-5 max |I|.  A voxel is excused from it only if the device chose another shift than the
restatement and the restatement's TV for the device's shift exceeds its minimum by at most 1e-5 (minimum + mean d_0 of that line); at
most 0.5 % of a case may be excused.  The checks on the inputs, which the seeds of CASES were chosen by with the restatement alone: its
fp32 mode needs no excuse at all, and no voxel's margin - the restatement's second smallest TV minus its smallest - lies between that
excuse and what storing the lines in fp32 can move a margin by, 4 (b - a + 1) half ulps of the largest |value| (each of the 2 (b - a + 1)
differences of the two scores moves by up to two half ulps): such a voxel is decided by the rounding of its input, not by the kernel."""
import json
import os

import numpy as np
import pytest
import torch

import volume_intake_ref as R
import volume_support as VS
import volume_unring_ref as U

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
BAR, TIE, EXCUSED = 1e-5, 1e-5, 0.005

# name: (shape [X,Y,Z], axes, shifts, window, stored as, seed): seeds at which the restatement's fp32 mode needs no excuse
CASES = {
    'even-odd': ((30, 21, 3), (0, 1), 20, (1, 3), 'f4', 1),
    'ragged': ((17, 16, 2), (0, 1), 20, (1, 3), 'f4', 1),
    'square': ((45, 45, 2), (0, 1), 20, (1, 3), 'f4', 1),
    'shortest-strided': ((8, 9, 10), (1, 2), 20, (1, 3), 'f4', 1),
    'longest-x': ((512, 8, 1), (0, 1), 20, (1, 3), 'f4', 8),
    'longest-y': ((8, 512, 1), (0, 1), 20, (1, 3), 'f4', 4),
    'lds-bound': ((30, 21, 3), (0, 1), 32, (2, 8), 'f4', 1),
    'int16': ((30, 21, 3), (0, 1), 20, (1, 3), 'i2', 1),
    'nonfinite': ((17, 16, 2), (0, 1), 20, (1, 3), 'nan', 1),
}
I2_SCALE = (0.5, -3.0)


def _stored(name):
    """-> (stored [X,Y,Z] array, (slope, inter))."""
    shape, axes, _, _, kind, seed = CASES[name]
    v = U.cumsum_noise(shape, axes, seed)
    if kind == 'i2':
        return np.asfortranarray(np.rint((v - I2_SCALE[1]) / I2_SCALE[0]).astype('<i2')), I2_SCALE
    vol = np.asfortranarray(v.astype('<f4'))
    if kind == 'nan':
        vol[3, 5, 1], vol[11, 2, 0] = np.nan, np.inf
    return vol, (1.0, 0.0)


@pytest.fixture(scope='module')
def cases():
    """{name: dict(raw, values fp32 [X,Y,Z], ref = the fp64 restatement of the stage, emu = its fp32 mode)} - computed once."""
    out = {}
    for name, (shape, axes, shifts, window, _, _) in CASES.items():
        vol, scale = _stored(name)
        values = R.values_float32(vol, *scale)
        kw = dict(axes=axes, shifts=shifts, window=window)
        out[name] = dict(raw=VS.raw_volume(vol, scale), values=values, kw=kw, ref=U.unring(values, **kw), emu=U.unring(values, dtype=np.float32, **kw))
    return out


def _mean_d0(lines, axis):
    return np.abs(lines - np.roll(lines, 1, axis)).mean(axis, keepdims=True)


def _near_tie(j_dev, j_ref, TV, lines, axis):
    """Where another shift than the restatement's was chosen, and the restatement's TV of that shift is within TIE of its minimum."""
    tv_dev = np.take_along_axis(TV, j_dev[None].astype(np.int64), 0)[0]
    tv_min = TV.min(0)
    assert np.array_equal(tv_min, np.take_along_axis(TV, j_ref[None].astype(np.int64), 0)[0])
    return (j_dev != j_ref) & (tv_dev - tv_min <= TIE * (tv_min + _mean_d0(lines, axis)))


def _decidable(TV, lines, axis, window):
    """No margin between the excuse and what fp32 storage of the lines alone can flip (the module's docstring)."""
    srt = np.sort(TV, 0)
    margin = srt[1] - srt[0]
    storage = 4 * (window[1] - window[0] + 1) * float(np.spacing(np.float32(np.abs(lines).max()))) / 2
    grey = (margin > TIE * (srt[0] + _mean_d0(lines, axis))) & (margin <= storage)
    return not grey.any()


def _held(what, got, want, near, scale):
    err = np.abs(got.astype(np.float64) - want)
    over = err > BAR * scale
    print(what, 'max error / max|I|', err.max() / scale, 'over the bar', int(over.sum()), 'near ties', int(near.sum()), 'of', err.size)
    assert not (over & ~near).any(), (what, float(err[over & ~near].max() / scale))
    assert int((over & near).sum()) <= EXCUSED * err.size
    return int((over & near).sum())


@pytest.mark.parametrize('name', list(CASES))
def test_line_pass_is_the_restatement(cases, name):
    """mud_volume_unring_lines alone, on the fp32 volume itself, along both in-plane axes: values, the map of the chosen shifts and the
    counters; out = in with accumulate adds; two runs give the same bits."""
    from mudiff_hip import ops, volume_unring as VU
    c = cases[name]
    shape, axes, shifts, window, _, _ = CASES[name]
    values = np.where(np.isfinite(c['values']), c['values'], np.float32(0))
    scale = float(np.abs(values).max())
    normal = 3 - axes[0] - axes[1]
    for axis in axes:
        n = shape[axis]
        table = torch.from_numpy(VU.shift_table(n, shifts)).to(DEV)
        lines = np.moveaxis(values.astype(np.float64), axis, -1)
        want, j_ref, TV = U.unring_lines(lines, shifts, *window)
        emu, j_emu, _ = U.unring_lines(lines, shifts, *window, dtype=np.float32)
        assert _held(f'{name} axis {axis} fp32 mode', emu, want, _near_tie(j_emu, j_ref, TV, lines, -1), scale) == 0 and np.array_equal(j_emu, j_ref)
        assert _decidable(TV, lines, -1, window)
        vol = VS.to_device_zyx(values)
        out = torch.full_like(vol, 2.0)
        got, jmap, counters = ops.volume_unring_lines(vol, shape, axis, normal, shifts, window, table, out=out, jmap=True)
        assert got is out and torch.equal(vol, VS.to_device_zyx(values))                       # the input is left alone
        got, j_dev = np.moveaxis(VS.to_host_xyz(got), axis, -1), np.moveaxis(VS.to_host_xyz(jmap), axis, -1)
        near = _near_tie(j_dev, j_ref, TV, lines, -1)
        _held(f'{name} axis {axis}', got, want, near, scale)
        assert not ((j_dev != j_ref) & ~near).any() and int(near.sum()) <= EXCUSED * near.size
        assert tuple(int(v) for v in counters.cpu()) == U.counters(j_dev, shifts)
        if not near.any():
            assert tuple(int(v) for v in counters.cpu()) == U.counters(j_ref, shifts)
        assert (j_dev != 0).any() and (j_dev > shifts).any() and (j_dev == 0).any()            # all three branches of the re-interpolation
        # in place, then added to what the output holds: identical bits, counters included
        again, jmap2, counters2 = ops.volume_unring_lines(vol.clone(), shape, axis, normal, shifts, window, table, jmap=True)
        assert torch.equal(again, out) and torch.equal(jmap2, jmap) and torch.equal(counters2, counters)
        added, _, counters3 = ops.volume_unring_lines(vol, shape, axis, normal, shifts, window, table, out=torch.full_like(vol, 2.0), accumulate=True)
        assert torch.equal(added, out + 2.0) and torch.equal(counters3, counters)


@pytest.mark.parametrize('name', list(CASES))
def test_the_stage_is_the_restatement(cases, name):
    """unring(): the filter pair, the two line passes, the report; non-finite voxels counted and read as 0; two runs, identical bits."""
    from mudiff_hip import ops, volume_intake as VI, volume_unring as VU
    c = cases[name]
    shape, axes, shifts, window, kind, _ = CASES[name]
    ref, emu, raw = c['ref'], c['emu'], c['raw']
    scale = float(np.abs(np.where(np.isfinite(c['values']), c['values'], 0)).max())
    # the filter pair
    tables = [torch.from_numpy(t).to(DEV) for t in VU.filter_tables(shape[axes[0]], shape[axes[1]])]
    ix, iy, bad = ops.volume_unring_filter(VI.upload(raw, DEV), *raw.kernel_meta('test'), axes, *tables)
    ix, iy = VS.to_host_xyz(ix), VS.to_host_xyz(iy)
    clean = np.where(np.isfinite(c['values']), c['values'], np.float32(0))
    print(name, 'filter: max error / max|I|', np.abs(ix - ref['ix']).max() / scale, np.abs(iy - ref['iy']).max() / scale)
    assert np.abs(ix - ref['ix']).max() <= BAR * scale and np.abs(iy - ref['iy']).max() <= BAR * scale
    assert np.array_equal(iy, clean - ix) and int(bad.cpu().numpy().view(np.uint32)[0]) == ref['nonfinite'] == (2 if kind == 'nan' else 0)
    # the stage
    out, rep = VU.unring(raw, DEV, maps=True, **c['kw'])
    got = out.values_float32()
    assert isinstance(out, VU.UnringedVolume) and got.shape == shape and got.dtype == np.float32 and out.affine is raw.affine
    jx, jy = (VS.to_host_xyz(j) for j in rep.pop('jmaps'))
    lx, ly = np.moveaxis(ref['ix'], axes[0], -1), np.moveaxis(ref['iy'], axes[1], -1)
    mv = lambda a, axis, lead=0: np.moveaxis(a, axis + lead, -1)      # noqa: E731
    near_x = np.moveaxis(_near_tie(mv(jx, axes[0]), mv(ref['jx'], axes[0]), mv(ref['tvx'], axes[0], 1), lx, -1), -1, axes[0])
    near_y = np.moveaxis(_near_tie(mv(jy, axes[1]), mv(ref['jy'], axes[1]), mv(ref['tvy'], axes[1], 1), ly, -1), -1, axes[1])
    near = near_x | near_y
    assert _held(f'{name} fp32 mode', emu['out'], ref['out'], np.zeros(shape, bool), scale) == 0
    assert _decidable(mv(ref['tvx'], axes[0], 1), lx, -1, window) and _decidable(mv(ref['tvy'], axes[1], 1), ly, -1, window)
    _held(name, got, ref['out'], near, scale)
    assert not ((jx != ref['jx']) & ~near_x).any() and not ((jy != ref['jy']) & ~near_y).any() and int(near.sum()) <= EXCUSED * near.size
    counters = rep.pop('counters')
    assert [tuple(k) for k in counters] == [U.counters(jx, shifts), U.counters(jy, shifts)]
    if not near.any():
        assert [tuple(k) for k in counters] == [U.counters(ref['jx'], shifts), U.counters(ref['jy'], shifts)]
    voxels = float(np.prod(shape))
    assert rep == dict(axes=list(axes), shifts=shifts, window=list(window), n=[shape[axes[0]], shape[axes[1]]], nonfinite=ref['nonfinite'],
                       moved=[counters[0][0] / voxels, counters[1][0] / voxels],
                       mean_abs_shift=[counters[0][1] / (2 * shifts + 1) / voxels, counters[1][1] / (2 * shifts + 1) / voxels])
    assert 0 < rep['moved'][0] < 1 and 0 < rep['mean_abs_shift'][1] < 0.5
    again, rep2 = VU.unring(raw, DEV, **c['kw'])
    assert np.array_equal(again.values_float32().view(np.uint32), got.view(np.uint32)) and rep2 == rep      # two runs: identical bits


def test_a_zero_slice_stays_zero_and_a_constant_one_constant():
    from mudiff_hip import volume_unring as VU
    v = U.cumsum_noise((21, 18, 4), (0, 1), 3).astype('<f4')
    v[:, :, 1] = 0.0
    v[:, :, 2] = 7.25
    out, rep = VU.unring(VS.raw_volume(np.asfortranarray(v)), DEV)
    got = out.values_float32()
    assert not got[:, :, 1].any() and np.abs(got[:, :, 2] - 7.25).max() <= 1e-5 * 7.25 and np.abs(got[:, :, 0] - v[:, :, 0]).max() > 1e-3
    want = U.unring(v)['out']
    assert np.abs(got[:, :, (0, 3)] - want[:, :, (0, 3)]).max() <= BAR * np.abs(v).max()


def test_c_abi_rejects_bad_arguments_without_launching():
    import mudiff_hip
    from mudiff_hip import volume_unring as VU
    lib = mudiff_hip.load()
    X, Y, Z = 20, 18, 2
    vol = torch.full((X * Y * Z,), 7, dtype=torch.int16, device=DEV)
    tw, kern = (torch.from_numpy(t).to(DEV) for t in VU.filter_tables(X, Y))
    table = torch.from_numpy(VU.shift_table(X, 20)).to(DEV)
    big = torch.from_numpy(VU.shift_table(X, 32)).to(DEV)
    ix, iy, out = (torch.full((X * Y * Z,), 5.0, dtype=torch.float32, device=DEV) for _ in range(3))
    src = torch.full((X * Y * Z,), 3.0, dtype=torch.float32, device=DEV)
    bad, jmap = torch.full((1,), 5, dtype=torch.int32, device=DEV), torch.full((X * Y * Z,), 5, dtype=torch.int8, device=DEV)
    counters = torch.full((2,), 5, dtype=torch.int64, device=DEV)
    p = lambda t: None if t is None else t.data_ptr()      # noqa: E731

    def split(v=vol, dt=4, dims=(X, Y, Z), axes=(0, 1), t=tw, k=kern, a=ix, b=iy, c=bad):
        return lib.mud_volume_unring_filter(p(v), dt, *dims, 1.0, 0.0, *axes, p(t), p(k), p(a), p(b), p(c), None)

    def lines(v=src, dims=(X, Y, Z), axis=0, normal=2, n=20, a=1, b=3, t=table, o=out, acc=0, j=jmap, c=counters):
        return lib.mud_volume_unring_lines(p(v), *dims, axis, normal, n, a, b, p(t), p(o), acc, p(j), p(c), None)

    for kw in (dict(v=None), dict(t=None), dict(k=None), dict(a=None), dict(b=None), dict(c=None), dict(dt=64), dict(dims=(0, Y, Z)), dict(axes=(0, 0)),
               dict(axes=(0, 3)), dict(axes=(-1, 1)), dict(b=ix), dict(dims=(513, 4, 1)), dict(dims=(4, 513, 1)), dict(dims=(1, Y, Z))):
        assert split(**kw) == 1, kw
    for kw in (dict(v=None), dict(t=None), dict(o=None), dict(c=None), dict(dims=(X, 0, Z)), dict(axis=2, normal=2), dict(axis=3), dict(normal=-1),
               dict(n=0), dict(n=33, t=big), dict(a=0), dict(a=4, b=3), dict(b=9), dict(dims=(7, Y, Z)), dict(dims=(513, 4, 1)), dict(a=2, b=8, axis=1, dims=(X, 17, Z))):
        assert lines(**kw) == 1, kw
    assert lines(n=33, t=big) == 1 and b'33 shifts' in lib.mud_last_error()
    assert lines(dims=(7, Y, Z)) == 1 and b'lines of 7 voxels' in lib.mud_last_error()
    torch.cuda.synchronize()
    assert float(ix.min()) == 5.0 and float(iy.max()) == 5.0 and float(out.min()) == 5.0 and int(bad[0]) == 5      # nothing launched or cleared
    assert int(jmap.min()) == 5 and counters.tolist() == [5, 5]
    assert split() == 0 and lines() == 0 and lines(n=32, t=big, a=2, b=8, j=None) == 0         # a NULL map is allowed; the library still works
    torch.cuda.synchronize()
    assert int(bad[0]) == 0 and float((ix - 3.5).abs().max()) <= 7e-5 and torch.equal(iy, 7.0 - ix)      # Gx = 1/2 at kx = ky = 0
    assert float(out.min()) == 3.0 == float(out.max()) and counters.tolist() == [0, 0]         # a constant volume: nothing moves


# ---------------------------------------------------------------------------------------------------
# end to end: the tiny model of the other volume tests, three ringing inputs on one grid
# ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def runs(tmp_path_factory):
    from mudiff_hip import volume as V
    tmp = tmp_path_factory.mktemp('ringing')
    VS.write_tiny_model(tmp)
    p = {k: str(tmp / f'{k}.nii.gz') for k in ('flair', 't2', 't1')}
    for seed, k in enumerate(p):
        ringing = U.phantom(24, seed)[0]
        vol = np.stack([ringing * (900.0 + 40.0 * z) for z in range(9)], axis=2)
        V.write_nifti(p[k], np.asfortranarray(vol.astype(np.float32)), np.eye(4))
    model = VS.model_argv(tmp, 2, 5, '--resize_back')
    inputs = ['--input_flair', p['flair'], '--input_t2', p['t2'], '--input_t1', p['t1']]
    jobs = {'unr_host': ['--unring'], 'unr_dev': ['--unring', '--device_intake'], 'plain_host': [], 'plain_dev': ['--device_intake']}
    jobs = {k: model + inputs + a + ['--output_dir', str(tmp / k)] for k, a in jobs.items()}
    manifest = tmp / 'cohort.tsv'
    manifest.write_text('id\tt1\tt1ce\tt2\tflair\ns0\t' + '\t'.join([p['t1'], '', p['t2'], p['flair']]) + '\n')
    cohort = model + ['--unring', '--manifest', str(manifest), '--output_dir', str(tmp / 'unr_cohort')]
    steps = [VS.cohort_step('unr_cohort', cohort)] + [VS.volume_step(k, argv) for k, argv in jobs.items()]
    log = VS.run_plan(tmp, steps, 900, ignore='RuntimeWarning')
    return dict(tmp=tmp, log=log, pred=lambda k: VS.payload(str(tmp / k / 'predicted_t1ce.nii.gz')))


def test_predict_volume_unring_end_to_end(runs):
    tmp = runs['tmp']
    where = {k: tmp / k for k in ('unr_host', 'unr_dev')}
    where['unr_cohort'] = tmp / 'unr_cohort' / 's0'
    reports = {}
    for name, d in where.items():
        rep = reports[name] = json.load(open(d / 'unring_t1ce.json'))
        assert list(rep) == ['FLAIR', 'T2', 'T1']
        for r in rep.values():
            assert (r['axes'], r['shifts'], r['window'], r['n'], r['nonfinite']) == ([0, 1], 20, [1, 3], [24, 24], 0)
            assert all(0.05 < m < 1 for m in r['moved']) and all(0 < s < 0.5 for s in r['mean_abs_shift'])
        assert VS.done_line(runs['log'][name]).endswith(' | unring=FLAIR,T2,T1')
    assert all(r == reports['unr_host'] for r in reports.values())
    assert runs['pred']('unr_host') == runs['pred']('unr_dev') == VS.payload(str(where['unr_cohort'] / 'predicted_t1ce.nii.gz'))
    assert runs['pred']('unr_host') != runs['pred']('plain_host')                  # and the corrected inputs reached the sampler


def test_without_the_flag_nothing_changes(runs):
    tmp = runs['tmp']
    assert runs['pred']('plain_dev') == runs['pred']('plain_host')
    for name in ('plain_host', 'plain_dev'):
        assert 'unring' not in runs['log'][name] and VS.done_line(runs['log'][name]).endswith('| slices=2..6')
        assert sorted(os.listdir(tmp / name)) == ['predicted_t1ce.nii.gz']
