"""GPU: --brain_extract.  The kernels of csrc/volume_brain.hip against the numpy restatement
(tests/volume_brain_ref.py), all comparisons exact: mud_volume_edt bit for bit against the brute-force definition on the adversarial masks
of the labelling tests, at four shapes (one with a line longer than a workgroup), three spacings and both values; mud_volume_edt_select
with the > / <= edge; the whole brain_mask() on the head phantom stored as int16 with slope / inter and as fp32 with a NaN and an inf, at
1 mm and at 1 x 1 x 2 mm; degenerate inputs; the C ABI's refusals; `predict_volume --brain_extract` end to end."""
import json
import os

import numpy as np
import pytest
import torch

import volume_brain_ref as B
import volume_foreground_ref as F
import volume_intake_ref as R
import volume_support as VS

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
EDT_SHAPES = ((37, 29, 23), (5, 4, 3), (70, 19, 11), (300, 5, 3))
EDT_SPACINGS = ((1.0, 1.0, 1.0), (0.9375, 0.9375, 3.0), (0.7, 1.3, 2.1))
I2_SCALE = (0.25, -3.0)
RADII = B.PHANTOM_RADII


def _edt_masks(shape):
    masks = {k: v for k, v in F.label_masks(shape).items() if k in ('random0.5', 'random0.7', 'comb', 'on', 'off')}
    corner, middle = np.zeros(shape, np.uint8), np.zeros(shape, np.uint8)
    corner[shape[0] - 1, 0, shape[2] - 1] = 1
    middle[shape[0] // 2, shape[1] // 2, shape[2] // 2] = 1
    return dict(masks, corner=corner, middle=middle)


@pytest.mark.parametrize('value', [1, 0])
@pytest.mark.parametrize('spacing', EDT_SPACINGS, ids=str)
@pytest.mark.parametrize('shape', EDT_SHAPES, ids=str)
def test_edt_is_the_restatement_bit_for_bit(shape, spacing, value):
    from mudiff_hip import ops
    masks = _edt_masks(shape)
    assert list(masks) == ['on', 'off', 'comb', 'random0.5', 'random0.7', 'corner', 'middle']
    for name, mask in masks.items():
        want = B.edt2(mask, value, spacing)
        dev = VS.to_device_zyx(mask)
        d2 = ops.volume_edt(dev, shape, value, spacing)
        got = VS.to_host_xyz(d2)
        assert got.dtype == np.float64 and got.shape == shape
        same = got.view(np.int64) == want.view(np.int64)
        assert same.all(), (name, int((~same).sum()), got[~same][:3], want[~same][:3])
        if (name, value) in (('on', 0), ('off', 1)):
            assert np.isposinf(got).all()
        else:
            assert np.isfinite(got).all() and (got == 0).sum() == ((mask != 0) == (value != 0)).sum()
        assert torch.equal(ops.volume_edt(dev, shape, value, spacing).view(torch.int64), d2.view(torch.int64))      # two runs: identical bits


def test_edt_select_is_exact():
    from mudiff_hip import ops
    shape, spacing = (37, 29, 23), (0.9375, 0.9375, 3.0)
    mask = F.label_masks(shape)['random0.7']
    within = F.label_masks(shape)['comb']
    d2 = ops.volume_edt(VS.to_device_zyx(mask), shape, 0, spacing)
    host = VS.to_host_xyz(d2)
    present = np.unique(host[host > 0])
    assert present.size >= 3
    for r2 in (0.0, float(present[0]), float(present[1]), float(np.nextafter(present[1], 0.0)), 7.25, 1e300):
        for above in (1, 0):
            for inside in (None, within):
                got, count = ops.volume_edt_select(d2, r2, above, None if inside is None else VS.to_device_zyx(inside))
                want = (host > r2) if above else (host <= r2)
                if inside is not None:
                    want = want & (inside != 0)
                assert got.dtype == torch.uint8 and got.shape == d2.shape and np.array_equal(VS.to_host_xyz(got), want.astype(np.uint8)), (r2, above)
                assert int(count[0]) == int(want.sum())
    inf = ops.volume_edt(VS.to_device_zyx(np.ones(shape, np.uint8)), shape, 0, spacing)          # +inf everywhere: above any radius, within none
    assert int(ops.volume_edt_select(inf, 1e300, 1)[1][0]) == int(np.prod(shape)) and int(ops.volume_edt_select(inf, 1e300, 0)[1][0]) == 0


def _stored(kind, spacing):
    """-> (stored volume, (slope, inter), labels, affine): the head phantom as int16 behind a slope and an intercept, or as fp32 with a
    NaN and an inf planted in the air; at 1 x 1 x 2 mm every second plane of it."""
    p, labels = B.phantom()
    if spacing[2] == 2.0:
        p, labels = p[:, :, ::2], labels[:, :, ::2]
    affine = np.diag(list(spacing) + [1.0])
    if kind == 'i2':
        return np.asfortranarray(np.rint((p - I2_SCALE[1]) / I2_SCALE[0]).astype('<i2')), I2_SCALE, labels, affine
    vol = np.asfortranarray(p.astype('<f4'))
    assert labels[0, 0, 0] == B.AIR and labels[-1, 1, 2] == B.AIR
    vol[0, 0, 0], vol[-1, 1, 2] = np.nan, np.inf
    return vol, (1.0, 0.0), labels, affine


@pytest.mark.parametrize('spacing', [(1.0, 1.0, 1.0), (1.0, 1.0, 2.0)], ids=str)
@pytest.mark.parametrize('kind', ['i2', 'f4'])
def test_brain_mask_is_the_restatement(kind, spacing):
    from mudiff_hip import volume_brain as VBR
    vol, scale, labels, affine = _stored(kind, spacing)
    raw, values = VS.raw_volume(vol, scale, affine), R.values_float32(vol, *scale)
    for options in (dict(), dict(keep_holes=True), dict(bins=64)):
        want, want_report, _ = B.brain_mask(values, spacing=spacing, **RADII, **options)
        mask, report = VBR.brain_mask(raw, DEV, **RADII, **options)
        print(kind, spacing, options, report)
        assert mask.dtype == torch.uint8 and tuple(mask.shape) == vol.shape[::-1]
        assert np.array_equal(VS.to_host_xyz(mask), want.astype(np.uint8))
        assert report == want_report and report['threshold'] is not None and report['spacing'] == list(spacing)
        if not options.get('keep_holes'):
            assert B.properties(VS.to_host_xyz(mask), labels, spacing, RADII['dilate_mm']) == dict(no_scalp=True, no_air=True, ventricle=True, bridge_cut=True,
                                                                                         short_of_scalp=True, brain=True)
    if kind == 'f4':
        assert report['candidates'] == int((labels != B.AIR).sum())                    # the NaN and the inf are no candidates
    again, report2 = VBR.brain_mask(raw, DEV, **RADII, bins=64)
    assert report2 == report and torch.equal(again, mask)                              # two runs: identical bits
    stripped = VBR.apply_mask(raw, mask, DEV)                                          # applying it: the volume's own geometry
    got = stripped.values_float32()
    assert got.shape == raw.shape and stripped.affine is raw.affine and stripped.header is raw.header
    keep = VS.to_host_xyz(mask) != 0
    assert np.array_equal(got[keep].view(np.uint32), values[keep].view(np.uint32)) and not got[~keep].any()


def test_degenerate_inputs_come_back_untouched():
    """All zeros (no candidate), a constant volume, two values (zeros and one other value: hi == lo) and an erosion radius larger than the
    object: no mask, and the restatement's report."""
    from mudiff_hip import volume_brain as VBR
    two = np.full((9, 8, 7), 7.0, '<f4', order='F')
    two[4:, 4:, 4:], two[0, 0, 0] = 0.0, np.nan
    for vol in (np.zeros((9, 8, 7), np.int16, order='F'), np.full((9, 8, 7), 5, np.int16, order='F'), two):
        mask, report = VBR.brain_mask(VS.raw_volume(vol), DEV)
        assert mask is None and report['threshold'] is None and report['kept'] == 0
        assert report == B.brain_mask(R.values_float32(vol))[1]
    assert (report['lo'], report['hi'], report['candidates']) == (7.0, 7.0, 9 * 8 * 7 - 5 * 4 * 3 - 1)
    block = np.zeros((20, 18, 16), np.int16, order='F')
    block[:] = 10
    block[6:13, 6:12, 5:11] = 900
    mask, report = VBR.brain_mask(VS.raw_volume(block), DEV, erode_mm=4.0, dilate_mm=5.0)
    assert mask is None and report['threshold'] is not None and (report['tissue'], report['eroded'], report['core'], report['kept']) == (7 * 6 * 6, 0, 0, 0)
    assert report == B.brain_mask(R.values_float32(block), erode_mm=4.0, dilate_mm=5.0)[1]
    mask, report = VBR.brain_mask(VS.raw_volume(block), DEV, erode_mm=2.0, dilate_mm=2.0)        # (one voxel less and something is left)
    assert mask is not None and report == B.brain_mask(R.values_float32(block), erode_mm=2.0, dilate_mm=2.0)[1] and report['eroded'] > 0


def test_c_abi_rejects_bad_arguments_without_launching():
    import mudiff_hip
    lib = mudiff_hip.load()
    X, Y, Z = 16, 8, 4
    n = X * Y * Z
    mask = torch.full((n,), 1, dtype=torch.uint8, device=DEV)
    d2 = torch.full((n + 2,), 5.0, dtype=torch.float64, device=DEV)
    out = torch.full((n,), 5, dtype=torch.uint8, device=DEV)
    count = torch.full((1,), 5, dtype=torch.int32, device=DEV)
    p = lambda t, off=0: None if t is None else t.data_ptr() + off      # noqa: E731
    nan, inf = float('nan'), float('inf')

    def edt(m=mask, dims=(X, Y, Z), value=1, spacing=(1.0, 1.0, 1.0), d=d2, off=0):
        return lib.mud_volume_edt(p(m), *dims, value, *spacing, p(d, off), None)

    def select(d=d2, off=0, count_=n, r2=1.0, above=1, w=None, o=out, c=count):
        return lib.mud_volume_edt_select(p(d, off), count_, r2, above, p(w), p(o), p(c), None)

    bad = [dict(value=2), dict(value=-1), dict(m=None), dict(d=None), dict(off=8), dict(dims=(0, Y, Z)), dict(dims=(X, Y, -1)),
           dict(dims=(2048, 1024, 1024)), dict(dims=(1025, 2, 2)), dict(dims=(2, 1025, 2)), dict(dims=(2, 2, 1025))]
    bad += [dict(spacing=s) for s in ((0.0, 1.0, 1.0), (1.0, nan, 1.0), (1.0, 1.0, -1.0), (inf, 1.0, 1.0))]
    for kw in bad:
        assert edt(**kw) == 1 and lib.mud_last_error().startswith(b'mud_volume_edt:'), kw
    assert edt(dims=(2, 1025, 2)) == 1 and b'1024' in lib.mud_last_error()              # the limit is stated
    for kw in (dict(d=None), dict(o=None), dict(c=None), dict(off=4), dict(count_=0), dict(count_=1 << 31), dict(r2=-1.0), dict(r2=nan), dict(r2=inf),
               dict(above=2), dict(w=out)):
        assert select(**kw) == 1 and lib.mud_last_error().startswith(b'mud_volume_edt_select:'), kw
    torch.cuda.synchronize()
    assert float(d2.min()) == 5.0 and float(d2.max()) == 5.0 and int(out.min()) == 5 and int(out.max()) == 5 and int(count[0]) == 5      # nothing ran
    # the library still works: every voxel is on
    assert edt() == 0 and select(r2=0.0, above=0, w=mask) == 0
    torch.cuda.synchronize()
    assert float(d2[:n].max()) == 0.0 and float(d2[n:].min()) == 5.0 and int(out.min()) == 1 and int(count[0]) == n


# ---------------------------------------------------------------------------------------------------
# end to end: the tiny model of the other volume tests; the phantom is the T1 input, FLAIR (the grid) and T2 carry the same head on a
# grid that is shifted by whole voxels, so that --regrid reproduces the T1 voxels exactly
# ---------------------------------------------------------------------------------------------------
SHIFT = (2, -1, 1)


def _on_shifted_grid(vol):
    """vol on the grid whose voxel i is the voxel i + SHIFT of vol's own grid (0 outside)."""
    out = np.zeros_like(vol)
    src, dst = [], []
    for t, n in zip(SHIFT, vol.shape):
        src.append(slice(max(t, 0), n + min(t, 0)))
        dst.append(slice(max(-t, 0), n + min(-t, 0)))
    out[tuple(dst)] = vol[tuple(src)]
    return out


@pytest.fixture(scope='module')
def runs(tmp_path_factory):
    from mudiff_hip import volume as V
    tmp = tmp_path_factory.mktemp('stripped')
    VS.write_tiny_model(tmp)
    p = {k: str(tmp / f'{k}.nii.gz') for k in ('flair', 't2', 't1')}
    grid = np.eye(4)
    grid[:3, 3] = SHIFT
    V.write_nifti(p['t1'], np.asfortranarray(B.phantom()[0]), np.eye(4))
    for seed, k in ((12, 'flair'), (13, 't2')):
        V.write_nifti(p[k], np.asfortranarray(_on_shifted_grid(B.phantom(seed=seed)[0])), grid)
    model = VS.model_argv(tmp, 2, 5, '--resize_back', '--regrid')
    inputs = ['--input_flair', p['flair'], '--input_t2', p['t2'], '--input_t1', p['t1']]
    brain = ['--brain_extract', '--brain_mask_out', '--brain_erode_mm', str(RADII['erode_mm']), '--brain_dilate_mm', str(RADII['dilate_mm'])]
    jobs = {'brain_host': brain, 'brain_dev': brain + ['--device_intake'], 'plain': [], 'unparsed': []}
    jobs = {k: model + inputs + a + ['--output_dir', str(tmp / k)] for k, a in jobs.items()}
    strip = {'unparsed': ['brain_']}                                               # the options as a parser without the new flags leaves them
    log = VS.run_plan(tmp, [VS.volume_step(k, argv, strip=strip.get(k, [])) for k, argv in jobs.items()], 600, ignore='RuntimeWarning')
    return dict(tmp=tmp, log=log, pred=lambda k: VS.payload(str(tmp / k / 'predicted_t1ce.nii.gz')))


def test_predict_volume_brain_extract_end_to_end(runs):
    from mudiff_hip import volume as V
    tmp = runs['tmp']
    t1_on_grid = _on_shifted_grid(B.phantom()[0])                                      # what --regrid makes of the T1 input, exactly
    want, want_report, _ = B.brain_mask(t1_on_grid, **RADII)
    assert B.properties(want, _on_shifted_grid(B.phantom()[1]), (1.0, 1.0, 1.0), RADII['dilate_mm'])['no_scalp']
    for name in ('brain_host', 'brain_dev'):
        assert VS.done_line(runs['log'][name]).endswith(' | brain=T1') and ' | regrid=T1' in VS.done_line(runs['log'][name])
        assert sorted(os.listdir(tmp / name)) == ['brain_t1ce.json', 'brain_t1ce_mask.nii.gz', 'predicted_t1ce.nii.gz']
        assert json.load(open(tmp / name / 'brain_t1ce.json')) == dict(want_report, source='T1')
        mask, affine, _ = V.read_nifti(str(tmp / name / 'brain_t1ce_mask.nii.gz'))
        assert np.array_equal(np.asarray(mask), want.astype(np.uint8)) and np.array_equal(np.asarray(affine)[:3, 3], SHIFT)
    assert runs['pred']('brain_host') == runs['pred']('brain_dev')                     # host file == device file
    assert VS.payload(str(tmp / 'brain_host' / 'brain_t1ce_mask.nii.gz')) == VS.payload(str(tmp / 'brain_dev' / 'brain_t1ce_mask.nii.gz'))
    assert runs['pred']('brain_host') != runs['pred']('plain')


def test_without_the_flag_nothing_changes(runs):
    tmp = runs['tmp']
    assert runs['pred']('plain') == runs['pred']('unparsed')
    assert VS.done_line(runs['log']['plain']).replace(str(tmp / 'plain'), 'OUT') == VS.done_line(runs['log']['unparsed']).replace(str(tmp / 'unparsed'), 'OUT')
    for name in ('plain', 'unparsed'):
        assert 'brain' not in runs['log'][name] and VS.done_line(runs['log'][name]).endswith(' | regrid=T1')
        assert sorted(os.listdir(tmp / name)) == ['predicted_t1ce.nii.gz']
