"""GPU: --foreground.  The kernels of csrc/volume_foreground.hip against the numpy restatement
(tests/volume_foreground_ref.py), all comparisons exact: the labelling alone, for the values 1 and 0, on the adversarial masks at 37 x 29 x
23, 5 x 4 x 3 and 70 x 19 x 11 (three 32 x 8 x 4 tiles along every axis and a multiple of none), with the census and the winner; the
morphology against scipy; the whole foreground() on the phantom stored as int16 with slope / inter and as fp32 with a NaN, an inf and a
block of zeros; degenerate inputs; the C ABI's refusals; `predict_volume --foreground` end to end."""
import json
import os

import numpy as np
import pytest
import torch

import volume_foreground_ref as F
import volume_intake_ref as R
import volume_support as VS

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
LABEL_SHAPES = ((37, 29, 23), (5, 4, 3), (70, 19, 11))
I2_SCALE = (0.25, -3.0)


@pytest.fixture(scope='module')
def label_references():
    """{(shape, name, value): (mask, labels, counts, face, winner, components)} of the restatement - computed once."""
    ref = {}
    for shape in LABEL_SHAPES:
        for name, mask in F.label_masks(shape).items():
            for value in (1, 0):
                lab = F.label(mask, value)
                ref[shape, name, value] = (mask, lab) + F.census(lab)
    return ref


@pytest.mark.parametrize('value', [1, 0])
@pytest.mark.parametrize('shape', LABEL_SHAPES)
def test_labels_census_and_winner_are_the_restatement(label_references, shape, value):
    from mudiff_hip import ops
    n = int(np.prod(shape))
    for name in F.label_masks(shape):
        mask, want, counts, face, winner, components = label_references[shape, name, value]
        labels = ops.volume_fg_label(VS.to_device_zyx(mask), shape, value)
        got = VS.to_host_xyz(labels)
        assert got.dtype == np.int32 and np.array_equal(got, want), (name, int((got != want).sum()))
        census, summary = ops.volume_fg_census(labels, shape)
        census = census.cpu().numpy().view(np.uint32)
        best, roots = (int(v) for v in summary.cpu().numpy().view(np.uint64))
        assert np.array_equal((census & 0x7FFFFFFF).astype(np.int64), counts) and np.array_equal((census >> 31).astype(bool), face), name
        assert roots == components, name
        if components:
            assert (best >> 32, 0xFFFFFFFF - (best & 0xFFFFFFFF)) == (int(counts[winner]), winner), name
        else:
            assert best == 0
        again = ops.volume_fg_label(VS.to_device_zyx(mask), shape, value)
        assert torch.equal(again, labels)                                              # two runs: identical bits
        if components:                                                                 # keeping the winner
            kept, count = ops.volume_fg_select(labels, None, winner, False)
            assert np.array_equal(VS.to_host_xyz(kept), (want == winner).astype(np.uint8)) and int(count[0]) == int(counts[winner])
    if value == 1:
        checker = label_references[shape, 'checker', 1]
        assert checker[4] == 0 and checker[5] == (n + 1) // 2                          # the tie goes to index 0
        assert label_references[shape, 'serpentine', 1][5] == 1


@pytest.mark.parametrize('shape', LABEL_SHAPES)
def test_filling_the_holes_is_the_restatement(label_references, shape):
    from mudiff_hip import ops
    for name in ('random0.7', 'random0.5', 'comb', 'on', 'off'):
        mask = label_references[shape, name, 1][0]
        dev = VS.to_device_zyx(mask)
        labels = ops.volume_fg_label(dev, shape, 0)
        filled, count = ops.volume_fg_select(labels, ops.volume_fg_census(labels, shape)[0], 0, True, dev)
        want = F.fill_holes(mask)
        assert filled is dev and np.array_equal(VS.to_host_xyz(filled), want.astype(np.uint8)), name
        assert int(count[0]) == int(want.sum()) - int((mask != 0).sum())


@pytest.mark.parametrize('steps', [1, 3])
def test_morphology_is_scipys(steps):
    from scipy import ndimage
    from mudiff_hip import ops
    six = ndimage.generate_binary_structure(3, 1)
    for shape in LABEL_SHAPES:
        for name, mask in F.label_masks(shape).items():
            if name not in ('on', 'single', 'random0.7', 'random0.5', 'comb'):
                continue
            eroded = dilated = VS.to_device_zyx(mask)
            for _ in range(steps):
                eroded, dilated = ops.volume_fg_morph(eroded, shape, False), ops.volume_fg_morph(dilated, shape, True)
            assert np.array_equal(VS.to_host_xyz(eroded) != 0, ndimage.binary_erosion(mask != 0, six, iterations=steps, border_value=1)), (shape, name)
            assert np.array_equal(VS.to_host_xyz(dilated) != 0, ndimage.binary_dilation(mask != 0, six, iterations=steps, border_value=0)), (shape, name)
            assert set(np.unique(VS.to_host_xyz(eroded))) <= {0, 1} and set(np.unique(VS.to_host_xyz(dilated))) <= {0, 1}


def _stored(kind):
    """-> (stored volume, (slope, inter)): the phantom as int16 behind a slope and an intercept, or as fp32 with the specials."""
    p = F.phantom()[0]
    if kind == 'i2':
        return np.asfortranarray(np.rint((p - I2_SCALE[1]) / I2_SCALE[0]).astype('<i2')), I2_SCALE
    vol = np.asfortranarray(p.astype('<f4'))
    vol[18, 14, 11], vol[0, 28, 22], vol[36, 0, 0] = np.nan, np.inf, -np.inf         # a NaN inside the ventricle, infs outside the head
    vol[30:34, 20:24, 2:5] = 0.0                                                      # a block of exact zeros in the air
    vol[17, 13, 10] = -0.0
    return vol, (1.0, 0.0)


@pytest.fixture(scope='module')
def phantoms():
    """{kind: (raw, fp32 values [X,Y,Z])} - computed once."""
    out = {}
    for kind in ('i2', 'f4'):
        vol, scale = _stored(kind)
        out[kind] = (VS.raw_volume(vol, scale), np.asfortranarray(R.values_float32(vol, *scale)))
    return out


@pytest.mark.parametrize('options', [dict(), dict(open=1), dict(keep_holes=True), dict(bins=64, open=2)], ids=str)
@pytest.mark.parametrize('kind', ['i2', 'f4'])
def test_foreground_is_the_restatement(phantoms, kind, options):
    from mudiff_hip import volume_foreground as VF
    raw, values = phantoms[kind]
    head, ventricle, block = F.phantom()[1:]
    want, want_mask, want_report, _ = F.foreground(values, **options)
    out, report = VF.foreground(raw, DEV, mask_out=True, **options)
    got = out.values_float32()
    print(kind, options, report)
    assert isinstance(out, VF.MaskedVolume) and got.shape == raw.shape == out.shape and got.dtype == np.float32 and out.code == 16
    assert out.affine is raw.affine and out.header is raw.header and not out.scaled and out.dev.shape == raw.shape[::-1]
    assert np.array_equal(out.mask, want_mask.astype(np.uint8)) and out.mask.dtype == np.uint8
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert report == want_report and report['threshold'] is not None
    assert not out.mask[block].any() and (options.get('keep_holes') or out.mask[ventricle].all())
    if kind == 'f4':
        assert report['candidates'] == values.size - 3 - 48 - 1
        if not options.get('keep_holes'):
            assert np.isnan(got[18, 14, 11])                                          # inside a filled hole: the bits stay
        assert got[0, 28, 22] == 0 and got[36, 0, 0] == 0 and not np.signbit(got[17, 13, 10] if not out.mask[17, 13, 10] else 0.0)
    again, report2 = VF.foreground(raw, DEV, **options)
    assert report2 == report and again.mask is None
    assert np.array_equal(again.values_float32().view(np.uint32), got.view(np.uint32))      # two runs: identical bits


def test_degenerate_inputs_come_back_untouched():
    """All zeros (no candidate), a constant volume, and a two-valued volume - zeros and one other value, with non-finite voxels that are no
    candidates either - whose candidates all sit in one bin (hi == lo): the same object, threshold None, the restatement's report.  (With
    hi > lo the smallest candidate is in bin 0 and the largest in the last bin, so fewer than two non-empty bins cannot occur on the device;
    otsu_bin's None is covered by the host tests.)"""
    from mudiff_hip import volume_foreground as VF
    two = np.full((9, 8, 7), 7.0, '<f4', order='F')
    two[1:3, 1:3, 1:3], two[4:, 4:, 4:], two[0, 0, 0] = np.inf, 0.0, np.nan
    for vol, candidates in ((np.zeros((9, 8, 7), np.int16, order='F'), 0), (np.full((9, 8, 7), 5, np.int16, order='F'), 9 * 8 * 7),
                            (two, 9 * 8 * 7 - 8 - 5 * 4 * 3 - 1)):
        flat = VS.raw_volume(vol)
        same, report = VF.foreground(flat, DEV)
        assert same is flat and report['threshold'] is None and report['bin'] is None and report['candidates'] == candidates
        assert report == F.foreground(R.values_float32(vol))[2]
    assert (report['lo'], report['hi']) == (7.0, 7.0)


def test_c_abi_rejects_bad_arguments_without_launching():
    import mudiff_hip
    lib = mudiff_hip.load()
    X, Y, Z = 16, 8, 4
    n = X * Y * Z
    vol = torch.full((n,), 7, dtype=torch.int16, device=DEV)
    rng = torch.full((3,), 5, dtype=torch.int32, device=DEV)
    hist = torch.full((1024,), 5, dtype=torch.int32, device=DEV)
    mask = torch.full((n,), 5, dtype=torch.uint8, device=DEV)
    mask2 = torch.full((n,), 5, dtype=torch.uint8, device=DEV)
    labels = torch.full((n,), 5, dtype=torch.int32, device=DEV)
    census = torch.full((n,), 5, dtype=torch.int32, device=DEV)
    summary = torch.full((2,), 5, dtype=torch.int64, device=DEV)
    out = torch.full((n,), 5.0, dtype=torch.float32, device=DEV)
    count = torch.full((1,), 5, dtype=torch.int32, device=DEV)
    p = lambda t: None if t is None else t.data_ptr()      # noqa: E731
    nan, inf = float('nan'), float('inf')

    def frange(v=vol, dt=4, dims=(X, Y, Z), r=rng):
        return lib.mud_volume_fg_range(p(v), dt, *dims, 1.0, 0.0, p(r), None)

    def fhist(v=vol, dt=4, dims=(X, Y, Z), lo=0.0, scale=1.0, bins=256, h=hist):
        return lib.mud_volume_fg_hist(p(v), dt, *dims, 1.0, 0.0, lo, scale, bins, p(h), None)

    def fmask(v=vol, dt=4, dims=(X, Y, Z), lo=0.0, scale=1.0, bins=256, k=3, m=mask):
        return lib.mud_volume_fg_mask(p(v), dt, *dims, 1.0, 0.0, lo, scale, bins, k, p(m), None)

    def morph(a=mask, dims=(X, Y, Z), dilate=0, b=mask2):
        return lib.mud_volume_fg_morph(p(a), *dims, dilate, p(b), None)

    def label(m=mask, dims=(X, Y, Z), value=1, lab=labels):
        return lib.mud_volume_fg_label(p(m), *dims, value, p(lab), None)

    def fcensus(lab=labels, dims=(X, Y, Z), c=census, s=summary):
        return lib.mud_volume_fg_census(p(lab), *dims, p(c), p(s), None)

    def select(lab=labels, c=census, count_=n, root=0, holes=0, m=mask, cnt=count):
        return lib.mud_volume_fg_select(p(lab), p(c), count_, root, holes, p(m), p(cnt), None)

    def apply(v=vol, dt=4, dims=(X, Y, Z), m=mask, o=out, r=count):
        return lib.mud_volume_fg_apply(p(v), dt, *dims, 1.0, 0.0, p(m), p(o), p(r), None)

    sizes = (dict(dims=(0, Y, Z)), dict(dims=(X, Y, -1)), dict(dims=(2048, 1024, 1024)))
    for kw in (dict(v=None), dict(r=None), dict(dt=64)) + sizes:
        assert frange(**kw) == 1, kw
    bins = (dict(bins=15), dict(bins=1025), dict(scale=0.0), dict(scale=-1.0), dict(scale=nan), dict(scale=inf), dict(lo=nan))
    for kw in (dict(v=None), dict(h=None), dict(dt=3)) + sizes + bins:
        assert fhist(**kw) == 1, kw
    for kw in (dict(v=None), dict(m=None), dict(dt=3), dict(k=-1), dict(k=255), dict(bins=16, k=15)) + sizes + bins:
        assert fmask(**kw) == 1, kw
    assert fmask(k=255) == 1 and b'threshold bin 255' in lib.mud_last_error()
    for kw in (dict(a=None), dict(b=None), dict(b=mask), dict(dilate=2)) + sizes:
        assert morph(**kw) == 1, kw
    for kw in (dict(m=None), dict(lab=None), dict(value=2), dict(value=-1)) + sizes:
        assert label(**kw) == 1, kw
    for kw in (dict(lab=None), dict(c=None), dict(s=None)) + sizes:
        assert fcensus(**kw) == 1, kw
    for kw in (dict(lab=None), dict(m=None), dict(cnt=None), dict(count_=0), dict(count_=1 << 31), dict(root=-1), dict(root=n), dict(holes=2),
               dict(holes=1, c=None)):
        assert select(**kw) == 1, kw
    for kw in (dict(v=None), dict(m=None), dict(o=None), dict(r=None), dict(dt=64)) + sizes:
        assert apply(**kw) == 1, kw
    torch.cuda.synchronize()
    for t in (rng, hist, mask, mask2, labels, census, summary, count):                 # nothing launched or cleared
        assert int(t.min()) == 5 and int(t.max()) == 5
    assert float(out.min()) == 5.0 and float(out.max()) == 5.0
    # the library still works: a constant 7 everywhere
    assert frange() == 0 and fhist(lo=0.0, scale=1.0, bins=16) == 0 and fmask(bins=16, k=3) == 0
    assert morph() == 0 and label() == 0 and fcensus() == 0 and select() == 0 and apply() == 0
    torch.cuda.synchronize()
    assert int(rng[2]) == n and int(hist[7]) == n and int(hist.sum()) == n + 5 * (1024 - 16) and int(mask.min()) == 1
    assert int(mask2.min()) == 1 and int(labels.max()) == 0 and int(census[0]) == n - (1 << 31) and int(summary[1]) == 1
    assert int(count[0]) == 0 and float(out.min()) == 7.0 and float(out.max()) == 7.0


# ---------------------------------------------------------------------------------------------------
# end to end: the tiny model of the other volume tests, three phantom inputs with Rician air
# ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def runs(tmp_path_factory):
    from mudiff_hip import volume as V
    tmp = tmp_path_factory.mktemp('heads')
    VS.write_tiny_model(tmp)
    p = {k: str(tmp / f'{k}.nii.gz') for k in ('flair', 't2', 't1')}
    for seed, k in enumerate(p):
        V.write_nifti(p[k], np.asfortranarray(F.phantom(seed=5 + seed)[0]), np.eye(4))
    model = VS.model_argv(tmp, 2, 5, '--resize_back')
    inputs = ['--input_flair', p['flair'], '--input_t2', p['t2'], '--input_t1', p['t1']]
    jobs = {'fg_host': ['--foreground'], 'fg_dev': ['--foreground', '--device_intake'], 'fg_host_z': ['--foreground', '--norm', 'zscore'],
            'fg_dev_z': ['--foreground', '--norm', 'zscore', '--device_intake'],
            'fg_all': ['--denoise', '--foreground', '--bias_correct', '--foreground_mask_out'],
            'plain_host': [], 'plain_dev': ['--device_intake'], 'plain_host_z': ['--norm', 'zscore']}
    jobs = {k: model + inputs + a + ['--output_dir', str(tmp / k)] for k, a in jobs.items()}
    manifest = tmp / 'cohort.tsv'
    manifest.write_text('id\tt1\tt1ce\tt2\tflair\ns0\t' + '\t'.join([p['t1'], '', p['t2'], p['flair']]) + '\n')
    cohort = model + ['--foreground', '--manifest', str(manifest), '--output_dir', str(tmp / 'fg_cohort')]
    steps = [VS.cohort_step('fg_cohort', cohort)] + [VS.volume_step(k, argv) for k, argv in jobs.items()]
    log = VS.run_plan(tmp, steps, 900, ignore='RuntimeWarning')
    return dict(tmp=tmp, log=log, pred=lambda k: VS.payload(str(tmp / k / 'predicted_t1ce.nii.gz')))


def test_predict_volume_foreground_end_to_end(runs):
    tmp = runs['tmp']
    where = {k: tmp / k for k in ('fg_host', 'fg_dev', 'fg_host_z', 'fg_dev_z')}
    where['fg_cohort'] = tmp / 'fg_cohort' / 's0'
    reports = {}
    for name, d in where.items():
        rep = reports[name] = json.load(open(d / 'foreground_t1ce.json'))
        assert list(rep) == ['FLAIR', 'T2', 'T1']
        for seed, r in enumerate(rep.values()):
            assert r == F.foreground(F.phantom(seed=5 + seed)[0])[2]                   # the report is the restatement's
            assert r['components'] >= 2 and r['filled'] >= 81 and r['removed'] > 15000 and (r['bins'], r['open'], r['keep_holes']) == (256, 0, False)
        assert VS.done_line(runs['log'][name]).endswith(' | foreground=FLAIR,T2,T1')
        assert sorted(os.listdir(d)) == ['foreground_t1ce.json', 'predicted_t1ce.nii.gz']
    assert all(r == reports['fg_host'] for r in reports.values())
    assert runs['pred']('fg_host') == runs['pred']('fg_dev') == VS.payload(str(where['fg_cohort'] / 'predicted_t1ce.nii.gz'))
    assert runs['pred']('fg_host_z') == runs['pred']('fg_dev_z')                       # host file == device file in both --norm modes
    assert runs['pred']('fg_host') != runs['pred']('plain_host') and runs['pred']('fg_host_z') != runs['pred']('plain_host_z')
    assert VS.done_line(runs['log']['fg_host']).replace(str(where['fg_host']), 'OUT') == VS.done_line(runs['log']['fg_dev']).replace(str(where['fg_dev']), 'OUT')


def test_all_three_stages_together_and_the_masks(runs):
    from mudiff_hip import volume as V
    tmp = runs['tmp']
    assert VS.done_line(runs['log']['fg_all']).endswith(' | bias=FLAIR,T2,T1 | denoise=FLAIR,T2,T1 | foreground=FLAIR,T2,T1')
    assert sorted(os.listdir(tmp / 'fg_all')) == ['bias_t1ce.json', 'denoise_t1ce.json', 'foreground_t1ce.json', 'foreground_t1ce_flair.nii.gz',
                                                  'foreground_t1ce_t1.nii.gz', 'foreground_t1ce_t2.nii.gz', 'predicted_t1ce.nii.gz']
    head = F.phantom()[1]
    rep = json.load(open(tmp / 'fg_all' / 'foreground_t1ce.json'))
    for name in ('flair', 't2', 't1'):
        mask = np.asarray(V.read_nifti(str(tmp / 'fg_all' / f'foreground_t1ce_{name}.nii.gz'))[0])
        assert mask.shape == F.PHANTOM_SHAPE and int(mask.sum()) == rep[name.upper()]['kept'] and F.dice(mask != 0, head) > 0.95      # (a sanity bound: the head, not the air or the block)


def test_without_the_flag_nothing_changes(runs):
    tmp = runs['tmp']
    assert runs['pred']('plain_dev') == runs['pred']('plain_host')
    for name in ('plain_host', 'plain_dev', 'plain_host_z'):
        assert 'foreground' not in runs['log'][name] and VS.done_line(runs['log'][name]).endswith('| slices=9..13' + (' | norm=zscore' if name.endswith('_z') else ''))
        assert sorted(os.listdir(tmp / name)) == ['predicted_t1ce.nii.gz']
