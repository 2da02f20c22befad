"""CPU: the host side of --conform / --antialias (mudiff_hip.volume_conform) against its numpy restatement
(tests/volume_conform_ref.py): the conform grid, the anti-aliasing rule, the restatement's own behaviour on stripes, the header, the
flags, and the place of the stage in prepare_inputs with the device stages replaced."""
import argparse
import json

import numpy as np
import pytest

import volume_conform_ref as CR
import volume_intake_ref as I
import volume_reorient_ref as R
from volume_support import raw_volume

BASE = ['--target_modality', 'T1CE', '--output_dir', 'o', '--exp', 'e']


def _centre(shape):
    return np.append((np.asarray(shape, np.float64) - 1) / 2, 1.0)


# ---------------------------------------------------------------------------------------------------
# the grid
# ---------------------------------------------------------------------------------------------------
def test_grid_centre_and_axes():
    from mudiff_hip import volume_conform as VCF, volume_reorient as VO
    first_shape = (176, 512, 300)
    firsts = {'oblique': R.rotation(0, 12.0) @ R.affine_of('RAS', first_shape, spacing=(1.0, 1.0, 1.0), origin=(-80.0, 30.0, 7.0)),
              'anisotropic': R.affine_of('RAS', first_shape, spacing=(0.5, 0.5, 5.0), origin=(3.0, -2.0, 7.5)),
              'sagittal': R.affine_of('PSL', first_shape, spacing=(0.45, 0.45, 1.2))}
    for name, world in firsts.items():
        shape, a = VCF.conform_grid(first_shape, world)
        assert shape == (240, 240, 155) and np.array_equal(a[:3, :3], np.diag([-1.0, -1.0, 1.0])) and np.array_equal(a[3], [0, 0, 0, 1]), name
        assert np.abs(a @ _centre(shape) - world @ _centre(first_shape)).max() <= 1e-9, name      # centre on centre, in mm
        assert VO.axcodes(a) == 'LPS' and VO.obliquity_deg(a) == 0.0
        want = CR.conform_grid(first_shape, world)[1]
        assert np.abs(a - want).max() <= 1e-9
    for code in VO.TARGETS:                              # all 48: axis-aligned, and the code reads back
        shape, a = VCF.conform_grid(first_shape, firsts['oblique'], shape=(24, 20, 16), spacing=(2.0, 1.5, 3.0), target=code)
        lin = a[:3, :3]
        assert ((lin != 0).sum(0) == 1).all() and ((lin != 0).sum(1) == 1).all() and VO.axcodes(a) == code, code
        assert np.array_equal(np.abs(lin).sum(0), [2.0, 1.5, 3.0]), code
        assert np.abs(a @ _centre(shape) - firsts['oblique'] @ _centre(first_shape)).max() <= 1e-9
        assert np.abs(a - CR.conform_grid(first_shape, firsts['oblique'], (24, 20, 16), (2.0, 1.5, 3.0), code)[1]).max() <= 1e-9
    assert VCF.conform_grid(first_shape, np.eye(4), spacing=2)[1][0, 0] == -2.0          # one value: all three axes
    for bad in (dict(shape=(0, 2, 2)), dict(shape=(2, 2)), dict(spacing=(1.0, -1.0, 1.0)), dict(spacing=(1.0, 1.0)), dict(spacing=0.0),
                dict(target='LLS')):
        with pytest.raises(ValueError):
            VCF.conform_grid(first_shape, np.eye(4), **bad)
    with pytest.raises(ValueError, match='finite'):
        VCF.conform_grid(first_shape, np.full((4, 4), np.nan))


def test_a_conform_grid_gives_back_its_own_affine():
    from mudiff_hip import volume_conform as VCF
    from mudiff_hip.volume_regrid import same_grid
    for shape, spacing, origin in (((240, 240, 155), (1.0, 1.0, 1.0), (119.3, 97.25, -64.7)), ((24, 24, 16), (2.0, 2.0, 2.0), (22.1, 25.9, -13.3))):
        own = R.affine_of('LPS', shape, spacing, origin).astype(np.float32).astype(np.float64)      # what a header stores
        got_shape, got = VCF.conform_grid(shape, own, shape=shape, spacing=spacing)
        assert np.array_equal(got.astype(np.float32), own.astype(np.float32)) and same_grid(shape, own, got_shape, got)


# ---------------------------------------------------------------------------------------------------
# the rule
# ---------------------------------------------------------------------------------------------------
def test_rule():
    from mudiff_hip import volume_conform as VCF
    from mudiff_hip.volume_regrid import grid_matrix
    assert VCF.sigma_of(1.0) == 0.0 and VCF.sigma_of(0.5) == 0.0 and VCF.weights(0.0) is None
    table = {1.25: 1, 2: 3, 2.5: 3, 3: 4, 5: 7, 8: 11}
    for f, r in table.items():
        s = VCF.sigma_of(f)
        assert VCF.radius(s) == r == CR.radius(CR.sigma(f)) and abs(s - CR.sigma(f)) <= 1e-15 * s
        assert abs(s * 2 * np.sqrt(2 * np.log(2)) - np.sqrt(f * f - 1)) <= 1e-12                  # the FWHM in quadrature
        w = VCF.weights(s)
        assert w.dtype == np.float64 and w.size == 2 * r + 1 and w[r] == 1.0 and np.array_equal(w, w[::-1]) and np.array_equal(w, CR.weights(s))
    shape = (40, 40, 40)
    src = R.affine_of('RAS', shape, origin=(-19.5, -19.5, -19.5))                              # the grid centre at the world origin
    for axis in range(3):                                # a rotation about the grid centre at equal spacing: nothing is filtered
        M = grid_matrix(src, R.rotation(axis, 12.0) @ src)
        assert VCF.sigmas(M) == [0.0, 0.0, 0.0] and VCF.lowpass_plan(M)['weights'] == [None, None, None]
        assert VCF.lowpass_plan(M)['radii'] == [0, 0, 0]
    # a permuted axis-aligned M: reference axes (x, y, z) step 3 / 1 / 2 voxels along SOURCE axes (z, x, y)
    src = R.affine_of('RAS', shape, spacing=(1.0, 1.0, 1.0))
    ref = R.affine_of('ASR', shape, spacing=(1.0, 2.0, 3.0))
    M = grid_matrix(src, ref)
    assert np.allclose(VCF.factors(M), [3.0, 1.0, 2.0]) and np.allclose(VCF.factors(M), CR.factors(M))
    plan = VCF.lowpass_plan(M)
    assert plan['radii'] == [4, 0, 3] and plan['weights'][1] is None and plan['sigmas'][1] == 0.0
    assert np.allclose(VCF.factors(grid_matrix(R.affine_of('RAS', shape, spacing=(0.5, 0.5, 2.0)), R.affine_of('LPS', shape))), [2.0, 2.0, 0.5])
    with pytest.raises(ValueError, match=r'T2\.nii.*axis y.*radius of 17'):
        VCF.lowpass_plan(np.diag([1.0, 13.0, 1.0, 1.0]), 'T2.nii')
    assert VCF.lowpass_plan(np.diag([1.0, 12.0, 1.0, 1.0]))['radii'] == [0, 16, 0] and VCF.MAX_RADIUS == 16


def test_restatement_on_stripes():
    """Period-2 stripes 0 / 200 sampled at every second voxel: exactly 0 unfiltered, within 13.86 of the mean 100 behind the filter for
    f = 2 (the weights give 200 * 0.7941 / 1.8437 = 86.147 at an even voxel: 13.853 off)."""
    v = CR.stripes((64, 5, 4))
    assert np.array_equal(v[::2], np.zeros((32, 5, 4))) and np.array_equal(np.unique(v), [0.0, 200.0])
    w = CR.weights(CR.sigma(2.0))
    low, bad = CR.lowpass(v, [w, None, None])
    assert bad == 0 and low.dtype == np.float32
    from mudiff_hip import volume_conform as VCF
    plan = VCF.lowpass_plan(np.diag([2.0, 1.0, 1.0, 1.0]))                                         # the package's rule on this case: the same filter
    assert plan['radii'] == [3, 0, 0] and np.array_equal(CR.lowpass(v, plan['weights'])[0], low)
    interior = low[3:-3]
    assert float(np.abs(interior - 100.0).max()) <= 13.86 and float(np.abs(interior - 100.0).max()) >= 13.8
    assert float(np.abs(low[::2][2:-2] - 100.0).max()) <= 13.86                                  # what sampling at even indices now reads
    # the properties of one pass: a constant stays, zeros wider than R stay exactly 0, the range is kept
    const, _ = CR.lowpass(np.full((9, 8, 7), 37.25, np.float32), [w, w, w])
    assert np.abs(const - np.float32(37.25)).max() <= np.spacing(np.float32(37.25))
    z = v.copy()
    z[20:40] = 0
    low, _ = CR.lowpass(z, [w, None, None])
    assert np.array_equal(low[23:37], np.zeros((14, 5, 4))) and low.min() >= 0.0 and low.max() <= 200.0


# ---------------------------------------------------------------------------------------------------
# the header
# ---------------------------------------------------------------------------------------------------
def test_conformed_header_round_trips(tmp_path):
    from mudiff_hip import volume as V, volume_conform as VCF
    first = np.asfortranarray(np.arange(5 * 4 * 3, dtype='<i2').reshape((5, 4, 3), order='F'))
    world = R.rotation(1, 12.0) @ R.affine_of('RAS', first.shape, spacing=(0.5, 0.5, 5.0), origin=(1.0, 2.0, 3.0))
    path = I.write_nifti_typed(tmp_path / 'first.nii.gz', first, slope=0.25, inter=-3.0, affine=world)
    like = V.open_nifti1(path)[1]
    shape, a = VCF.conform_grid(first.shape, like.world_affine, shape=(6, 7, 8), spacing=(2.0, 1.5, 3.0))
    hdr = VCF.conformed_header(shape, a, like)
    assert isinstance(hdr, V.NiftiHeader) and hdr.endian == '<' and len(hdr.raw) == 348
    assert hdr.shape == shape and hdr._get('8h', 40) == (3, 6, 7, 8, 1, 1, 1, 1) and hdr._get('8f', 76)[1:4] == (2.0, 1.5, 3.0)
    assert hdr._get('h', 70)[0] == 16 and hdr._get('h', 72)[0] == 32 and hdr._get('2f', 112) == (1.0, 0.0)
    assert hdr._get('h', 252)[0] == 0 and hdr._get('h', 254)[0] == 1
    assert np.array_equal(hdr.world_affine, a.astype(np.float32).astype(np.float64)) and np.array_equal(hdr.affine, hdr.world_affine)
    assert hdr.raw[148:228] == like.raw[148:228] and hdr.raw[123] == like.raw[123]               # descriptive fields: the first input's
    vol = np.asfortranarray(np.random.default_rng(0).random(shape).astype(np.float32))
    out = str(tmp_path / 'out.nii.gz')
    V.write_nifti(out, vol, hdr.affine, hdr)
    _, back, code = V.open_nifti1(out)
    assert code == 16 and back.raw == hdr.raw                                                    # reused as it is: nothing left to fix up
    got, got_affine, _ = V.read_nifti(out)
    assert np.array_equal(got, vol) and np.array_equal(got_affine, hdr.affine)
    blank = VCF.conformed_header(shape, a, None)
    assert blank.shape == shape and np.array_equal(blank.world_affine, hdr.world_affine) and blank._get('8f', 76)[0] == 1.0


# ---------------------------------------------------------------------------------------------------
# flags and options
# ---------------------------------------------------------------------------------------------------
def test_flags_and_options(capsys):
    from mudiff_hip import cohort, volume as V
    from mudiff_hip.volume_prepare import IntakeOptions
    args = V.build_argparser(BASE)
    assert (args.conform, args.conform_shape, args.conform_spacing, args.conform_to, args.conform_back, args.antialias) == \
        (False, [240, 240, 155], [1.0, 1.0, 1.0], 'LPS', False, None)
    # the four pinned properties of IntakeOptions
    assert IntakeOptions._fields[-1] == 'denoise' and IntakeOptions._fields[:5] == ('norm', 'regrid', 'coreg', 'bias', 'half_range')
    assert IntakeOptions._fields.index('brain') == IntakeOptions._fields.index('foreground') + 1
    assert IntakeOptions.from_args(args) == IntakeOptions('percentile', False, None, None, 80)
    f = IntakeOptions._fields
    assert f.index('reorient') < f.index('conform') < f.index('antialias') < f.index('denoise')
    assert IntakeOptions().conform is None and IntakeOptions().antialias is False
    on = IntakeOptions.from_args(V.build_argparser(BASE + ['--conform']))
    assert on.conform == dict(shape=(240, 240, 155), spacing=(1.0, 1.0, 1.0), target='LPS') and on.antialias is True and on.regrid is False
    o = IntakeOptions.from_args(V.build_argparser(BASE + ['--conform', '--conform_shape', '24', '24', '16', '--conform_spacing', '2', '--conform_to',
                                                          'ras', '--antialias', 'off', '--conform_back']))
    assert o.conform == dict(shape=(24, 24, 16), spacing=(2.0, 2.0, 2.0), target='RAS') and o.antialias is False
    assert IntakeOptions.from_args(V.build_argparser(BASE + ['--conform', '--conform_spacing', '0.5', '0.5', '2'])).conform['spacing'] == (0.5, 0.5, 2.0)
    alone = IntakeOptions.from_args(V.build_argparser(BASE + ['--regrid', '--antialias', 'on']))
    assert alone.antialias is True and alone.conform is None
    assert IntakeOptions.from_args(argparse.Namespace(conform=True)).conform == on.conform        # the defaults live in from_args
    assert IntakeOptions.from_args(argparse.Namespace(conform=True)).antialias is True
    for bad in (['--conform_back'], ['--conform', '--conform_shape', '24', '0', '16'], ['--conform', '--conform_shape', '-1', '4', '4'],
                ['--conform', '--conform_spacing', '0'], ['--conform', '--conform_spacing', '1', '-2', '1'], ['--conform', '--conform_spacing', '1', '2'],
                ['--conform', '--conform_to', 'LLS'], ['--conform', '--conform_to', 'RAS', '--reorient', '--reorient_to', 'LPS'],
                ['--antialias', 'maybe']):
        with pytest.raises(SystemExit):
            V.build_argparser(BASE + bad)
    capsys.readouterr()
    follows = V.build_argparser(BASE + ['--conform', '--conform_to', 'RAS', '--reorient'])          # --reorient_to not given: it follows
    assert follows.reorient_to == 'RAS' and V.build_argparser(BASE + ['--reorient']).reorient_to == 'LPS'
    assert V.build_argparser(BASE + ['--conform', '--conform_to', 'RAS', '--reorient', '--reorient_to', 'ras']).conform_to == 'RAS'
    assert cohort.build_argparser(BASE + ['--manifest', 'm.tsv', '--conform', '--conform_back']).conform_back
    helps = V.make_parser().format_help()
    assert '--antialias' in helps and helps.count('untuned') >= 2


# ---------------------------------------------------------------------------------------------------
# prepare_inputs with the device stages replaced
# ---------------------------------------------------------------------------------------------------
def _raw(vol, affine):
    return raw_volume(np.asarray(vol, np.int16), affine=np.asarray(affine, np.float64))


GRID = dict(shape=(6, 5, 8), spacing=(2.0, 2.0, 2.0), target='LPS')


def _spy(monkeypatch, calls):
    """volume_regrid.regrid_to and volume_coreg.coregister replaced: the calls are recorded, the grid logic (same_grid) is kept."""
    from mudiff_hip import volume_coreg as VC, volume_regrid as VR

    def regrid_to(raw, ref_shape, ref_affine, device, mode='linear', header=None, world=None, found=None, antialias=False, name=None):
        calls.append(('regrid_to', name, tuple(ref_shape), np.array(ref_affine), mode, header, world, antialias))
        moved = world is not None and not np.array_equal(world, np.eye(4))
        if not moved and VR.same_grid(raw.shape, VR.world_affine_of(raw.affine, raw.header), ref_shape, ref_affine):
            return raw
        if found is not None and antialias:
            found.update(lowpass=True, nonfinite=2)
        return VR.RegriddedVolume(None, ref_shape, np.asarray(ref_affine, np.float64), header)

    def coregister(first, raw, device, **kw):
        calls.append(('coregister', first, raw))
        w = np.eye(4)
        w[0, 3] = 1.5
        return w, dict(found=True)
    monkeypatch.setattr(VR, 'regrid_to', regrid_to)
    monkeypatch.setattr(VC, 'coregister', coregister)
    monkeypatch.setattr(VC, 'coreg_suffix', lambda entries: '')


def test_prepare_inputs_conforms_every_input(monkeypatch, tmp_path):
    from mudiff_hip import volume_conform as VCF, volume_prepare as VP
    calls = []
    _spy(monkeypatch, calls)
    first = _raw(np.zeros((12, 10, 4)), R.rotation(0, 12.0) @ R.affine_of('RAS', (12, 10, 4), spacing=(1.0, 1.0, 4.0), origin=(-5.0, 3.0, 2.0)))
    later = _raw(np.zeros((24, 20, 16)), R.affine_of('RAS', (24, 20, 16), spacing=(0.5, 0.5, 1.0), origin=(-5.0, 3.0, 2.0)))
    named = [('FLAIR', first), ('T2', later), ('T1', later)]
    options = VP.IntakeOptions(half_range=2, coreg=dict(strides=(1,), max_mm=1.0, max_deg=1.0), conform=dict(GRID), antialias=True)
    prepared, ref, report = VP.prepare_inputs(named, options, 'cpu', labels={'FLAIR': 'flair.nii'})
    want_shape, want_affine = CR.conform_grid(first.shape, first.affine, **GRID)
    assert ref[0] == want_shape and np.abs(ref[1] - want_affine).max() <= 1e-9 and ref[3:] == (2, 6)         # the slab of the conform Z
    assert ref[2].shape == want_shape and np.array_equal(ref[2].world_affine, ref[1].astype(np.float32).astype(np.float64))
    # the order: register each later input against the UNRESAMPLED first one, then one regrid_to per input, the first included
    assert [c[0] for c in calls] == ['regrid_to', 'coregister', 'regrid_to', 'coregister', 'regrid_to']
    assert all(c[1] is first and c[2] is later for c in calls if c[0] == 'coregister')
    regrids = [c for c in calls if c[0] == 'regrid_to']
    assert [c[1] for c in regrids] == ['flair.nii', 'T2', 'T1']
    assert regrids[0][6] is None and all(c[6] is not None and c[6][0, 3] == 1.5 for c in regrids[1:])         # `world` only on the later ones
    assert all(c[2] == want_shape and np.array_equal(c[3], ref[1]) and c[4] == 'linear' and c[5] is ref[2] and c[7] is True for c in regrids)
    assert all(v.shape == want_shape for v in prepared) and report.regridded == []
    assert report.suffix() == ' | conform=6x5x8@2mm:FLAIR,T2,T1 | antialias=on' and report.nonfinite == 6
    assert [n for n, _ in report.conform] == ['FLAIR', 'T2', 'T1']
    e = dict(report.conform)
    assert set(e['FLAIR']) == {'shape_from', 'spacing_from', 'obliquity_deg', 'factors', 'sigmas', 'radii', 'resampled', 'nonfinite'}
    assert e['FLAIR']['shape_from'] == [12, 10, 4] and np.allclose(e['FLAIR']['spacing_from'], [1.0, 1.0, 4.0]) and e['FLAIR']['resampled'] is True
    assert abs(e['FLAIR']['obliquity_deg'] - 12.0) <= 1e-9 and e['T2']['obliquity_deg'] == 0.0
    assert np.allclose(e['T2']['factors'], [4.0, 4.0, 2.0]) and e['T2']['radii'] == [5, 5, 3] and e['T2']['nonfinite'] == 2
    assert e['FLAIR']['radii'][2] == 0 and e['FLAIR']['factors'][2] < 1                                       # 4 mm -> 2 mm: upsampled, unfiltered
    report.write(str(tmp_path), 'T1CE', ref[1], ref[2])
    assert sorted(f.name for f in tmp_path.iterdir()) == ['conform_t1ce.json', 'coreg_t1ce.json']
    written = json.load(open(tmp_path / 'conform_t1ce.json'))
    assert written == {'grid': '6x5x8@2mm', 'inputs': {k: v for k, v in report.conform}}
    assert VCF.grid_name((240, 240, 155), (1.0, 1.0, 1.0)) == '240x240x155@1mm' and VCF.grid_name((4, 4, 4), (0.5, 0.5, 2.0)) == '4x4x4@0.5x0.5x2mm'
    # --antialias off: the same calls without the filter, and the line does not claim one
    calls.clear()
    _, _, report = VP.prepare_inputs(named[:2], options._replace(antialias=False, coreg=None, interp='cubic'), 'cpu')
    assert [c[0] for c in calls] == ['regrid_to', 'regrid_to'] and all(c[7] is False and c[4] == 'cubic' and c[6] is None for c in calls)
    assert report.suffix() == ' | interp=cubic | conform=6x5x8@2mm:FLAIR,T2' and dict(report.conform)['T2']['radii'] == [0, 0, 0]


def test_prepare_inputs_leaves_an_input_on_the_grid_untouched(monkeypatch):
    from mudiff_hip import volume_prepare as VP
    calls = []
    _spy(monkeypatch, calls)
    own = R.affine_of('LPS', GRID['shape'], GRID['spacing'], origin=(5.0, 4.0, -7.0))
    first, later = _raw(np.zeros(GRID['shape']), own), _raw(np.zeros((12, 10, 16)), R.affine_of('LPS', (12, 10, 16), origin=(5.5, 4.5, -7.5)))
    prepared, ref, report = VP.prepare_inputs([('FLAIR', first), ('T2', later)], VP.IntakeOptions(half_range=2, conform=dict(GRID), antialias=True), 'cpu')
    assert prepared[0] is first and prepared[1] is not later and ref[0] == GRID['shape']
    assert np.array_equal(ref[1].astype(np.float32), own.astype(np.float32))
    assert report.suffix() == ' | conform=6x5x8@2mm:T2 | antialias=on'
    assert dict(report.conform)['FLAIR']['resampled'] is False and dict(report.conform)['FLAIR']['radii'] == [0, 0, 0]


def test_without_the_flags_nothing_new_runs(monkeypatch, tmp_path):
    from mudiff_hip import volume_prepare as VP
    calls = []
    _spy(monkeypatch, calls)
    a = _raw(np.zeros((6, 5, 8)), np.eye(4))
    prepared, ref, report = VP.prepare_inputs([('FLAIR', a), ('T2', a), ('T1', a)], VP.IntakeOptions(half_range=2), 'cpu')
    assert calls == [] and all(v is a for v in prepared) and ref[0] == (6, 5, 8) and ref[1] is a.affine
    assert report.suffix() == '' and report.conform == [] and report.lowpass is False
    report.write(str(tmp_path), 'T1CE', ref[1], ref[2])
    assert list(tmp_path.iterdir()) == []
    # --regrid alone calls regrid_to exactly as it did: positionally the same, no antialias, no name
    b = _raw(np.zeros((6, 5, 8)), np.diag([2.0, 2.0, 2.0, 1.0]))
    _, _, report = VP.prepare_inputs([('FLAIR', a), ('T2', b)], VP.IntakeOptions(half_range=2, regrid=True), 'cpu')
    assert [(c[0], c[1], c[7]) for c in calls] == [('regrid_to', None, False)] and report.suffix() == ' | regrid=T2'
    # --regrid --antialias on: the later input is filtered, and the line says so
    calls.clear()
    _, _, report = VP.prepare_inputs([('FLAIR', a), ('T2', b)], VP.IntakeOptions(half_range=2, regrid=True, antialias=True), 'cpu')
    assert [(c[0], c[1], c[7]) for c in calls] == [('regrid_to', 'T2', True)] and report.suffix() == ' | regrid=T2 | antialias=on'


def test_conform_back_wraps_the_writer(monkeypatch):
    from mudiff_hip import volume_conform as VCF, volume_regrid as VR
    seen = []
    first = _raw(np.zeros((12, 10, 4)), np.diag([1.0, 1.0, 4.0, 1.0]))
    first.header = 'the original header'
    grid_shape, grid_affine = VCF.conform_grid(first.shape, first.affine, **GRID)
    back = np.asfortranarray(np.arange(480, dtype=np.float32).reshape(first.shape, order='F'))

    def regrid_to(raw, ref_shape, ref_affine, device, mode='linear', header=None, world=None, found=None, antialias=False, name=None):
        seen.append((raw.shape, np.array(raw.affine), raw.code, tuple(ref_shape), np.array(ref_affine), mode, antialias))
        out = VR.RegriddedVolume(None, ref_shape, ref_affine, header)
        out.data = back.reshape(-1, order='F')
        return out
    monkeypatch.setattr(VR, 'regrid_to', regrid_to)
    calls = []
    write = VCF.write_back(lambda *a: calls.append(a), first, grid_shape, grid_affine, 'cpu', interp='cubic', antialias=True)
    write('p.nii.gz', np.zeros(grid_shape, np.float32), grid_affine, None)
    (path, vol, aff, hdr), = calls
    assert path == 'p.nii.gz' and vol.shape == first.shape and np.array_equal(vol, back) and aff is first.affine and hdr == 'the original header'
    (src_shape, src_affine, code, to_shape, to_affine, mode, antialias), = seen
    assert src_shape == grid_shape and np.array_equal(src_affine, grid_affine) and code == 16 and to_shape == first.shape
    assert np.array_equal(to_affine, first.affine) and mode == 'cubic' and antialias is True
