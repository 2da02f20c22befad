"""CPU: the host side of --brain_extract (mudiff_hip.volume_brain) and its numpy restatement
(tests/volume_brain_ref.py): the brute-force distance transform against scipy, the restatement's brain mask on the head phantom, the
flags, the choice of the source input, the place of the stage in volume_prepare.prepare_inputs, the [done] suffix and the report files."""
import json
import os

import numpy as np
import pytest

import volume_brain_ref as B
import volume_intake_ref as R
from volume_support import cli_argv


@pytest.mark.parametrize('spacing', [(1.0, 1.0, 1.0), (0.7, 1.3, 2.1)])
@pytest.mark.parametrize('shape', [(17, 13, 9), (5, 4, 3)])
def test_the_restatements_distance_is_scipys(shape, spacing):
    from scipy import ndimage
    rng = np.random.default_rng(shape[0])
    for density in (0.05, 0.5):
        mask = (rng.random(shape) < density).astype(np.uint8)
        mask[0, 0, 0] = 1
        mask[-1, -1, -1] = 0
        for value in (1, 0):
            got = np.sqrt(B.edt2(mask, value, spacing))
            want = ndimage.distance_transform_edt((mask != 0) != (value != 0), sampling=spacing)
            assert got.shape == shape and got.dtype == np.float64
            assert np.abs(got - want).max() <= 1e-12 * want.max()
    assert np.isinf(B.edt2(np.zeros(shape, np.uint8), 1, spacing)).all() and np.isinf(B.edt2(np.ones(shape, np.uint8), 0, spacing)).all()
    # the stated rounding order, on one voxel: a single member in the corner
    single = np.zeros(shape, np.uint8)
    single[0, 0, 0] = 1
    w = [np.float64(s) * np.float64(s) for s in spacing]
    p = tuple(s - 1 for s in shape)
    assert B.edt2(single, 1, spacing)[p] == ((w[0] * np.float64(p[0] * p[0])) + (w[1] * np.float64(p[1] * p[1]))) + (w[2] * np.float64(p[2] * p[2]))


@pytest.fixture(scope='module')
def head():
    return B.phantom()


def test_the_restatement_strips_the_phantom(head):
    """The geometry forces the outcome: the shell and the bridge erode away completely, the core survives, the regrowth stops short of
    the shell - at 1 mm and, on every second plane, at 1 x 1 x 2 mm."""
    values, labels = head
    assert values.shape == labels.shape == B.PHANTOM_SHAPE and values.dtype == np.float32
    assert all((labels == k).any() for k in range(6)) and int((labels == B.BRIDGE).sum()) == 12
    assert (values[labels == B.AIR] == 0).all() and (values[labels != B.AIR] > 0).all()
    for vol, lab, spacing in ((values, labels, (1.0, 1.0, 1.0)), (values[:, :, ::2], labels[:, :, ::2], (1.0, 1.0, 2.0))):
        mask, report, stages = B.brain_mask(vol, spacing=spacing, **B.PHANTOM_RADII)
        print(spacing, report)
        bright = (lab == B.BRAIN) | (lab == B.SCALP) | (lab == B.BRIDGE)
        assert np.array_equal(stages['tissue'], bright) and report['tissue'] == int(bright.sum())      # Otsu separates bright from dark
        assert not stages['eroded'][(lab == B.SCALP) | (lab == B.BRIDGE)].any() and stages['eroded'].any()
        assert report['components'] == 1 and report['core'] == report['eroded'] and np.array_equal(stages['core'], stages['eroded'])
        assert report['filled'] == int((lab == B.VENTRICLE).sum()) and report['kept'] == int(mask.sum())
        assert B.properties(mask, lab, spacing, B.PHANTOM_RADII['dilate_mm']) == dict(no_scalp=True, no_air=True, ventricle=True, bridge_cut=True,
                                                                                      short_of_scalp=True, brain=True)
        kept_holes = B.brain_mask(vol, spacing=spacing, keep_holes=True, **B.PHANTOM_RADII)[0]
        assert not kept_holes[lab == B.VENTRICLE].any() and np.array_equal(kept_holes, stages['grown'])
    # degenerate inputs leave no mask
    assert B.brain_mask(np.zeros((5, 4, 3), np.float32))[0] is None and B.brain_mask(np.full((5, 4, 3), 3.0, np.float32))[0] is None
    nothing, report, _ = B.brain_mask(values, erode_mm=40.0, dilate_mm=41.0)
    assert nothing is None and report['eroded'] == 0 and report['tissue'] > 0 and report['threshold'] is not None


def test_flags_defaults_and_refusals(capsys):
    from mudiff_hip import volume as V
    from mudiff_hip import volume_brain as VBR
    from mudiff_hip.volume_prepare import IntakeOptions
    args = V.build_argparser(cli_argv())
    assert args.brain_extract is False and args.brain_from is None and (args.brain_erode_mm, args.brain_dilate_mm, args.brain_bins) == (5.0, 6.0, 256)
    assert args.brain_keep_holes is False and args.brain_mask_out is False
    assert VBR.DEFAULTS == dict(bins=256, erode_mm=5.0, dilate_mm=6.0, keep_holes=False)
    # without the flag: the tuple it is today
    assert IntakeOptions.from_args(args).brain is None and IntakeOptions.from_args(args) == IntakeOptions('percentile', False, None, None, 80)
    assert IntakeOptions._fields[-1] == 'denoise' and IntakeOptions._fields.index('foreground') + 1 == IntakeOptions._fields.index('brain')
    assert IntakeOptions().brain is None
    assert IntakeOptions.from_args(V.build_argparser(cli_argv('--brain_extract'))).brain == dict(VBR.DEFAULTS, source=None, mask_out=False)
    args = V.build_argparser(cli_argv('--brain_extract', '--brain_from', 'T2', '--brain_erode_mm', '3', '--brain_dilate_mm', '4.5', '--brain_bins', '64',
                                   '--brain_keep_holes', '--brain_mask_out', '--foreground'))
    options = IntakeOptions.from_args(args)
    assert options.brain == dict(bins=64, erode_mm=3.0, dilate_mm=4.5, keep_holes=True, source='T2', mask_out=True) and options.foreground is not None
    assert IntakeOptions.from_args(V.build_argparser(cli_argv('--brain_erode_mm', '3'))).brain is None      # (the flag itself is missing)
    for bad, word in ((['--brain_bins', '15'], 'brain_bins'), (['--brain_bins', '1025'], 'brain_bins'), (['--brain_erode_mm', '0'], 'brain_erode_mm'),
                      (['--brain_erode_mm', 'nan'], 'brain_erode_mm'), (['--brain_dilate_mm', '4'], 'brain_dilate_mm'),
                      (['--brain_dilate_mm', 'inf'], 'brain_dilate_mm')):
        with pytest.raises(SystemExit):
            V.build_argparser(cli_argv('--brain_extract', *bad))
        assert word in capsys.readouterr().err
    nan, inf = float('nan'), float('inf')
    for kw, word in ((dict(bins=8), '--brain_bins'), (dict(bins=2048), '--brain_bins'), (dict(bins=64.5), '--brain_bins'),
                     (dict(erode_mm=0.0), '--brain_erode_mm'), (dict(erode_mm=-1.0), '--brain_erode_mm'), (dict(erode_mm=nan), '--brain_erode_mm'),
                     (dict(erode_mm=inf), '--brain_erode_mm'), (dict(dilate_mm=4.9), '--brain_dilate_mm'), (dict(dilate_mm=nan), '--brain_dilate_mm'),
                     (dict(dilate_mm=inf), '--brain_dilate_mm')):
        with pytest.raises(ValueError, match=word):
            VBR.check_options(**kw)
    VBR.check_options(bins=16, erode_mm=0.5, dilate_mm=0.5)
    VBR.check_options(bins=1024, erode_mm=5.0, dilate_mm=50.0, keep_holes=True)
    help_text = ' '.join(V.make_parser().format_help().split())
    assert 'morphological estimate, not a learned brain extraction' in help_text and '--brain_mask_out' in help_text
    from mudiff_hip import cohort
    assert cohort.build_argparser(cli_argv('--manifest', 'm.tsv', '--brain_extract', '--brain_erode_mm', '4')).brain_erode_mm == 4.0


def test_the_source_input():
    from mudiff_hip import volume_brain as VBR
    assert VBR.source_of(['FLAIR', 'T2', 'T1']) == 'T1' and VBR.source_of(['T1CE', 'T1', 'T2']) == 'T1'
    assert VBR.source_of(['FLAIR', 'T1CE', 'T2']) == 'T1CE' and VBR.source_of(['FLAIR', 'T2']) == 'FLAIR' and VBR.source_of(['T2', 'FLAIR']) == 'T2'
    assert VBR.source_of(['FLAIR', 'T2', 'T1'], 'T2') == 'T2' and VBR.source_of(['FLAIR', 'T2', 'T1'], 'flair') == 'FLAIR'
    with pytest.raises(ValueError, match='--brain_from T1CE'):
        VBR.source_of(['FLAIR', 'T2', 'T1'], 'T1CE')

    class Vol:
        header = None
        affine = np.array([[0.0, -0.9375, 0.0, 3.0], [0.9375, 0.0, 0.0, -2.0], [0.0, 0.0, 3.0, 1.0], [0.0, 0.0, 0.0, 1.0]])
    assert VBR.spacing_of(Vol) == (0.9375, 0.9375, 3.0) == B.spacing_of(Vol.affine)


class StandIn:
    def __init__(self, stage, source):
        self.stage, self.source = stage, source
        self.shape, self.affine, self.header = source.shape, source.affine, source.header


def test_prepare_inputs_masks_every_input_once_they_share_the_grid(tmp_path, monkeypatch):
    """One brain_mask call per subject, on the source input as it is after regrid and before any bias correction; the mask is applied to
    every input; the suffix and the report files are as stated; without the option nothing is called."""
    from mudiff_hip import volume as V, volume_bias as VB, volume_brain as VBR, volume_coreg as VC, volume_intake as VI, volume_regrid as VR
    from mudiff_hip.volume_prepare import IntakeOptions, IntakeReport, prepare_inputs
    rng = np.random.default_rng(4)
    names = ['FLAIR', 'T2', 'T1']
    raws = [VI.read_nifti_raw(R.write_nifti_typed(tmp_path / f'{m}.nii.gz', rng.integers(0, 50, (8, 8, 9)).astype(np.int16))) for m in names]
    calls = []
    device_mask = object()
    host = np.zeros((8, 8, 9), np.uint8, order='F')
    host[2:6, 2:6, 3:7] = 1

    def brain_mask(vol, device, **kw):
        calls.append(('brain_mask', vol, kw))
        return device_mask, dict(threshold=7.0, kept=64, source=None)

    def apply_mask(vol, mask, device):
        calls.append(('apply_mask', vol, mask))
        return StandIn('stripped', vol)

    def coregister(fixed, moving, device, **kw):
        calls.append(('coregister', fixed, moving))
        return np.eye(4), dict(params=[0.0] * 6, accepted=True)

    def regrid_to(raw, ref_shape, ref_affine, device, mode='linear', header=None, world=None):
        calls.append(('regrid_to', raw))
        return StandIn('regridded', raw)

    def correct(raw, device, **kw):
        calls.append(('correct', raw))
        return StandIn('corrected', raw), dict(iterations=[1])

    monkeypatch.setattr(VBR, 'brain_mask', brain_mask)
    monkeypatch.setattr(VBR, 'apply_mask', apply_mask)
    monkeypatch.setattr(VBR, 'host_mask', lambda mask: (calls.append(('host_mask', mask)), host)[1])
    monkeypatch.setattr(VC, 'coregister', coregister)
    monkeypatch.setattr(VR, 'regrid_to', regrid_to)
    monkeypatch.setattr(VB, 'correct', correct)
    brain = dict(VBR.DEFAULTS, source=None, mask_out=False)
    options = IntakeOptions(regrid=True, coreg=dict(strides=(4,)), bias=dict(VB.DEFAULTS, field=False), half_range=2, brain=brain)
    prepared, ref, report = prepare_inputs(list(zip(names, raws)), options, 'the device')
    assert [c[0] for c in calls] == ['coregister', 'regrid_to', 'coregister', 'regrid_to', 'brain_mask'] + ['apply_mask'] * 3 + ['correct'] * 3
    assert [c[0] for c in calls].count('brain_mask') == 1 and calls[4][2] == VBR.DEFAULTS      # (source / mask_out are the stage's own)
    assert calls[4][1].stage == 'regridded' and calls[4][1].source is raws[2]          # T1, on the grid, not corrected yet
    assert calls[5][1] is raws[0] and [c[1].stage for c in calls[6:8]] == ['regridded'] * 2 and all(c[2] is device_mask for c in calls[5:8])
    assert all(c[1].stage == 'stripped' for c in calls[8:]) and [p.stage for p in prepared] == ['corrected'] * 3
    assert [p.source.source.source for p in prepared[1:]] == raws[1:] and prepared[0].source.source is raws[0]
    assert ref[0] == raws[0].shape and ref[1] is raws[0].affine and ref[3:] == (2, 6)
    assert report.brain == [('T1', dict(threshold=7.0, kept=64, source='T1'), None)]
    assert report.suffix().startswith(' | regrid=T2,T1 | coreg=T2:') and report.suffix().endswith(' | bias=FLAIR,T2,T1 | brain=T1')
    report.write(str(tmp_path / 'out'), 'T1CE', np.eye(4), None)
    assert json.load(open(tmp_path / 'out' / 'brain_t1ce.json')) == dict(threshold=7.0, kept=64, source='T1')
    assert 'brain_t1ce_mask.nii.gz' not in os.listdir(tmp_path / 'out')
    # the flag alone, with --brain_from and --brain_mask_out: one mask from that input, every input stripped, the mask written on the grid
    del calls[:]
    grid = np.diag([0.9375, 0.9375, 3.0, 1.0])
    options = IntakeOptions(half_range=2, brain=dict(brain, source='FLAIR', mask_out=True, erode_mm=3.0))
    prepared, ref, report = prepare_inputs(list(zip(names, raws)), options, None)
    assert [c[0] for c in calls] == ['brain_mask', 'host_mask'] + ['apply_mask'] * 3 and calls[0][1] is raws[0] and calls[0][2]['erode_mm'] == 3.0
    assert [c[1] for c in calls[2:]] == raws and [p.source for p in prepared] == raws and report.suffix() == ' | brain=FLAIR'
    report.write(str(tmp_path / 'masked'), 'T1CE', grid, None)
    assert sorted(os.listdir(tmp_path / 'masked')) == ['brain_t1ce.json', 'brain_t1ce_mask.nii.gz']
    back, affine, _ = V.read_nifti(str(tmp_path / 'masked' / 'brain_t1ce_mask.nii.gz'))
    assert np.array_equal(np.asarray(back), host) and np.array_equal(np.asarray(affine)[:3], grid[:3])
    assert VI.read_nifti_raw(str(tmp_path / 'masked' / 'brain_t1ce_mask.nii.gz')).code == 2      # stored as uint8
    # a mask that could not be estimated: the inputs come back as they are, and the report says so
    del calls[:]
    monkeypatch.setattr(VBR, 'brain_mask', lambda vol, device, **kw: (calls.append(('brain_mask', vol, kw)), (None, dict(threshold=None, kept=0, source=None)))[1])
    prepared, ref, report = prepare_inputs(list(zip(names, raws)), options, None)
    assert [c[0] for c in calls] == ['brain_mask'] and prepared == raws and report.brain == [('FLAIR', dict(threshold=None, kept=0, source='FLAIR'), None)]
    # a --brain_from the subject does not have: refused before anything runs
    del calls[:]
    with pytest.raises(ValueError, match='--brain_from T1CE'):
        prepare_inputs(list(zip(names, raws)), IntakeOptions(half_range=2, regrid=True, brain=dict(brain, source='T1CE')), None)
    assert calls == []
    # without the option the stage is not called
    prepared, ref, report = prepare_inputs(list(zip(names, raws)), IntakeOptions(half_range=2), None)
    assert report.suffix() == '' and report.brain == [] and calls == [] and prepared == raws
    empty = IntakeReport()
    empty.write(str(tmp_path / 'none'), 'T1CE', np.eye(4), None)
    assert VBR.brain_suffix([]) == '' and VBR.brain_suffix(None) == '' and not os.path.exists(tmp_path / 'none')
