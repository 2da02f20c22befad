"""CPU: the host side of --foreground (mudiff_hip.volume_foreground) and its numpy restatement
(tests/volume_foreground_ref.py): the Otsu scan, the flags, the place of the stage in volume_prepare.prepare_inputs, the [done] suffix and
the report file, the restatement's labelling against scipy.ndimage.label on the adversarial masks, and the recovery of the phantom's head
by the restatement alone."""
import json
import os

import numpy as np
import pytest

import volume_foreground_ref as F
import volume_intake_ref as R
from volume_support import cli_argv

LABEL_SHAPES = ((37, 29, 23), (5, 4, 3), (70, 19, 11))


def test_otsu_bin_is_the_brute_force_scan():
    from mudiff_hip import volume_foreground as VF
    rng = np.random.default_rng(2)
    bimodal = np.zeros(256, np.int64)
    bimodal[10:60] = rng.integers(50, 500, 50)
    bimodal[150:240] = rng.integers(20, 300, 90)
    assert VF.otsu_bin(bimodal) == F.otsu(bimodal) and 59 <= VF.otsu_bin(bimodal) < 150
    for bins in (16, 64, 1024):
        for _ in range(5):
            c = rng.integers(0, 1000, bins) * (rng.random(bins) < 0.6)
            assert VF.otsu_bin(c) == F.otsu(c)
    # a tie: two bins far apart, every k between them separates them equally well - the first one wins
    tie = np.zeros(32, np.int64)
    tie[3], tie[20] = 7, 7
    assert VF.otsu_bin(tie) == F.otsu(tie) == 3
    # the last bin is never a threshold; one non-empty bin (or none) gives None
    two = np.zeros(16, np.int64)
    two[14], two[15] = 4, 9
    assert VF.otsu_bin(two) == F.otsu(two) == 14
    for k in (0, 5, 15):
        one = np.zeros(16, np.int64)
        one[k] = 11
        assert VF.otsu_bin(one) is None and F.otsu(one) is None
    assert VF.otsu_bin(np.zeros(16, np.int64)) is None
    # the keys of mud_volume_fg_range
    for v in (0.5, -0.5, 3.0e38, -3.0e38, 1e-45, 750.43878):
        bits = int(np.float32(v).view(np.uint32))
        key = (~bits & 0xFFFFFFFF) if bits & 0x80000000 else bits | 0x80000000
        assert VF.unkey(key) == float(np.float32(v)) and VF.unkey(~(~key & 0xFFFFFFFF)) == float(np.float32(v))


def test_flags_defaults_and_refusals(capsys):
    from mudiff_hip import volume as V
    from mudiff_hip import volume_foreground as VF
    from mudiff_hip.volume_prepare import IntakeOptions
    args = V.build_argparser(cli_argv())
    assert args.foreground is False and args.foreground_bins == 256 and args.foreground_open == 0
    assert args.foreground_keep_holes is False and args.foreground_mask_out is False
    assert VF.DEFAULTS == dict(bins=256, open=0, keep_holes=False, mask_out=False)
    # without the flag: the tuple it is today
    assert IntakeOptions.from_args(args).foreground is None and IntakeOptions.from_args(args) == IntakeOptions('percentile', False, None, None, 80)
    assert 'foreground' in IntakeOptions._fields and IntakeOptions().foreground is None and IntakeOptions().denoise is None
    assert IntakeOptions.from_args(V.build_argparser(cli_argv('--foreground'))).foreground == VF.DEFAULTS
    args = V.build_argparser(cli_argv('--foreground', '--foreground_bins', '64', '--foreground_open', '2', '--foreground_keep_holes',
                                   '--foreground_mask_out', '--denoise'))
    options = IntakeOptions.from_args(args)
    assert options.foreground == dict(bins=64, open=2, keep_holes=True, mask_out=True) and options.denoise is not None
    assert IntakeOptions.from_args(V.build_argparser(cli_argv('--foreground_bins', '64'))).foreground is None      # (the flag itself is missing)
    for bad, word in ((['--foreground_bins', '15'], 'foreground_bins'), (['--foreground_bins', '1025'], 'foreground_bins'),
                      (['--foreground_open', '-1'], 'foreground_open'), (['--foreground_open', '4'], 'foreground_open')):
        with pytest.raises(SystemExit):
            V.build_argparser(cli_argv('--foreground', *bad))
        assert word in capsys.readouterr().err
    for kw, word in ((dict(bins=8), '--foreground_bins'), (dict(bins=2048), '--foreground_bins'), (dict(bins=64.5), '--foreground_bins'),
                     (dict(open=4), '--foreground_open'), (dict(open=-1), '--foreground_open')):
        with pytest.raises(ValueError, match=word):
            VF.check_options(**kw)
    VF.check_options(bins=16, open=3)
    VF.check_options(bins=1024, open=0, keep_holes=True, mask_out=True)
    help_text = ' '.join(V.make_parser().format_help().split())
    assert 'NOT a brain extraction' in help_text
    from mudiff_hip import cohort
    assert cohort.build_argparser(cli_argv('--manifest', 'm.tsv', '--foreground', '--foreground_open', '1')).foreground_open == 1


def test_foreground_suffix_and_reports(tmp_path):
    from mudiff_hip import volume as V, volume_foreground as VF
    from mudiff_hip.volume_prepare import IntakeReport
    assert VF.foreground_suffix([]) == '' and VF.foreground_suffix(None) == ''

    class Masked:
        def __init__(self, mask, affine):
            self.mask, self.affine, self.header = mask, affine, None

    mask = np.zeros((5, 4, 3), np.uint8, order='F')
    mask[1:4, 1:3, 1] = 1
    own = np.diag([2.0, 2.0, 3.0, 1.0])
    reports = [('FLAIR', dict(threshold=258.2, bin=87, bins=256, kept=6925), Masked(mask, own)), ('T2', dict(threshold=None, bin=None, bins=256, kept=0), None)]
    assert VF.foreground_suffix(reports) == ' | foreground=FLAIR,T2'
    path = VF.write_reports(reports, str(tmp_path / 'o'), 'T1CE', np.eye(4), None)
    assert os.path.basename(path) == 'foreground_t1ce.json' and json.load(open(path)) == {r[0]: r[1] for r in reports}
    assert sorted(os.listdir(tmp_path / 'o')) == ['foreground_t1ce.json', 'foreground_t1ce_flair.nii.gz']
    back, affine, _ = V.read_nifti(str(tmp_path / 'o' / 'foreground_t1ce_flair.nii.gz'))
    assert np.array_equal(np.asarray(back), mask) and np.array_equal(np.asarray(affine)[:3], own[:3])      # on the input's own grid
    from mudiff_hip import volume_intake as VI
    assert VI.read_nifti_raw(str(tmp_path / 'o' / 'foreground_t1ce_flair.nii.gz')).code == 2              # stored as uint8
    report = IntakeReport()
    assert report.foreground == [] and report.suffix() == ''
    report.foreground += [r[:2] + (None,) for r in reports]
    report.denoise.append(('FLAIR', dict(sigma=3.0)))
    report.bias.append(('FLAIR', dict(iterations=[1]), None))
    assert report.suffix() == ' | bias=FLAIR | denoise=FLAIR | foreground=FLAIR,T2'
    report.write(str(tmp_path / 'p'), 'T1CE', np.eye(4), None)
    assert sorted(os.listdir(tmp_path / 'p')) == ['bias_t1ce.json', 'denoise_t1ce.json', 'foreground_t1ce.json']


class StandIn:
    def __init__(self, stage, source):
        self.stage, self.source = stage, source
        self.shape, self.affine, self.header = source.shape, source.affine, source.header


def test_prepare_inputs_masks_every_input_after_the_denoising(tmp_path, monkeypatch):
    """denoise, then foreground, for every input (the first included) before coregister sees any; `ref` is the first input's geometry;
    the suffix and foreground_<t>.json are as stated."""
    from mudiff_hip import volume_bias as VB, volume_coreg as VC, volume_denoise as VD, volume_foreground as VF, volume_intake as VI
    from mudiff_hip import volume_regrid as VR
    from mudiff_hip.volume_prepare import IntakeOptions, prepare_inputs
    rng = np.random.default_rng(4)
    names = ['FLAIR', 'T2', 'T1']
    raws = [VI.read_nifti_raw(R.write_nifti_typed(tmp_path / f'{m}.nii.gz', rng.integers(0, 50, (8, 8, 9)).astype(np.int16))) for m in names]
    calls = []

    def denoise(raw, device, **kw):
        calls.append(('denoise', raw, kw))
        return StandIn('denoised', raw), dict(sigma=1.0)

    def foreground(raw, device, **kw):
        calls.append(('foreground', raw, kw))
        return StandIn('masked', raw), dict(threshold=float(len(calls)), bin=3)

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
    monkeypatch.setattr(VF, 'foreground', foreground)
    monkeypatch.setattr(VC, 'coregister', coregister)
    monkeypatch.setattr(VR, 'regrid_to', regrid_to)
    monkeypatch.setattr(VB, 'correct', correct)
    options = IntakeOptions(regrid=True, coreg=dict(strides=(4,)), bias=dict(VB.DEFAULTS, field=False), half_range=2, denoise=dict(VD.DEFAULTS),
                            foreground=dict(VF.DEFAULTS))
    prepared, ref, report = prepare_inputs(list(zip(names, raws)), options, 'the device')
    assert [c[0] for c in calls] == ['denoise'] * 3 + ['foreground'] * 3 + ['correct', 'coregister', 'regrid_to', 'correct', 'coregister',
                                                                             'regrid_to', 'correct']
    assert [c[1].source for c in calls[3:6]] == raws and all(c[1].stage == 'denoised' and c[2] == VF.DEFAULTS for c in calls[3:6])
    assert ref[0] == raws[0].shape and ref[1] is raws[0].affine and ref[2] is raws[0].header and ref[3:] == (2, 6)
    first = calls[6][1]                                                                # the first input: denoised, masked, then corrected only
    assert first.stage == 'masked' and first.source.stage == 'denoised' and first.source.source is raws[0]
    for k in (7, 10):
        co, re, bi = calls[k:k + 3]
        assert co[1] is first and co[2].stage == 'masked' and re[1] is co[2] and bi[1].stage == 'regridded'
    assert [r[0] for r in report.foreground] == names and [r[1]['threshold'] for r in report.foreground] == [4.0, 5.0, 6.0]
    assert all(r[2] is None for r in report.foreground)                                # (no --foreground_mask_out: no volume is kept)
    assert report.suffix().startswith(' | regrid=T2,T1 | coreg=T2:') and report.suffix().endswith(' | bias=FLAIR,T2,T1 | denoise=FLAIR,T2,T1 | foreground=FLAIR,T2,T1')
    report.write(str(tmp_path / 'out'), 'T1CE', np.eye(4), None)
    assert json.load(open(tmp_path / 'out' / 'foreground_t1ce.json')) == {n: dict(threshold=4.0 + i, bin=3) for i, n in enumerate(names)}
    # the flag alone: the masked files come back in order, nothing else runs; an input left untouched is reported all the same
    del calls[:]
    monkeypatch.setattr(VF, 'foreground', lambda raw, device, **kw: (calls.append(('foreground', raw, kw)), (raw, dict(threshold=None)))[1])
    prepared, ref, report = prepare_inputs(list(zip(names, raws)), IntakeOptions(half_range=2, foreground=dict(VF.DEFAULTS, mask_out=True)), None)
    assert [c[0] for c in calls] == ['foreground'] * 3 and prepared == raws and report.suffix() == ' | foreground=FLAIR,T2,T1'
    assert all(r[2] is None for r in report.foreground)
    # without the flag the stage is not called
    del calls[:]
    assert prepare_inputs(list(zip(names, raws)), IntakeOptions(half_range=2), None)[2].suffix() == '' and calls == []


@pytest.mark.parametrize('shape', LABEL_SHAPES)
def test_the_restatements_labelling_is_scipys(shape):
    from scipy import ndimage
    masks = F.label_masks(shape)
    assert list(masks) == ['on', 'off', 'single', 'checker', 'serpentine', 'comb', 'random0.3', 'random0.5', 'random0.7']
    for name, mask in masks.items():
        for value in (1, 0):
            lab = F.label(mask, value)
            member = (mask != 0) == (value != 0)
            assert lab.dtype == np.int32 and np.array_equal(lab >= 0, member)
            assert np.array_equal(lab, F.canonical(ndimage.label(member)[0])), (name, value)
    n = int(np.prod(shape))
    counts, face, winner, components = F.census(F.label(masks['checker'], 1))
    assert components == (n + 1) // 2 and winner == 0 and counts.max() == 1            # every voxel its own component: the tie goes to index 0
    assert F.census(F.label(masks['serpentine'], 1))[2:] == (0, 1) and F.census(F.label(masks['on'], 1))[0][0] == n
    assert F.census(F.label(masks['off'], 1))[2:] == (None, 0)
    if shape[2] > 3:
        assert F.census(F.label(masks['comb'], 1))[3] == 1 and F.census(F.label(masks['comb'][:, :, :-1], 1))[3] == ((shape[0] + 1) // 2) * ((shape[1] + 1) // 2)


def test_morphology_of_the_restatement_is_scipys():
    from scipy import ndimage
    six = ndimage.generate_binary_structure(3, 1)
    rng = np.random.default_rng(6)
    for shape in ((9, 7, 5), (37, 29, 23)):
        mask = rng.random(shape) < 0.8
        assert np.array_equal(F.erode(mask), ndimage.binary_erosion(mask, six, border_value=1))
        assert np.array_equal(F.dilate(mask), ndimage.binary_dilation(mask, six, border_value=0))


def test_the_restatement_recovers_the_head():
    """DESIGN.md section 5.16, on the 37 x 29 x 23 phantom with this restatement: bin 87; Dice against the true ellipsoid 0.9906 for the raw
    mask, 0.9940 for the largest component (the detached block gone), 1.0 after the holes are filled (all 81 ventricle voxels back, and one
    dark noise voxel).  Bars: the recorded Dice minus 0.005 after steps 6 and 7; the block removed and the ventricle filled entirely."""
    values, head, ventricle, block = F.phantom()
    assert values.shape == F.PHANTOM_SHAPE == (37, 29, 23) and int(ventricle.sum()) == F.RECORDED['ventricle'] == 81 and int(block.sum()) == 48
    assert (values > 0).all()                                                          # Rician air: every voxel is "brain" to the != 0 rule
    out, mask, report, stages = F.foreground(values)
    figures = dict(bin=report['bin'], dice_raw=F.dice(stages['raw'], head), dice_largest=F.dice(stages['largest'], head), dice_filled=F.dice(mask, head))
    print(figures, report)
    assert report['bin'] == F.RECORDED['bin'] and report['candidates'] == values.size and report['components'] == 2
    assert figures['dice_largest'] >= F.RECORDED['dice_largest'] - F.DICE_SLACK and figures['dice_filled'] >= F.RECORDED['dice_filled'] - F.DICE_SLACK
    assert abs(figures['dice_raw'] - F.RECORDED['dice_raw']) < 1e-4
    assert stages['raw'][block].all() and not stages['largest'][block].any() and not mask[block].any()
    assert not stages['largest'][ventricle].any() and mask[ventricle].all()
    assert report['kept'] == int(mask.sum()) and report['filled'] == int(mask.sum() - stages['largest'].sum()) >= 81
    assert report['removed'] == values.size - report['kept']
    assert np.array_equal(out[mask], values[mask]) and not out[~mask].any() and not np.signbit(out[~mask]).any()
    kept_holes = F.foreground(values, keep_holes=True)
    assert np.array_equal(kept_holes[1], stages['largest']) and kept_holes[2]['filled'] == 0
    # degenerate inputs are left untouched
    for v in (np.zeros((4, 4, 4), np.float32), np.full((4, 4, 4), 7.0, np.float32)):
        assert F.foreground(v)[0] is None and F.foreground(v)[2]['threshold'] is None
    # a non-finite voxel inside a filled hole keeps its bits; outside the mask it becomes 0
    special = values.copy()
    special[18, 14, 11], special[0, 28, 22], special[1, 28, 22] = np.nan, np.inf, -np.inf
    out, mask, report, _ = F.foreground(special)
    assert mask[18, 14, 11] and np.isnan(out[18, 14, 11]) and out[0, 28, 22] == 0 and out[1, 28, 22] == 0
    assert report['candidates'] == values.size - 3
