"""CPU: the one preparation stage of the volume pipeline (mudiff_hip.volume_prepare) on three tiny int16 volumes, with the device stages
(volume_coreg.coregister, volume_regrid.regrid_to, volume_bias.correct) replaced by recorders: which stage sees which volume in which
order, what the report lists, prints and writes, the two refusals, and that the host stacks made through this route are the bits
load_and_preprocess_volume gives for every stored datatype, byte order and scaling."""
import json
import os

import numpy as np
import pytest

import volume_intake_ref as R

SHAPE = (8, 8, 9)
NEEDED = ['FLAIR', 'T2', 'T1']                       # MODALITY_ORDERS['T1CE']


@pytest.fixture
def subject(tmp_path):
    from mudiff_hip import volume_intake as VI
    rng = np.random.default_rng(4)
    paths = [R.write_nifti_typed(tmp_path / f'{m.lower()}.nii.gz', rng.integers(0, 50, SHAPE).astype(np.int16)) for m in NEEDED]
    return paths, [(m, VI.read_nifti_raw(p)) for m, p in zip(NEEDED, paths)]


class StandIn:
    """What a recorder returns in place of a volume: it remembers what it was made from."""

    def __init__(self, stage, source):
        self.stage, self.source = stage, source


@pytest.fixture
def recorded(monkeypatch):
    from mudiff_hip import volume_bias as VB
    from mudiff_hip import volume_coreg as VC
    from mudiff_hip import volume_regrid as VR
    calls = []

    def coregister(fixed, moving, device, **kw):
        calls.append(('coregister', fixed, moving, kw))
        W = np.eye(4)
        W[0, 3] = float(len(calls))                   # a different W per call
        return W, dict(params=[float(len(calls)), 0, 0, 0, 0, 0], accepted=True)

    def regrid_to(raw, ref_shape, ref_affine, device, mode='linear', header=None, world=None):
        calls.append(('regrid_to', raw, tuple(ref_shape), header, world))
        return StandIn('regridded', raw)

    def correct(raw, device, **kw):
        calls.append(('correct', raw, kw))
        return StandIn('corrected', raw), dict(iterations=[1], of=len(calls))

    monkeypatch.setattr(VC, 'coregister', coregister)
    monkeypatch.setattr(VR, 'regrid_to', regrid_to)
    monkeypatch.setattr(VB, 'correct', correct)
    return calls


def test_with_everything_off_the_inputs_pass_through(subject, recorded):
    from mudiff_hip import volume as V
    from mudiff_hip.volume_prepare import IntakeOptions, prepare_inputs
    paths, named = subject
    options = IntakeOptions.from_args(V.build_argparser(['--target_modality', 'T1CE', '--output_dir', 'o', '--exp', 'e', '--slice_half_range', '2']))
    assert options == IntakeOptions('percentile', False, None, None, 2)
    prepared, ref, report = prepare_inputs(named, options, None)
    assert len(prepared) == 3 and all(a is raw for a, (_, raw) in zip(prepared, named)) and recorded == []
    _, shp, aff, hdr, s0, s1 = V.load_and_preprocess_volume(paths[0], 2)
    assert ref[0] == shp == SHAPE and np.array_equal(ref[1], aff) and ref[2].raw == hdr.raw and ref[3:] == (s0, s1) == (2, 6)
    assert report.suffix() == '' and (report.regridded, report.coreg, report.bias) == ([], [], [])


def test_with_everything_on_the_stages_run_in_order(subject, recorded):
    from mudiff_hip import volume as V
    from mudiff_hip import volume_bias as VB
    from mudiff_hip import volume_coreg as VC
    from mudiff_hip.volume_prepare import IntakeOptions, prepare_inputs
    _, named = subject
    raws = [raw for _, raw in named]
    options = IntakeOptions('zscore', True, dict(strides=(4,), max_mm=10.0, max_deg=5.0), dict(VB.DEFAULTS, field=False), 2)
    prepared, ref, report = prepare_inputs(named, options, 'the device')
    assert [c[0] for c in recorded] == ['correct', 'coregister', 'regrid_to', 'correct', 'coregister', 'regrid_to', 'correct']
    assert recorded[0][1] is raws[0] and recorded[0][2] == options.bias                 # the first input: corrected only
    for k, raw in ((1, raws[1]), (4, raws[2])):
        co, re, bi = recorded[k:k + 3]
        assert co[1] is raws[0] and co[2] is raw and co[3] == options.coreg             # coregister(first, raw)
        assert re[1] is raw and re[2] == SHAPE and re[3] is ref[2] and re[4][0, 3] == float(k + 1)      # regrid_to(..., world = that W)
        assert bi[1].stage == 'regridded' and bi[1].source is raw                      # correct(the regridded volume)
    assert [(v.stage, v.source.stage if v.source is not raws[0] else None) for v in prepared] == [('corrected', None)] + [('corrected', 'regridded')] * 2
    assert report.regridded == ['T2', 'T1'] and [n for n, _ in report.coreg] == ['T2', 'T1']
    assert [(n, f) for n, _, f in report.bias] == [('FLAIR', None), ('T2', None), ('T1', None)]
    assert report.suffix() == V.regrid_suffix(['T2', 'T1']) + VC.coreg_suffix(report.coreg) + VB.bias_suffix(report.bias)
    assert report.suffix() == ' | regrid=T2,T1 | coreg=T2:2.00mm/0.00deg,T1:5.00mm/0.00deg | bias=FLAIR,T2,T1'
    report.regridded += ['gt_volume']                                                   # the evaluation inputs go after the inputs
    assert report.suffix().startswith(' | regrid=T2,T1,gt_volume | coreg=')


def test_report_files(subject, recorded, tmp_path):
    from mudiff_hip import volume_bias as VB
    from mudiff_hip.volume_prepare import IntakeOptions, IntakeReport, prepare_inputs
    _, named = subject
    report = prepare_inputs(named, IntakeOptions(regrid=True, coreg=dict(strides=(4,)), bias=dict(VB.DEFAULTS, field=False), half_range=2), None)[2]
    out = tmp_path / 'out'
    report.write(str(out), 'T1CE', np.eye(4), None)
    assert sorted(os.listdir(out)) == ['bias_t1ce.json', 'coreg_t1ce.json']
    assert list(json.load(open(out / 'coreg_t1ce.json'))) == ['T2', 'T1'] and list(json.load(open(out / 'bias_t1ce.json'))) == NEEDED
    IntakeReport().write(str(tmp_path / 'none'), 'T1CE', np.eye(4), None)
    IntakeReport(['gt_volume']).write(str(tmp_path / 'none'), 'T1CE', np.eye(4), None)
    assert not os.path.exists(tmp_path / 'none')                                        # an empty report: not even the directory


def test_refusals(subject, recorded, tmp_path):
    from mudiff_hip import volume as V
    from mudiff_hip import volume_intake as VI
    from mudiff_hip.volume_prepare import IntakeOptions, prepare_inputs
    _, named = subject
    other = VI.read_nifti_raw(R.write_nifti_typed(tmp_path / 'other.nii.gz', np.ones((8, 6, 9), np.int16)))
    with pytest.raises(ValueError, match=r'All input volumes must share shape. Got \(8, 6, 9\) vs \(8, 8, 9\) for T2$'):
        prepare_inputs([named[0], ('T2', other), named[2]], IntakeOptions(half_range=2), None)
    with pytest.raises(ValueError, match=r'share shape.* for /data/t2.nii$'):           # the device paths name the file
        prepare_inputs([named[0], ('T2', other), named[2]], IntakeOptions(half_range=2), None, labels={'T2': '/data/t2.nii'})
    V.write_nifti(str(tmp_path / 'series.nii.gz'), np.ones(SHAPE + (2,), np.float32), np.eye(4))
    series = VI.read_nifti_raw(str(tmp_path / 'series.nii.gz'))
    assert series.shape == SHAPE + (2,)
    everything = IntakeOptions(regrid=True, coreg={}, bias=dict(field=False), half_range=2)
    for options in (IntakeOptions(half_range=2), everything):
        with pytest.raises(ValueError, match=r'^T1: expected a 3D volume, got shape \(8, 8, 9, 2\)$'):
            prepare_inputs(named[:2] + [('T1', series)], options, None)
    assert recorded == []                                                               # refused before any device work


CASES = [('u1', '<', 0.0, 0.0), ('i2', '<', 0.0, 0.0), ('u2', '<', 0.0, 0.0), ('i4', '<', 0.0, 0.0), ('f4', '<', 0.0, 0.0), ('f8', '<', 0.0, 0.0),
         ('i2', '>', 0.0, 0.0), ('i2', '<', 0.5, -1.0)]


@pytest.mark.parametrize('norm', ['percentile', 'zscore'])
def test_host_stacks_are_the_bits_of_load_and_preprocess_volume(tmp_path, norm):
    """Every stored datatype, a big-endian file and a scaled one (f8 and big-endian come back through read_nifti as float32): the plain
    host path through read_nifti_raw -> prepare_inputs -> host_stacks gives what the loop over load_and_preprocess_volume gave."""
    from mudiff_hip import volume as V
    from mudiff_hip import volume_intake as VI
    from mudiff_hip.volume_prepare import IntakeOptions, prepare_inputs
    options = IntakeOptions(norm=norm, half_range=2)
    for i, (dtype, endian, slope, inter) in enumerate(CASES):
        path = R.write_nifti_typed(tmp_path / f'v{i}.nii.gz', R.synthetic(SHAPE, 'noise', dtype, seed=10 + i), endian, slope, inter)
        raw = VI.read_nifti_raw(path)
        assert (raw.code == R.CODES[dtype] and raw.scaled == R.is_scaled(slope, inter)) if (dtype != 'f8' and endian == '<') else raw.code == R.CODES['f4']
        prepared, ref, _ = prepare_inputs([('FLAIR', raw)], options, None)
        got = V.host_stacks(prepared, options)[0]
        slices, shp, _, _, s0, s1 = V.load_and_preprocess_volume(path, 2, norm)
        want = np.stack(slices, 0)
        assert got.dtype == want.dtype == np.float32 and got.shape == (5,) + SHAPE[:2] and got.tobytes() == want.tobytes() and want.any()
        assert (ref[0], ref[3], ref[4]) == (shp, s0, s1)
