"""CPU: the host side of --unring (mudiff_hip.volume_unring) and its numpy restatement
(tests/volume_unring_ref.py): the properties of the definition, the recovery of a k-space-truncated phantom by the restatement alone,
the host-built tables, the flags, the place of the stage in volume_prepare.prepare_inputs, the [done] suffix and the report file."""
import argparse
import json
import os

import numpy as np
import pytest

import volume_intake_ref as R
import volume_unring_ref as U
from volume_support import cli_argv


# ---------------------------------------------------------------------------------------------------
# the restatement against the definition's properties
# ---------------------------------------------------------------------------------------------------
def test_zeros_give_zeros_and_a_constant_comes_back():
    for shape, axes in (((12, 9, 2), (0, 1)), ((3, 8, 11), (1, 2))):
        found = U.unring(np.zeros(shape), axes)
        assert not found['out'].any() and not found['jx'].any() and not found['jy'].any()      # an all-equal score keeps s = 0
        for c in (7.25, -1e6, 3e-9):
            assert np.abs(U.unring(np.full(shape, c), axes)['out'] - c).max() <= 1e-12 * abs(c)
    x = np.full((8, 9), np.nan)
    x[1, 3], x[2, 5] = np.inf, 2.0
    found = U.unring(x[:, :, None] * np.ones(2), (1, 0))
    assert found['nonfinite'] == 2 * 71 and np.isfinite(found['out']).all()                   # non-finite voxels are read as 0 and counted


def test_shift_order_and_the_tie_rule():
    assert np.allclose(U.shifts(2), [0.0, 0.2, 0.4, -0.2, -0.4]) and np.allclose(U.shifts(20)[[1, 20, 21, 40]], [1 / 41, 20 / 41, -1 / 41, -20 / 41])
    TV = np.array([[3.0, 1.0, 2.0, 0.0], [1.0, 1.0, 3.0, 0.0], [1.0, 0.5, 2.0, 0.0], [0.5, 0.5, 2.0, 0.0], [0.5, 2.0, 2.5, 0.0]])
    assert U.choose(TV).tolist() == [3, 2, 0, 0]       # the first of the two 0.5s; the first 0.5; the earliest of an exact tie; all equal: s = 0
    # on a line: one that every shift leaves with the same score keeps s = 0 everywhere, and the map indexes the shifts in that order
    out, jmap, TV = U.unring_lines(np.zeros((2, 10)), 3)
    assert not jmap.any() and not TV.any() and not out.any()
    step = np.r_[np.zeros(12), np.ones(12)]
    ringing = np.fft.ifft(np.fft.fft(np.repeat(step, 4))[np.r_[0:12, 84:96]]).real / 4                          # 24 of 96 coefficients
    out, jmap, TV = U.unring_lines(ringing, 20)
    assert np.array_equal(TV[jmap.astype(int), np.arange(24)], TV.min(0)) and set(np.unique(jmap)) - {0}
    first = np.array([np.flatnonzero(TV[:, l] == TV[:, l].min())[0] for l in range(24)])
    assert np.array_equal(jmap, first)


def test_the_shifted_line_is_the_band_limited_line_at_l_plus_s():
    """y_s[l] of a sampled harmonic below the band edge is the harmonic at l + s; the Nyquist bin of an even n carries cos(pi s)."""
    for n in (9, 16):
        l = np.arange(n)
        D = U.shift_table(n, 3)
        for j, s in enumerate(U.shifts(3)):
            for k in (1, 3):
                x = np.cos(2 * np.pi * k * l / n + 0.3)
                assert np.abs(U.circulant(D[j]) @ x - np.cos(2 * np.pi * k * (l + s) / n + 0.3)).max() < 1e-13
            if n % 2 == 0:
                assert np.abs(U.circulant(D[j]) @ np.cos(np.pi * l) - np.cos(np.pi * s) * np.cos(np.pi * l)).max() < 1e-13
        assert np.array_equal(D[0], np.eye(n)[0]) or np.abs(D[0] - np.eye(n)[0]).max() < 1e-15


def test_the_filter_pair_sums_to_the_image_bit_for_bit():
    """Iy is I - Ix as computed, bit for bit, so Ix + Iy = I + the one rounding of that subtraction, which rounds back to I itself
    wherever |Iy| <= |I| and I has a spare trailing bit (a tie then goes to I): stored integers, as scanners write them, and a positive
    image, whose Ix is near I / 2.  On arbitrary fp64 values the sum may differ from I in the last place.  The corner bin is picked by
    index and holds 1/2; Gx + Gy = 1."""
    rng = np.random.default_rng(2)
    for shape in ((16, 12, 3), (15, 12, 2), (9, 7, 2)):
        vol = np.rint(100.0 + 10.0 * rng.standard_normal(shape))
        ix, iy = U.split(vol, (0, 1))
        assert np.array_equal(iy, vol - ix) and np.array_equal(ix + iy, vol) and np.abs(ix - vol / 2).max() < 40
        anyway = rng.standard_normal(shape)
        ax, ay = U.split(anyway, (0, 1))
        assert np.array_equal(ay, anyway - ax) and (np.abs(ax + ay - anyway) <= np.spacing(np.abs(anyway) + np.abs(ay))).all()
        ix32, iy32 = U.split(vol.astype(np.float32), (0, 1), np.float32)
        assert ix32.dtype == np.float32 and np.array_equal(ix32 + iy32, vol.astype(np.float32)) and np.abs(ix32 - ix).max() < 1e-4
    G = U.direction_filter(16, 12)
    assert G[8, 6] == 0.5 and G[0, 0] == 0.5 and np.isfinite(G).all() and np.allclose(G + U.direction_filter(12, 16).T, 1.0)
    assert U.direction_filter(15, 12)[7, 6] == 0.0 and U.direction_filter(16, 12)[8, 0] == 1.0      # cy = 0 -> 0; cx = 0 -> 1


def test_the_restatement_removes_the_ringing_of_a_truncated_phantom():
    """Six random ellipses rendered at 8x, truncated to n x n coefficients: the RMS error against the box-averaged truth, more than one
    pixel away from every edge, falls by at least 2 x at 48 x 48 (3.8 x with this phantom; the bar is about half of that, so that another
    random phantom passes) and strictly at 30 x 30; the opposite re-interpolation sign, which leaves every moved voxel two shifts away
    from its centre, is worse than the right one over the whole image (0.068 against 0.016 at 48 x 48)."""
    for n, factor in ((48, 2.0), (30, 1.0)):
        ringing, truth, away = U.phantom(n, seed=0)
        out = U.unring(ringing[:, :, None])['out'][:, :, 0]
        wrong = U.unring(ringing[:, :, None], sign=-1.0)['out'][:, :, 0]
        before, after = U.rms(ringing, truth, away), U.rms(out, truth, away)
        everywhere = np.ones((n, n), bool)
        print(n, 'before', before, 'after', after, 'ratio', before / after, 'whole image: right', U.rms(out, truth, everywhere), 'wrong sign',
              U.rms(wrong, truth, everywhere))
        assert away.sum() > n * n / 4 and after < before and factor * after <= before
        assert U.rms(out, truth, everywhere) < U.rms(ringing, truth, everywhere) < U.rms(wrong, truth, everywhere)


# ---------------------------------------------------------------------------------------------------
# the host's share: the tables
# ---------------------------------------------------------------------------------------------------
def test_the_tables_are_the_definition_rounded_to_fp32():
    from mudiff_hip import volume_unring as VU
    for n, N in ((8, 20), (9, 3), (30, 32), (511, 2), (512, 20)):
        D = VU.shift_table(n, N)
        assert D.dtype == np.float32 and D.shape == (2 * N + 1, n) and np.array_equal(D[0], np.eye(n, dtype=np.float32)[0])
        assert np.abs(D.astype(np.float64) - U.shift_table(n, N)).max() <= 2.0 ** -24 and np.allclose(VU.shift_values(N), U.shifts(N), rtol=0, atol=0)
    for nx, ny in ((8, 9), (9, 8), (16, 12), (512, 8)):
        tw, g = VU.filter_tables(nx, ny)
        assert tw.shape == (nx, 2) and g.shape == (nx // 2 + 1, ny) and tw.dtype == g.dtype == np.float64
        m = np.arange(nx)
        assert np.abs(tw[:, 0] - np.cos(2 * np.pi * m / nx)).max() <= 2.0 ** -52 and np.abs(tw[:, 1] + np.sin(2 * np.pi * m / nx)).max() <= 2.0 ** -52
        want = np.fft.ifft(U.direction_filter(nx, ny)[:nx // 2 + 1], axis=1)
        assert np.abs(want.imag).max() < 1e-15 and np.abs(g - want.real).max() <= 2.0 ** -50


# ---------------------------------------------------------------------------------------------------
# the stage: flags, pins, suffix, report, its place in prepare_inputs
# ---------------------------------------------------------------------------------------------------
def test_flags_and_defaults_on_both_command_lines():
    from mudiff_hip import cohort, volume as V
    from mudiff_hip import volume_unring as VU
    from mudiff_hip.volume_prepare import IntakeOptions
    assert VU.DEFAULTS == dict(axes=(0, 1), shifts=20, window=(1, 3))
    for build, extra in ((V.build_argparser, []), (cohort.build_argparser, ['--manifest', 'm.tsv'])):
        plain = build(cli_argv(*extra))
        assert plain.unring is False and plain.unring_axes == [0, 1] and plain.unring_shifts == 20 and plain.unring_window == [1, 3]
        assert IntakeOptions.from_args(plain).unring is None and IntakeOptions.from_args(plain) == IntakeOptions('percentile', False, None, None, 80)
        assert IntakeOptions.from_args(build(cli_argv('--unring', *extra))).unring == VU.DEFAULTS
        args = build(cli_argv('--unring', '--unring_axes', '1', '2', '--unring_shifts', '32', '--unring_window', '2', '8', '--denoise', *extra))
        options = IntakeOptions.from_args(args)
        assert options.unring == dict(axes=(1, 2), shifts=32, window=(2, 8)) and options.denoise is not None
    assert VU.options_from(argparse.Namespace()) == dict(unring=None) and VU.options_from(argparse.Namespace(unring=True)) == dict(unring=VU.DEFAULTS)


REFUSALS = [(['--unring_axes', '0', '0'], 'unring_axes'), (['--unring_axes', '0', '3'], 'unring_axes'), (['--unring_axes', '-1', '1'], 'unring_axes'),
            (['--unring_shifts', '0'], 'unring_shifts'), (['--unring_shifts', '33'], 'unring_shifts'), (['--unring_window', '0', '3'], 'unring_window'),
            (['--unring_window', '3', '2'], 'unring_window'), (['--unring_window', '1', '9'], 'unring_window'), (['--unring_axes', '1'], 'unring_axes'),
            (['--unring_shifts', '2.5'], 'unring_shifts')]


@pytest.mark.parametrize('bad, word', REFUSALS, ids=['-'.join(b) for b, _ in REFUSALS])
def test_bad_values_are_refused_naming_the_flag(bad, word, capsys):
    from mudiff_hip import cohort, volume as V
    for build in (lambda: V.build_argparser(cli_argv('--unring', *bad)), lambda: cohort.build_argparser(cli_argv('--manifest', 'm.tsv', *bad))):
        with pytest.raises(SystemExit) as e:
            build()
        assert e.value.code == 2 and word in capsys.readouterr().err


def test_check_options_and_check_shape_name_the_flag_and_the_input():
    from mudiff_hip import volume_unring as VU
    for kw, flag in ((dict(axes=(1, 1)), '--unring_axes'), (dict(axes=(0, 1, 2)), '--unring_axes'), (dict(shifts=0), '--unring_shifts'),
                     (dict(shifts=33), '--unring_shifts'), (dict(window=(0, 1)), '--unring_window'), (dict(window=(2, 1)), '--unring_window'),
                     (dict(window=(1, 9)), '--unring_window')):
        with pytest.raises(ValueError, match=flag):
            VU.check_options(**kw)
    VU.check_options(axes=(2, 0), shifts=32, window=(8, 8))
    VU.check_shape((8, 512, 3), 'FLAIR')
    VU.check_shape((3, 18, 18), 'FLAIR', axes=(1, 2), window=(2, 8))
    for shape, kw, flag in (((7, 9, 9), {}, '--unring_window'), ((9, 513, 9), {}, '--unring_axes'), ((30, 17, 9), dict(window=(2, 8)), '--unring_window'),
                            ((30, 30, 7), dict(axes=(0, 2)), '--unring_window')):
        with pytest.raises(ValueError, match='(?s)t2.nii.gz.*' + flag):
            VU.check_shape(shape, 't2.nii.gz', **kw)
    # unring() refuses such an input, by the name it is given, before it touches the device
    with pytest.raises(ValueError, match='(?s)FLAIR.*--unring_window'):
        VU.unring(argparse.Namespace(shape=(7, 20, 3)), 'no device', name='FLAIR')
    with pytest.raises(ValueError, match='3D'):
        VU.unring(argparse.Namespace(shape=(7, 20)), 'no device')


def test_the_pins_of_the_wiring():
    from mudiff_hip import volume as V
    from mudiff_hip import volume_align as VA, volume_unring as VU
    from mudiff_hip.volume_prepare import STAGES, IntakeOptions, IntakeReport
    assert STAGES[-1].module is VA and STAGES[-2].module is VU and STAGES[-2].written == 'unring'
    assert IntakeOptions._fields[-3:] == ('unring', 'align', 'denoise') and IntakeOptions().unring is None
    assert IntakeOptions._fields[:5] == ('norm', 'regrid', 'coreg', 'bias', 'half_range')
    assert IntakeOptions._fields.index('brain') == IntakeOptions._fields.index('foreground') + 1
    assert IntakeReport().unring == []
    p = V.make_parser()
    new = ['--unring', '--unring_axes', '--unring_shifts', '--unring_window']
    assert [o for a in p.lates[1]._actions for o in a.option_strings] == new                  # a late parser of its own, right after --align's
    assert not any(o in new for late in [p] + p.lates[:1] + p.lates[2:] for a in late._actions for o in a.option_strings)
    assert '--unring_window' in p.format_help()


def test_unring_suffix_and_reports(tmp_path):
    from mudiff_hip import volume_unring as VU
    from mudiff_hip.volume_prepare import IntakeReport
    assert VU.unring_suffix([]) == '' and VU.unring_suffix(None) == ''
    one = dict(axes=[0, 1], shifts=20, window=[1, 3], n=[240, 240], nonfinite=0, moved=[0.4, 0.5], mean_abs_shift=[0.1, 0.12])
    reports = [('FLAIR', one), ('T2', dict(one, nonfinite=3))]
    assert VU.unring_suffix(reports) == ' | unring=FLAIR,T2'
    path = VU.write_reports(reports, str(tmp_path / 'o'), 'T1CE')
    assert os.path.basename(path) == 'unring_t1ce.json' and json.load(open(path)) == dict(reports)
    report = IntakeReport()
    assert report.unring == [] and report.suffix() == ''
    report.unring += reports
    report.denoise.append(('FLAIR', dict(sigma=1.0)))
    report.align.append(('FLAIR', dict(kept=0)))
    assert report.suffix() == ' | denoise=FLAIR | unring=FLAIR,T2 | align=FLAIR:kept=0'         # the other parts keep their order
    report.align.clear()
    report.write(str(tmp_path / 'p'), 'T1CE', np.eye(4), None)
    assert sorted(os.listdir(tmp_path / 'p')) == ['denoise_t1ce.json', 'unring_t1ce.json']


class StandIn:
    def __init__(self, stage, source):
        self.stage, self.source = stage, source
        self.shape, self.affine, self.header = source.shape, source.affine, source.header


def test_prepare_inputs_unrings_every_input_after_denoise_and_before_foreground(tmp_path, monkeypatch):
    """unring is called for every input after denoise and before foreground and coregister, with the input's name; under --align the first
    input, which estimate_alignment has taken through the stages, is not processed twice."""
    from mudiff_hip import volume_align as VA, volume_coreg as VC, volume_denoise as VD, volume_foreground as VF, volume_intake as VI
    from mudiff_hip import volume_regrid as VR, volume_unring as VU
    from mudiff_hip import volume_conform as VCF
    from mudiff_hip.volume_prepare import IntakeOptions, estimate_alignment, prepare_inputs
    rng = np.random.default_rng(4)
    names = ['FLAIR', 'T2', 'T1']
    raws = [VI.read_nifti_raw(R.write_nifti_typed(tmp_path / f'{m}.nii.gz', rng.integers(0, 50, (8, 8, 9)).astype(np.int16))) for m in names]
    calls = []

    def stage(kind, result):
        def run(raw, device, name=None, **kw):
            calls.append((kind, raw, kw, name))
            return StandIn(result, raw), dict(step=len(calls), mask_voxels=1)
        return run

    def coregister(fixed, moving, device, **kw):
        calls.append(('coregister', fixed, moving, None))
        return np.eye(4), dict(params=[0.0] * 6, accepted=True)

    def regrid_to(raw, ref_shape, ref_affine, device, mode='linear', header=None, world=None, **kw):
        calls.append(('regrid_to', raw, None, None))
        return StandIn('regridded', raw)

    def estimate(first, device, **kw):
        calls.append(('estimate', first, kw, None))
        return np.eye(4), dict(accepted=True)

    monkeypatch.setattr(VD, 'denoise', stage('denoise', 'denoised'))
    monkeypatch.setattr(VU, 'unring', stage('unring', 'unrung'))
    monkeypatch.setattr(VF, 'foreground', stage('foreground', 'masked'))
    monkeypatch.setattr(VC, 'coregister', coregister)
    monkeypatch.setattr(VR, 'regrid_to', regrid_to)
    monkeypatch.setattr(VA, 'estimate', estimate)
    unring = dict(axes=(0, 1), shifts=7, window=(1, 2))
    options = IntakeOptions(regrid=True, coreg=dict(strides=(4,)), half_range=2, denoise=dict(VD.DEFAULTS), unring=unring,
                            foreground=dict(VF.DEFAULTS, mask_out=False))
    labels = {m: f'{m.lower()}.nii.gz' for m in names}
    prepared, ref, report = prepare_inputs(list(zip(names, raws)), options, 'the device', labels=labels)
    assert [c[0] for c in calls] == ['denoise'] * 3 + ['unring'] * 3 + ['foreground'] * 3 + ['coregister', 'regrid_to'] * 2
    assert [c[1].source for c in calls[3:6]] == raws and all(c[1].stage == 'denoised' and c[2] == unring for c in calls[3:6])
    assert [c[3] for c in calls[3:6]] == ['flair.nii.gz', 't2.nii.gz', 't1.nii.gz']            # what an error message would call the input
    assert all(c[1].stage == 'unrung' for c in calls[6:9]) and calls[9][1].stage == 'masked'
    assert [n for n, _ in report.unring] == names and [r['step'] for _, r in report.unring] == [4, 5, 6]
    assert report.suffix() == ' | regrid=T2,T1 | coreg=T2:0.00mm/0.00deg,T1:0.00mm/0.00deg | denoise=FLAIR,T2,T1 | foreground=FLAIR,T2,T1 | unring=FLAIR,T2,T1'
    # the flag alone: the corrected volumes come back in order, nothing else runs; without it the stage is not called
    del calls[:]
    prepared, ref, report = prepare_inputs(list(zip(names, raws)), IntakeOptions(half_range=2, unring=unring), None)
    assert [c[0] for c in calls] == ['unring'] * 3 and [v.source for v in prepared] == raws and report.suffix() == ' | unring=FLAIR,T2,T1'
    del calls[:]
    prepared, ref, report = prepare_inputs(list(zip(names, raws)), IntakeOptions(half_range=2), None)
    assert calls == [] and prepared == raws and report.unring == []
    # --align: the plane is estimated from the first input after denoise and unring, which prepare_inputs then runs on the later inputs only
    del calls[:]
    options = IntakeOptions(half_range=2, denoise=dict(VD.DEFAULTS), unring=unring, conform=dict(shape=VCF.DEFAULT_SHAPE, spacing=VCF.DEFAULT_SPACING, target=VCF.DEFAULT_TARGET), align=dict(VA.DEFAULTS))
    found = estimate_alignment(raws[0], options, 'the device')
    assert [c[0] for c in calls] == ['denoise', 'unring', 'estimate'] and calls[2][1].stage == 'unrung' and found.first is calls[2][1]
    assert calls[1][3] == 'the first input' and [r['step'] for _, r in found.stages.unring] == [2]
    del calls[:]
    prepared, ref, report = prepare_inputs(list(zip(names, raws)), options, 'the device', align=found)
    assert [c[0] for c in calls] == ['denoise'] * 2 + ['unring'] * 2 + ['regrid_to'] * 3
    assert [c[1].source for c in calls[2:4]] == raws[1:] and calls[4][1] is found.first
    assert [n for n, _ in report.unring] == names and [r['step'] for _, r in report.unring] == [2, 3, 4]
