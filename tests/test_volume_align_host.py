"""Host: --align.  The definitions of mudiff_hip.volume_align (the mirror is an involution that fixes the plane,
the pose transform carries the grid's centre column onto it), the flags on both command lines, the suffix and the report file, and the
search itself over the numpy restatement of the moments (tests/volume_align_ref.py): it recovers the planted planes of the analytic head
to the method's own resolution, and falls back to the identity for a plane outside the search range and for a constant volume."""
import argparse
import json

import numpy as np
import pytest

import volume_align_ref as AR
import volume_support as VS

POSES_ANY = ((7.0, -5.0, 3.0), (-12.0, 9.0, -4.5), (0.0, 0.0, 0.0), (20.0, -20.0, 12.0))
CENTRE = np.array([5.0, -8.0, 12.0])


# ---------------------------------------------------------------------------------------------------
# the definitions
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('pose', POSES_ANY)
def test_the_mirror_is_an_involution_that_fixes_the_plane(pose):
    from mudiff_hip import volume_align as VA
    H, n = VA.mirror_world(pose, CENTRE), VA.normal(pose[0], pose[1])
    assert np.allclose(H @ H, np.eye(4), atol=1e-12) and abs(np.linalg.norm(n) - 1.0) < 1e-15
    assert np.allclose(n, VA.rotation(pose[0], pose[1]) @ np.array([1.0, 0, 0]))
    rng = np.random.default_rng(3)
    u = rng.standard_normal((50, 3))
    on_plane = CENTRE + pose[2] * n + u - np.outer(u @ n, n)               # n . (p - c) = t
    assert np.allclose(on_plane @ H[:3, :3].T + H[:3, 3], on_plane, atol=1e-11)
    p = CENTRE + 30.0 * u                                                 # any point: its image lies as far on the other side
    q = p @ H[:3, :3].T + H[:3, 3]
    assert np.allclose((q - CENTRE) @ n - pose[2], -((p - CENTRE) @ n - pose[2]), atol=1e-11)
    assert np.allclose(np.linalg.det(H[:3, :3]), -1.0)


@pytest.mark.parametrize('pose', POSES_ANY)
def test_the_pose_transform_maps_the_centre_column_onto_the_plane(pose):
    from mudiff_hip import volume_align as VA
    T, n = VA.pose_world(pose, CENTRE), VA.normal(pose[0], pose[1])
    assert np.allclose(T[:3, :3] @ T[:3, :3].T, np.eye(3), atol=1e-14) and np.allclose(np.linalg.det(T[:3, :3]), 1.0)
    rng = np.random.default_rng(4)
    p = CENTRE + 40.0 * rng.standard_normal((50, 3))
    p[:, 0] = CENTRE[0]                                                   # the plane x = c_x
    q = p @ T[:3, :3].T + T[:3, 3]
    assert np.allclose((q - CENTRE) @ n, pose[2], atol=1e-11)
    assert np.allclose(T[:3, :3] @ np.array([1.0, 0, 0]), n)              # the left-right axis becomes the normal
    assert np.array_equal(VA.pose_world((0.0, 0.0, 0.0), CENTRE), np.eye(4))
    # the mirror through the plane is the pose transform's image of the mirror through x = c_x
    flip = np.eye(4)
    flip[0, 0], flip[0, 3] = -1.0, 2.0 * CENTRE[0]
    assert np.allclose(T @ flip @ np.linalg.inv(T), VA.mirror_world(pose, CENTRE), atol=1e-11)


def test_the_turned_conform_grid_has_its_centre_column_on_the_plane():
    from mudiff_hip import volume_align as VA
    from mudiff_hip import volume_conform as VCF
    from mudiff_hip import volume_prepare as VP
    pose, A = (7.0, -5.0, 3.0), AR.affine()
    shape, grid = VCF.conform_grid(AR.SHAPE, A, shape=(24, 22, 20), spacing=(3.0, 3.0, 4.0))
    assert np.allclose(grid[:3, :3] @ ((np.array(shape) - 1.0) / 2.0) + grid[:3, 3], CENTRE)
    turned = VP.aligned_affine(VA.pose_world(pose, CENTRE), grid)
    n = VA.normal(pose[0], pose[1])
    column = np.array([[(shape[0] - 1) / 2.0, j, k, 1.0] for j in (0, 7, 21) for k in (0, 9, 19)]).T
    assert np.allclose(((turned @ column)[:3].T - CENTRE) @ n, pose[2], atol=1e-11)
    assert np.allclose(turned[:3, 0] / np.linalg.norm(turned[:3, 0]), -n)      # LPS: the first voxel axis runs towards the left, along -n
    assert VP.aligned_affine(np.eye(4), grid) is grid


def test_scores():
    from mudiff_hip import volume_align as VA
    a = np.array([0, 1, 2, 3, 4, 5], np.int64)
    b = np.array([1, 1, 2, 5, 4, 7], np.int64)
    sums = [len(a), a.sum(), b.sum(), (a * a).sum(), (b * b).sum(), (a * b).sum()]
    r = VA.scores([sums, sums, [6, 6, 9, 6, 15, 9], [0] * 6], 10, min_overlap=0.5)
    assert abs(r[0] - np.corrcoef(a, b)[0, 1]) < 1e-14 and r[1] == r[0]
    assert r[2] == -np.inf and r[3] == -np.inf                             # a flat side; nothing counted
    assert VA.scores([sums], 13, min_overlap=0.5)[0] == -np.inf            # 6 < 6.5: too little of the volume in view
    assert VA.sample_points((48, 44, 40), 1) == 48 * 44 * 40 and VA.sample_points((48, 44, 41), 3) == 16 * 15 * 14


def test_schedule():
    from mudiff_hip import volume_align as VA
    levels = VA.schedule(5.0, 4.0, 0.35, 0.25, (4, 2))
    assert levels == [(5.0, 4.0, 4), (2.5, 2.0, 4), (1.25, 1.0, 4), (0.625, 0.5, 2), (0.3125, 0.25, 2)]
    assert VA.schedule(1.0, 8.0, 1.0, 1.0, (3, 1)) == [(1.0, 8.0, 1), (0.5, 4.0, 1), (0.25, 2.0, 1), (0.125, 1.0, 1)]


# ---------------------------------------------------------------------------------------------------
# the flags
# ---------------------------------------------------------------------------------------------------
def test_flags_and_defaults_on_both_command_lines():
    from mudiff_hip import cohort, volume as V
    from mudiff_hip import volume_align as VA
    from mudiff_hip.volume_prepare import STAGES, IntakeOptions
    assert STAGES[-1].module is VA and IntakeOptions._fields[-2:] == ('align', 'denoise') and IntakeOptions().align is None
    want = dict(max_deg=20.0, max_mm=12.0, step_deg=5.0, step_mm=4.0, final_deg=0.35, final_mm=0.25, strides=(4, 2), bins=32, min_overlap=0.5)
    assert VA.DEFAULTS == want
    for build, extra in ((V.build_argparser, []), (cohort.build_argparser, ['--manifest', 'm.tsv'])):
        plain = build(VS.cli_argv(*extra))
        assert plain.align is False and IntakeOptions.from_args(plain).align is None
        assert IntakeOptions.from_args(build(VS.cli_argv('--conform', *extra))).align is None
        on = build(VS.cli_argv('--conform', '--align', *extra))
        assert IntakeOptions.from_args(on).align == want and IntakeOptions.from_args(on).conform is not None
        args = build(VS.cli_argv('--conform', '--align', '--align_max_deg', '15', '--align_max_mm', '9', '--align_step_deg', '3', '--align_step_mm',
                                 '3', '--align_final_deg', '0.5', '--align_final_mm', '0.5', '--align_strides', '3', '1', '--align_bins', '64',
                                 '--align_min_overlap', '0.6', *extra))
        assert IntakeOptions.from_args(args).align == dict(max_deg=15.0, max_mm=9.0, step_deg=3.0, step_mm=3.0, final_deg=0.5, final_mm=0.5,
                                                           strides=(3, 1), bins=64, min_overlap=0.6)
    assert VA.options_from(argparse.Namespace()) == dict(align=None)
    assert VA.options_from(argparse.Namespace(align=True, conform=True)) == dict(align=want)      # a namespace that lacks the other flags


def test_the_flags_live_in_the_late_parser_and_mix_with_the_others(capsys):
    """The main parser's option list is pinned (tests/test_volume_cli_host.py); the --align flags are parsed by VolumeParser.late."""
    from mudiff_hip import cohort, volume as V
    p = V.make_parser()
    main = [o for a in p._actions for o in a.option_strings]
    late = [o for a in p.late._actions for o in a.option_strings]
    assert not [o for o in main if o.startswith('--align')] and late[0] == '--align' and len(late) == 10 and all(o.startswith('--align') for o in late)
    assert '--align_min_overlap' in p.format_help() and '--conform_back' in p.format_help()
    args = V.build_argparser(['--align_strides', '3', '1', '--target_modality', 'T1CE', '--align', '--output_dir', 'out', '--align_max_mm', '9', '--exp', 'e',
                              '--conform', '--align_bins', '64', '--batch_size', '5'])
    assert args.align and args.conform and args.align_strides == [3, 1] and args.align_max_mm == 9.0 and args.align_bins == 64 and args.batch_size == 5
    assert args.align_max_deg == 20.0 and args.output_dir == 'out'
    for build, bad in ((V.build_argparser, ['--aling']), (cohort.build_argparser, ['--manifest', 'm.tsv', '--align_bin', '3', '--nonsense'])):
        with pytest.raises(SystemExit) as e:
            build(VS.cli_argv('--conform', *bad))
        assert e.value.code == 2 and 'unrecognized arguments' in capsys.readouterr().err


REFUSALS = [(['--align_max_deg', '0'], 'align_max_deg'), (['--align_max_deg', '90'], 'align_max_deg'), (['--align_max_mm', '-1'], 'align_max_mm'),
            (['--align_step_deg', '25'], 'align_step_deg'), (['--align_step_mm', '0'], 'align_step_mm'), (['--align_final_deg', '0'], 'align_final_deg'),
            (['--align_final_mm', 'nan'], 'align_final_mm'), (['--align_strides', '2', '4'], 'align_strides'), (['--align_strides', '0', '0'], 'align_strides'),
            (['--align_bins', '1'], 'align_bins'), (['--align_bins', '257'], 'align_bins'), (['--align_min_overlap', '0'], 'align_min_overlap'),
            (['--align_min_overlap', '1.5'], 'align_min_overlap')]


@pytest.mark.parametrize('bad, word', REFUSALS, ids=['-'.join(b[0:2]) for b, _ in REFUSALS])
def test_bad_values_are_refused_naming_the_flag(bad, word, capsys):
    from mudiff_hip import cohort, volume as V
    for build in (lambda: V.build_argparser(VS.cli_argv('--conform', '--align', *bad)),
                  lambda: cohort.build_argparser(VS.cli_argv('--manifest', 'm.tsv', '--conform', '--align', *bad))):
        with pytest.raises(SystemExit) as e:
            build()
        err = capsys.readouterr().err
        assert e.value.code == 2 and '--' + word in err and 'unrecognized' not in err      # (options_from's refusal, not an unknown flag's)


def test_align_without_conform_is_refused_naming_both_flags(capsys):
    from mudiff_hip import cohort, volume as V
    from mudiff_hip import volume_align as VA
    with pytest.raises(ValueError, match='--align needs --conform'):
        VA.options_from(argparse.Namespace(align=True))
    for build in (lambda: V.build_argparser(VS.cli_argv('--align')), lambda: cohort.build_argparser(VS.cli_argv('--manifest', 'm.tsv', '--align'))):
        with pytest.raises(SystemExit) as e:
            build()
        err = capsys.readouterr().err
        assert e.value.code == 2 and '--align' in err and '--conform' in err


def test_suffix_and_report_file(tmp_path):
    from mudiff_hip import volume_align as VA
    from mudiff_hip.volume_prepare import IntakeReport
    rep = dict(yaw_deg=6.875, roll_deg=-5.0, offset_mm=3.0, r=0.99, r_identity=0.6, overlap=0.8, candidates=677, levels=5, kept=1)
    assert VA.align_suffix([]) == '' and VA.align_suffix([('FLAIR', rep)]) == ' | align=FLAIR:6.88/-5.00deg/3.00mm'
    assert VA.align_suffix([('FLAIR', dict(rep, kept=0))]) == ' | align=FLAIR:kept=0'
    report = IntakeReport()
    assert report.suffix() == ''
    report.write(str(tmp_path / 'none'), 'T1CE', np.eye(4), None)
    assert not (tmp_path / 'none').exists()                                # nothing to report: not even the directory
    report.align.append(('FLAIR', rep))
    assert report.suffix() == ' | align=FLAIR:6.88/-5.00deg/3.00mm'
    report.write(str(tmp_path / 'out'), 'T1CE', np.eye(4), None)
    assert [p.name for p in (tmp_path / 'out').iterdir()] == ['align_t1ce.json']
    assert json.load(open(tmp_path / 'out' / 'align_t1ce.json')) == {'FLAIR': rep}


# ---------------------------------------------------------------------------------------------------
# the search over the numpy cost
# ---------------------------------------------------------------------------------------------------
def _host_search(vol, **kw):
    from mudiff_hip import volume_align as VA
    from mudiff_hip.volume_coreg import grid_centre
    A = AR.affine()
    centre = grid_centre(AR.SHAPE, A)
    assert np.allclose(centre, CENTRE)
    v = np.asarray(vol, np.float32)
    lo, scale = AR.bin_range(v, AR.BINS)
    return VA.finish(AR.host_cost(v, A, centre, lo, scale, AR.BINS), lambda s: VA.sample_points(AR.SHAPE, s), centre, **dict(AR.SEARCH, **kw))


@pytest.mark.parametrize('pose', AR.POSES)
def test_the_search_recovers_the_planted_plane(pose):
    """The bar is the method's own resolution: each angle within two final angle steps (2 x 0.3125 deg), the offset within two final
    offset steps (2 x 0.25 mm).  Measured (numpy cost, the int16 head with its lesion, 677 candidates in 5 levels):
    (7, -5, 3) -> errors 0.1875 deg, 0 deg, 0 mm; (-12, 9, -4.5) -> 0.125 deg, 0.0625 deg, 0 mm; (0, 0, 0) -> 0, 0, 0."""
    from mudiff_hip import volume_align as VA
    T, rep = _host_search(AR.phantom(pose))
    err = np.abs(np.array([rep['yaw_deg'], rep['roll_deg'], rep['offset_mm']]) - np.array(pose))
    print('pose', pose, 'found', rep['yaw_deg'], rep['roll_deg'], rep['offset_mm'], 'errors', err.tolist(), 'r', rep['r'], 'r_identity', rep['r_identity'],
          'overlap', rep['overlap'], 'candidates', rep['candidates'], 'levels', rep['levels'])
    assert rep['steps'] == [0.3125, 0.3125, 0.25] and rep['levels'] == 5 and rep['candidates'] == 9 * 9 * 7 + 4 * 27 + 2
    assert rep['kept'] == 1 and err[0] <= 2 * 0.3125 and err[1] <= 2 * 0.3125 and err[2] <= 2 * 0.25
    assert np.allclose(T, VA.pose_world((rep['yaw_deg'], rep['roll_deg'], rep['offset_mm']), CENTRE)) and np.array_equal(np.array(rep['T']), T)
    assert rep['r'] >= rep['r_identity'] and rep['overlap'] >= 0.5
    if pose != (0.0, 0.0, 0.0):
        assert rep['r'] > 0.99 and rep['r_identity'] < 0.7


def test_a_plane_outside_the_search_range_leaves_the_input_unaligned(capsys):
    T, rep = _host_search(AR.phantom((30.0, 0.0, 0.0)))
    out = capsys.readouterr().out
    print(out, rep)
    assert np.array_equal(T, np.eye(4)) and rep['kept'] == 0 and abs(rep['yaw_deg']) == 20.0 and rep['T'] == np.eye(4).tolist()
    assert out.count('[align] warning:') == 1 and 'boundary' in out and 'left unaligned' in out


def test_a_constant_volume_leaves_the_input_unaligned(capsys):
    T, rep = _host_search(np.full(AR.SHAPE, 7, np.int16))
    out = capsys.readouterr().out
    assert np.array_equal(T, np.eye(4)) and rep['kept'] == 0 and rep['r'] is None and rep['r_identity'] is None and rep['levels'] == 1
    assert (rep['yaw_deg'], rep['roll_deg'], rep['offset_mm']) == (0.0, 0.0, 0.0)
    assert out.count('[align] warning:') == 1 and 'left unaligned' in out
