"""CPU: a target acquired as accelerated thick slices (mudiff_hip.multislice): the flag checks on both command
lines, the batching it shares with mudiff_hip.thick, and the fp64 restatement of the projection (tests/multislice_ref.py) the GPU tests
compare with, together with the fp32 emulation that shows its rounding bound holds with room."""
import argparse
import re

import numpy as np
import pytest

import kspace_ref as KR
import multislice_ref as R
import thick_ref as TR
import volume_support as VS

KNOWN = ['--known_volume', 'k.nii.gz']
MS = ['--known_multislice', 'equispaced', '--multislice_thick', '3']


def test_symbol_and_kind_are_declared_and_bound():
    import mudiff_hip
    from mudiff_hip import ops
    assert 'mud_slab_kspace_constrain' in mudiff_hip.EXPORTED_SYMBOLS
    kinds = {ops.KIND_X_INIT, ops.KIND_Z, ops.KIND_NOISE, ops.KIND_KNOWN, ops.KIND_RENOISE, ops.KIND_KSPACE, ops.KIND_THICK, ops.KIND_MULTISLICE}
    assert ops.KIND_MULTISLICE == 7 and len(kinds) == 8


def test_the_mode_is_the_fourth_and_the_first_three_stay():
    from mudiff_hip import known_region, kspace, multislice, thick, volume as V
    assert V.known_modes()[:3] == (known_region, kspace, thick) and V.known_modes()[3:] == (multislice,)


def test_flags_are_parsed_and_checked():
    from mudiff_hip import cohort as Co, multislice as M, volume as V
    a = V.build_argparser(VS.cli_argv())
    assert M.options_from(a) is None and M.suffix(None) == '' and V._done_tail(a, 'auto') == ''
    a = V.build_argparser(VS.cli_argv(*KNOWN, *MS))
    assert M.options_from(a) == dict(pattern='equispaced', L=3, gap=0, offset=0, profile='box', accel=4, center=0.08, axis=0, mask_file=None,
                                     baseline=False)
    a = V.build_argparser(VS.cli_argv(*KNOWN, '--known_multislice', 'random', '--multislice_thick', '5', '--multislice_gap', '1', '--multislice_offset',
                                      '2', '--multislice_profile', 'gauss', '--multislice_accel', '2', '--multislice_center', '0.25', '--multislice_axis',
                                      '1', '--multislice_baseline', '--known_drop_slices', '2:3', '--known_resample', '2'))
    assert M.options_from(a) == dict(pattern='random', L=5, gap=1, offset=2, profile='gauss', accel=2, center=0.25, axis=1, mask_file=None,
                                     baseline=True)
    a = V.build_argparser(VS.cli_argv(*KNOWN, '--known_multislice', 'file', '--multislice_thick', '2', '--multislice_mask_file', 'm.npy'))
    assert M.options_from(a)['mask_file'] == 'm.npy'
    bad = [([f'--multislice_{f}', v], f'--multislice_{f} needs --known_multislice')
           for f, v in (('thick', '3'), ('gap', '1'), ('offset', '1'), ('profile', 'box'), ('accel', '2'), ('center', '0.1'), ('axis', '1'),
                        ('mask_file', 'm.npy'))]
    bad += [(['--multislice_baseline'], '--multislice_baseline needs --known_multislice'),
            (MS, '--known_multislice needs --known_volume'),
            (KNOWN + ['--known_multislice', 'equispaced'], '--known_multislice needs --multislice_thick'),
            (KNOWN + ['--known_multislice', 'equispaced', '--multislice_thick', '0'], '--multislice_thick must'),
            (KNOWN + ['--known_multislice', 'equispaced', '--multislice_thick', '17'], '--multislice_thick must'),
            (KNOWN + MS + ['--multislice_gap', '-1'], '--multislice_gap must'),
            (KNOWN + MS + ['--multislice_offset', '-2'], '--multislice_offset must'),
            (KNOWN + MS + ['--multislice_accel', '0'], '--multislice_accel must'),
            (KNOWN + MS + ['--multislice_center', '1.5'], '--multislice_center must'),
            (KNOWN + MS + ['--multislice_mask_file', 'm.npy'], '--multislice_mask_file goes with'),
            (KNOWN + ['--known_multislice', 'file', '--multislice_thick', '3'], '--multislice_mask_file goes with'),
            (KNOWN + MS + ['--image_size', '24'], '--known_multislice needs an --image_size'),
            (KNOWN + MS + ['--seed', '-1'], '--known_multislice needs a --seed'),
            (KNOWN + MS + ['--known_mask', 'm.nii.gz'], '--known_multislice cannot be combined with --known_mask'),
            (KNOWN + MS + ['--known_kspace', 'random'], '--known_multislice cannot be combined with --known_kspace'),
            (KNOWN + MS + ['--known_thick', '3'], '--known_multislice cannot be combined with --known_thick')]
    for argv, msg in bad:
        for parser, more in ((V, []), (Co, ['--manifest', 'c.tsv'])):          # both command lines
            if parser is Co and msg.endswith('needs --known_volume'):
                continue                                                     # (a cohort's K is the manifest's `known` column)
            if parser is V:
                with pytest.raises(ValueError, match=re.escape(msg)):
                    M.options_from(parser.make_parser().parse_args(VS.cli_argv(*argv, *more)))
            with pytest.raises(SystemExit):                                  # the command line refuses it before anything is read
                parser.build_argparser(VS.cli_argv(*argv, *more))
    # a cohort takes K from its manifest and the --multislice_* flags from the command line
    c = Co.build_argparser(VS.cli_argv('--manifest', 'c.tsv', '--known_multislice', 'lowres', '--multislice_thick', '4', '--multislice_gap', '2'))
    assert M.options_from(c)['L'] == 4 and M.options_from(c)['gap'] == 2 and M.options_from(c)['pattern'] == 'lowres'


def test_flag_errors_name_the_flag_on_the_command_line(capsys):
    from mudiff_hip import cohort as Co, volume as V
    for parser, more in ((V, []), (Co, ['--manifest', 'c.tsv'])):
        with pytest.raises(SystemExit):
            parser.build_argparser(VS.cli_argv('--multislice_gap', '1', *more))
        assert '--multislice_gap needs --known_multislice' in capsys.readouterr().err
        with pytest.raises(SystemExit):
            parser.build_argparser(VS.cli_argv(*KNOWN, *MS, '--known_thick', '3', *more))
        assert '--known_multislice cannot be combined with --known_thick' in capsys.readouterr().err
        with pytest.raises(SystemExit):                                        # the older pair stays refused in its own words
            parser.build_argparser(VS.cli_argv(*KNOWN, '--known_thick', '3', '--known_kspace', 'random', *more))
        assert '--known_thick cannot be combined with --known_kspace (in-plane undersampling of thick slices is out of scope)' in capsys.readouterr().err


def test_the_older_modes_give_none_on_a_namespace_of_this_mode_alone():
    from mudiff_hip import known_region, kspace, multislice as M, thick
    ns = argparse.Namespace(known_multislice='equispaced', multislice_thick=3)
    for module in (known_region, kspace, thick):
        assert module.options_from(ns) is None
    assert M.options_from(argparse.Namespace()) is None
    with pytest.raises(ValueError, match='--known_multislice needs --known_volume'):
        M.options_from(ns)


def _measurement(n, starts, L, S=2):
    import torch
    from mudiff_hip import multislice as M, thick as TK
    y = torch.arange(len(starts) * S * S, dtype=torch.float32).view(len(starts), S, S).to(torch.complex64)
    mask = torch.ones(1, S, S, dtype=torch.uint8)
    report = dict(L=L, gap=1, profile='box', pattern='equispaced', accel=2, measured_slabs=len(starts), slabs=[{}] * (len(starts) + 1))
    return M.MultisliceMeasurement(y, mask, starts, n, TK.profile_weights(L).astype(np.float32), report, 1, dict(baseline=False))


def test_units_chunks_and_tables_are_those_of_thick_slices():
    from mudiff_hip import constraints as Cn, thick as TK
    m = _measurement(12, [0, 4, 8], 3)                              # slices 3, 7, 11 are gap slices
    assert m.tag == 'multislice' and m.baseline_through_plane and m.baseline() is None
    assert m.done_suffix() == ' | multislice=3+1 box equispaced x2 (3/4 slabs)'
    assert m.units() == [[0, 1, 2], [3], [4, 5, 6], [7], [8, 9, 10], [11]]
    assert TK.batches(m.units(), 7) == [[0, 1, 2, 3, 4, 5, 6], [7, 8, 9, 10, 11]]
    assert TK.batches(m.units(), 5) == [[0, 1, 2, 3], [4, 5, 6, 7], [8, 9, 10, 11]]        # closed early before a slab that would not fit
    with pytest.raises(ValueError, match='--batch_size 2 '):
        TK.batches(m.units(), 2)
    with pytest.raises(ValueError, match='cuts the measured slab'):
        m.units(0, 5)
    assert m.units(3, 8) == [[3], [4, 5, 6], [7]]
    assert m.chunk_end(0, 5) == 4 and m.chunk_end(0, 4) == 4 and m.chunk_end(4, 12) == 12
    with pytest.raises(ValueError, match='smaller than a slab'):
        m.chunk_end(4, 6)
    bound = m.for_rows([4, 5, 6, 7, -1, -1])                                    # a padded row is in no group
    assert isinstance(bound, Cn.SlabKSpaceRows)
    (y, mask, members, w, g), gids = bound
    assert members.tolist() == [[0, 1, 2]] and gids.tolist() == [1] and np.array_equal(y.numpy(), m.y[1:2].numpy()) and mask is m.mask
    assert np.array_equal(w, np.full(3, 1 / 3, np.float32)) and np.array_equal(g, TR.gains(w))
    (y, _, members, _, _), gids = m.for_rows([8, 9, 10, 10, 9, 8, 11], [0, 0, 0, 1, 1, 1, 0])      # an ensemble's batch, rows out of order
    assert members.tolist() == [[0, 1, 2], [5, 4, 3]] and gids.tolist() == [2, 2]
    (y, _, members, _, _), gids = m.for_rows([3, 7, -1])
    assert members.shape == (0, 3) and gids.numel() == 0 and y.shape == (0, 2, 2)
    with pytest.raises(ValueError, match='2 of the 3 thin slices'):
        m.for_rows([4, 5, 7])
    # the thick measurement built from the same layout gives the same units, chunk ends and member tables
    t = TK.ThickMeasurement(m.y.real.contiguous(), [0, 4, 8], 12, m.weights, dict(slabs=[]), 1, dict(interp=False))
    assert t.units() == m.units() and all(t.chunk_end(0, e) == m.chunk_end(0, e) for e in range(3, 12))
    assert t.for_rows([4, 5, 6, 7])[0][1].tolist() == m.for_rows([4, 5, 6, 7])[0][2].tolist()


def _case(g, S, L, kind, groups=2, free=3):
    w = TR.profile(L, kind)
    rows = groups * L + free
    members = np.stack([np.arange(L) * groups + j for j in range(groups)])      # interleaved groups, then the free rows
    k, x = np.tanh(g.standard_normal((rows, S, S))), g.standard_normal((rows, S, S))
    mask = KR.symmetrise((g.random((1, S, S)) < 0.3).astype(np.uint8))
    assert 0 < mask.sum() < mask.size
    return w, w / (w * w).sum(), members, k, x, mask


def test_the_restatements_projection():
    g = np.random.default_rng(5)
    S = 16
    for L, kind in ((1, 'box'), (3, 'box'), (5, 'gauss'), (16, 'gauss')):
        w, gn, members, k, x, mask = _case(g, S, L, kind)
        on = mask[0] != 0
        y = R.measure(k, members, w, mask)
        out = R.constrain(x, y, mask, members, w, gn, None, None, 0, None, None, True)
        Fo, Fx = KR.fft2(TR.average(out, members, w)), KR.fft2(TR.average(x, members, w))
        assert np.abs((Fo - y)[:, on]).max() <= 1e-12                          # the clean step meets y on the measured coefficients
        assert np.abs((Fo - Fx)[:, ~on]).max() <= 1e-12                        # the unmeasured ones of the slab average are unchanged
        assert np.array_equal(out[2 * L:], x[2 * L:])                          # free rows
        again = R.constrain(out, y, mask, members, w, gn, None, None, 0, None, None, True)
        assert np.abs(again - out).max() <= 1e-12                              # idempotent
        if L > 1:                                                              # components orthogonal to w are unchanged
            v = g.standard_normal((L, S, S))
            v -= w[:, None, None] * (w[:, None, None] * v).sum(0) / (w * w).sum()
            for grp in members:
                assert np.abs((v * (out[grp] - x[grp])).sum(0)).max() <= 1e-12
        # a noise level gives a y + s F(sum_l w_l eta_l) on the measured coefficients
        a_tab, s_tab = np.array([1.0, 0.8, 0.3]), np.array([0.0, 0.6, np.sqrt(1 - 0.09)])
        eta, t = g.standard_normal(x.shape), np.full(x.shape[0], 1)
        for toff in (0, 1):
            out = R.constrain(x, y, mask, members, w, gn, eta, t, toff, a_tab, s_tab, False)
            want = a_tab[1 + toff] * y + s_tab[1 + toff] * KR.fft2(TR.average(eta, members, w))
            assert np.abs((KR.fft2(TR.average(out, members, w)) - want)[:, on]).max() <= 1e-12
        # the level is the first member's
        t2 = t.copy()
        t2[members[:, 1:].ravel()] = 0
        assert np.array_equal(R.constrain(x, y, mask, members, w, gn, eta, t2, 0, a_tab, s_tab, False),
                              R.constrain(x, y, mask, members, w, gn, eta, t, 0, a_tab, s_tab, False))


def test_the_restatement_reduces_to_its_two_parents():
    g = np.random.default_rng(6)
    S = 16
    a_tab, s_tab = np.array([1.0, 0.8, 0.3]), np.array([0.0, 0.6, np.sqrt(1 - 0.09)])
    # L = 1, w = g = 1: kspace_ref.constrain on those rows
    w, gn, members, k, x, mask = _case(g, S, 1, 'box', groups=3, free=0)
    eta, t = g.standard_normal(x.shape), np.array([0, 1, 5])
    y = R.measure(k, members, w, mask)
    for clean in (False, True):
        got = R.constrain(x, y, mask, members, w, gn, eta, t, 0, a_tab, s_tab, clean)
        assert np.abs(got - KR.constrain(x, y, mask, eta, t, 0, a_tab, s_tab, clean)).max() <= 1e-12
    # a mask of ones: thick_ref.constrain with the image-domain measurement Re F^H y
    w, gn, members, k, x, _ = _case(g, S, 5, 'gauss')
    ones = np.ones((1, S, S), np.uint8)
    eta, t = g.standard_normal(x.shape), np.full(x.shape[0], 1)
    y = R.measure(k, members, w, ones)
    yi = KR.fft2(y, inverse=True).real
    assert np.abs(yi - TR.average(k, members, w)).max() <= 1e-12
    for clean in (False, True):
        got = R.constrain(x, y, ones, members, w, gn, eta, t, 0, a_tab, s_tab, clean)
        assert np.abs(got - TR.constrain(x, yi, members, w, gn, eta, t, 0, a_tab, s_tab, clean)).max() <= 1e-12


def test_the_fp32_transform_of_the_emulation_is_a_transform():
    g = np.random.default_rng(7)
    for S in (16, 32):
        z = g.standard_normal((S, S)) + 1j * g.standard_normal((S, S))
        for inverse in (False, True):
            re, im = R.fft2_f32(z.real, z.imag, inverse)
            want = KR.fft2(z.astype(np.complex64), inverse)
            err = np.sqrt((np.abs(re + 1j * im - want) ** 2).sum() / (np.abs(want) ** 2).sum())
            assert re.dtype == np.float32 and err <= KR.rule(S), (S, inverse, err)


@pytest.mark.parametrize('S', (16, 32, 256))
@pytest.mark.parametrize('kind', ('box', 'gauss'))
def test_an_fp32_emulation_stays_below_six_tenths_of_the_bound(kind, S):
    """The bound the GPU tests hold the kernel to adds kspace's 3 rule(S) to thick's rounding count; the same chain in numpy fp32 on
    N(0,1) data uses at most 0.6 of it, for every L."""
    g = np.random.default_rng(11 + S)
    worst = 0.0
    mask = KR.symmetrise((g.random((1, S, S)) < 0.3).astype(np.uint8))
    a, s = np.float32(0.8), np.float32(0.6)
    for L in range(1, 17):
        w = TR.profile(L, kind).astype(np.float32)
        gn = TR.gains(w)
        members = np.arange(L)[None]
        x, eta, k = (g.standard_normal((L, S, S)).astype(np.float32) for _ in range(3))
        y = R.measure(k, members, w, mask).astype(np.complex64)
        t = np.zeros(L, np.int64)
        for clean in (False, True):
            got = R.emulate_fp32(x, y[0], mask, w, gn, eta, a, s, clean)
            ref = R.constrain(x, y, mask, members, w, gn, eta, t, 0, [a], [s], clean)
            bound = R.bound(x, y, members, w, gn, eta, t, 0, [a], [s], clean)
            err = np.sqrt(((got - ref) ** 2).sum((1, 2)))
            worst = max(worst, float((err / bound).max()))
    print(f'{kind} S={S}: worst |out - ref| / bound {worst:.3f}')
    assert worst <= 0.6


def test_the_baseline_of_the_restatement():
    g = np.random.default_rng(8)
    S, L, starts, n = 16, 3, [0, 4, 8], 12
    mask = KR.symmetrise((g.random((1, S, S)) < 0.4).astype(np.uint8))
    k = np.tanh(g.standard_normal((n, S, S)))
    members = np.asarray([list(range(s, s + L)) for s in starts])
    y = R.measure(k, members, TR.profile(L), mask)
    got = R.baseline(y, starts, L, n)
    z = KR.fft2(y, inverse=True).real
    assert np.abs(got[1] - z[0]).max() <= 1e-15 and np.abs(got[3] - 0.5 * (z[0] + z[1])).max() <= 1e-15 and np.abs(got[11] - z[2]).max() <= 1e-15
    ones = R.measure(k, members, TR.profile(L), np.ones((1, S, S), np.uint8))   # fully sampled: thick's interpolated baseline
    assert np.abs(R.baseline(ones, starts, L, n) - TR.interpolate(TR.average(k, members, TR.profile(L)), starts, L, n)).max() <= 1e-12
