"""CPU: a target acquired with thick slices (mudiff_hip.thick): the layout, the profiles, the flag checks, the
batching that keeps a measured slab whole, and the fp64 restatement of the projection (tests/thick_ref.py) the GPU tests compare with,
together with the fp32 emulation that shows its rounding bounds hold with room."""
import argparse
import re

import numpy as np
import pytest

import thick_ref as R
import volume_support as VS

SYMBOLS = ('mud_slab_constrain', 'mud_slab_average')


def test_symbols_are_declared_and_bound():
    import mudiff_hip
    from mudiff_hip import ops, thick as TK
    assert all(s in mudiff_hip.EXPORTED_SYMBOLS for s in SYMBOLS)
    kinds = {ops.KIND_X_INIT, ops.KIND_Z, ops.KIND_NOISE, ops.KIND_KNOWN, ops.KIND_RENOISE, ops.KIND_KSPACE, ops.KIND_THICK}
    assert ops.KIND_THICK == 6 and len(kinds) == 7 and ops.SLAB_MAX_MEMBERS == TK.MAX_L == 16


@pytest.mark.parametrize('Z,L,G,O,want', [
    (12, 3, 1, 0, [(0, 2, True), (4, 6, True), (8, 10, True)]),
    (12, 3, 1, 1, [(1, 3, True), (5, 7, True), (9, 11, True)]),
    (12, 3, 1, 2, [(2, 4, True), (6, 8, True), (10, 11, False)]),              # a partial tail
    (10, 5, 0, 0, [(0, 4, True), (5, 9, True)]),
    (11, 5, 0, 0, [(0, 4, True), (5, 9, True), (10, 10, False)]),
    (4, 1, 0, 0, [(z, z, True) for z in range(4)]),                            # L = 1: every slice its own slab
    (5, 1, 1, 1, [(1, 1, True), (3, 3, True)]),
    (3, 16, 0, 0, [(0, 2, False)]),
    (6, 2, 3, 7, []),
])
def test_layout(Z, L, G, O, want):
    from mudiff_hip import thick as TK
    assert TK.layout(Z, L, G, O) == want == R.layout(Z, L, G, O)
    full = [s for s in want if s[2]]
    assert all(b - a + 1 == L for a, b, _ in full) and all(n[0] - p[0] == L + G for p, n in zip(want, want[1:]))


@pytest.mark.parametrize('L', range(1, 17))
def test_profiles_sum_to_one_and_gauss_is_symmetric(L):
    from mudiff_hip import thick as TK
    for kind in ('box', 'gauss'):
        w = TK.profile_weights(L, kind)
        assert w.dtype == np.float64 and w.shape == (L,) and (w > 0).all() and abs(w.sum() - 1.0) <= 1e-15
        assert np.array_equal(w, w[::-1]) and np.abs(w - R.profile(L, kind)).max() <= 1e-15
    assert np.array_equal(TK.profile_weights(L, 'box'), np.full(L, 1.0 / L))
    g = TK.profile_weights(L, 'gauss')
    d = np.arange(L) - (L - 1) / 2.0                                # FWHM = L slices: exp(-4 ln 2 d^2 / L^2) is 1/2 at d = L / 2
    assert np.abs(g / g[0] - np.exp(-4 * np.log(2) * (d * d - d[0] * d[0]) / L ** 2)).max() <= 1e-12
    if L > 2:
        assert g[L // 2] > g[0] > 0.5 * g[L // 2]                   # the profile's ends lie inside the half maximum
    with pytest.raises(ValueError):
        TK.profile_weights(17)


def test_flags_are_parsed_and_checked():
    from mudiff_hip import cohort as Co, thick as TK, volume as V
    a = V.build_argparser(VS.cli_argv())
    assert TK.options_from(a) is None and TK.suffix(None) == '' and V._done_tail(a, 'auto') == ''
    a = V.build_argparser(VS.cli_argv('--known_volume', 'k.nii.gz', '--known_thick', '5'))
    assert TK.options_from(a) == dict(L=5, gap=0, offset=0, profile='box', interp=False)
    a = V.build_argparser(VS.cli_argv('--known_volume', 'k.nii.gz', '--known_thick', '3', '--thick_gap', '1', '--thick_offset', '2', '--thick_profile',
                                      'gauss', '--thick_interp', '--known_drop_slices', '2:3', '--known_resample', '2'))
    assert TK.options_from(a) == dict(L=3, gap=1, offset=2, profile='gauss', interp=True)
    known = ['--known_volume', 'k.nii.gz']
    bad = [(['--thick_gap', '1'], '--thick_gap needs --known_thick'), (['--thick_offset', '1'], '--thick_offset needs --known_thick'),
           (['--thick_profile', 'box'], '--thick_profile needs --known_thick'), (['--thick_interp'], '--thick_interp needs --known_thick'),
           (['--known_thick', '3'], '--known_thick needs --known_volume'),
           (known + ['--known_thick', '0'], '--known_thick must'), (known + ['--known_thick', '17'], '--known_thick must'),
           (known + ['--known_thick', '3', '--thick_gap', '-1'], '--thick_gap must'),
           (known + ['--known_thick', '3', '--thick_offset', '-2'], '--thick_offset must'),
           (known + ['--known_thick', '3', '--known_kspace', 'random'], '--known_thick cannot be combined with --known_kspace'),
           (known + ['--known_thick', '3', '--known_mask', 'm.nii.gz'], '--known_thick cannot be combined with --known_mask')]
    for argv, msg in bad:
        for parser, more in ((V, []), (Co, ['--manifest', 'c.tsv'])):          # both command lines
            if parser is Co and msg.endswith('needs --known_volume'):
                continue                                                     # (a cohort's K is the manifest's `known` column)
            ns = parser.make_parser().parse_args(VS.cli_argv(*argv, *more)) if parser is V else None
            if ns is not None:
                with pytest.raises(ValueError, match=re.escape(msg)):
                    TK.options_from(ns)
            with pytest.raises(SystemExit):                                  # the command line refuses it before anything is read
                parser.build_argparser(VS.cli_argv(*argv, *more))
    # a cohort takes K from its manifest and the --thick_* flags from the command line
    c = Co.build_argparser(VS.cli_argv('--manifest', 'c.tsv', '--known_thick', '4', '--thick_gap', '2'))
    assert TK.options_from(c) == dict(L=4, gap=2, offset=0, profile='box', interp=False)


def test_flag_errors_name_the_flag_on_the_command_line(capsys):
    from mudiff_hip import cohort as Co, volume as V
    for parser, more in ((V, []), (Co, ['--manifest', 'c.tsv'])):
        with pytest.raises(SystemExit):
            parser.build_argparser(VS.cli_argv('--thick_gap', '1', *more))
        assert '--thick_gap needs --known_thick' in capsys.readouterr().err


def test_a_namespace_of_the_older_parser_gives_none():
    from mudiff_hip import thick as TK, volume as V
    assert TK.options_from(argparse.Namespace()) is None
    a = V.build_argparser(VS.cli_argv('--known_volume', 'k.nii.gz'))
    for k in [k for k in vars(a) if k.startswith(('known_thick', 'thick_'))]:
        delattr(a, k)
    assert TK.options_from(a) is None and V._done_tail(a, 'auto') == ''


def _measurement(n, starts, L):
    import torch
    from mudiff_hip import thick as TK
    y = torch.arange(len(starts) * 4, dtype=torch.float32).view(len(starts), 2, 2)
    return TK.ThickMeasurement(y, starts, n, TK.profile_weights(L).astype(np.float32), dict(slabs=[]), 1, dict(interp=False))


def test_batches_never_split_a_measured_slab():
    from mudiff_hip import thick as TK
    m = _measurement(12, [0, 4, 8], 3)                              # slices 3, 7, 11 are gap slices
    assert m.units() == [[0, 1, 2], [3], [4, 5, 6], [7], [8, 9, 10], [11]]
    assert TK.batches(m.units(), 7) == [[0, 1, 2, 3, 4, 5, 6], [7, 8, 9, 10, 11]]
    assert TK.batches(m.units(), 4) == [[0, 1, 2, 3], [4, 5, 6, 7], [8, 9, 10, 11]]
    assert TK.batches(m.units(), 5) == [[0, 1, 2, 3], [4, 5, 6, 7], [8, 9, 10, 11]]        # closed early before a slab that would not fit
    assert TK.batches(m.units(), 3) == [[0, 1, 2], [3], [4, 5, 6], [7], [8, 9, 10], [11]]
    for B in range(3, 14):
        got = TK.batches(m.units(), B)
        assert sum(got, []) == list(range(12)) and all(len(b) <= B for b in got)
        assert all(sum(z in b for b in got for z in range(s, s + 3)) == 3 and sum(any(z in b for z in range(s, s + 3)) for b in got) == 1
                   for s in (0, 4, 8))
    with pytest.raises(ValueError, match='--batch_size 2 '):
        TK.batches(m.units(), 2)
    with pytest.raises(ValueError, match='cuts the measured slab'):
        m.units(0, 5)
    assert m.units(3, 8) == [[3], [4, 5, 6], [7]]
    free = _measurement(5, [], 3)                                   # nothing measured: the plain order
    assert TK.batches(free.units(), 2) == [[0, 1], [2, 3], [4]]


def test_for_rows_builds_the_tables_in_slice_order():
    m = _measurement(12, [0, 4, 8], 3)
    (y, members, w, g), gids = m.for_rows([4, 5, 6, 7, -1, -1])                # a padded row is in no group
    assert members.tolist() == [[0, 1, 2]] and gids.tolist() == [1] and y.shape == (1, 2, 2) and np.array_equal(y.numpy(), m.y[1:2].numpy())
    assert np.array_equal(w, np.full(3, 1 / 3, np.float32)) and np.array_equal(g, R.gains(w))
    # an ensemble's batch: two samples of one slab, and rows in another order than the slices
    (y, members, _, _), gids = m.for_rows([8, 9, 10, 10, 9, 8, 11], [0, 0, 0, 1, 1, 1, 0])
    assert members.tolist() == [[0, 1, 2], [5, 4, 3]] and gids.tolist() == [2, 2]
    (y, members, _, _), gids = m.for_rows([3, 7, -1])
    assert members.shape == (0, 3) and gids.numel() == 0 and y.shape == (0, 2, 2)
    with pytest.raises(ValueError, match='2 of the 3 thin slices'):
        m.for_rows([4, 5, 7])


def test_the_restatements_projection():
    g = np.random.default_rng(5)
    for L, kind in ((1, 'box'), (3, 'box'), (5, 'gauss'), (16, 'gauss')):
        w = R.profile(L, kind)
        gn = w / (w * w).sum()                                      # fp64 gains: the restatement's own properties
        rows, n = 2 * L + 3, 33
        members = np.stack([np.arange(L) * 2, np.arange(L) * 2 + 1])             # two interleaved groups and three free rows
        k, x = np.tanh(g.standard_normal((rows, n))), g.standard_normal((rows, n))
        y = R.average(k, members, w)
        out = R.constrain(x, y, members, w, gn, None, None, 0, None, None, True)
        assert np.abs(R.average(out, members, w) - y).max() <= 1e-12          # the clean step meets y
        assert np.array_equal(out[2 * L:], x[2 * L:])                          # free rows
        again = R.constrain(out, y, members, w, gn, None, None, 0, None, None, True)
        assert np.abs(again - out).max() <= 1e-12                              # idempotent
        if L > 1:                                                              # components orthogonal to w are unchanged
            v = g.standard_normal((L, n))
            v -= w[:, None] * (w[:, None] * v).sum(0) / (w * w).sum()
            assert np.abs((w[:, None] * v).sum(0)).max() <= 1e-12
            for grp in members:
                assert np.abs((v * (out[grp] - x[grp])).sum(0)).max() <= 1e-12
        # a noise level gives the slab average of q_sample(k)
        a_tab, s_tab = np.array([1.0, 0.8, 0.3]), np.array([0.0, 0.6, np.sqrt(1 - 0.09)])
        eta, t = g.standard_normal((rows, n)), np.full(rows, 1)
        out = R.constrain(x, y, members, w, gn, eta, t, 0, a_tab, s_tab, False)
        q = a_tab[1] * k + s_tab[1] * eta
        assert np.abs(R.average(out, members, w) - R.average(q, members, w)).max() <= 1e-12
        out1 = R.constrain(x, y, members, w, gn, eta, t, 1, a_tab, s_tab, False)
        assert np.abs(R.average(out1, members, w) - R.average(a_tab[2] * k + s_tab[2] * eta, members, w)).max() <= 1e-12


@pytest.mark.parametrize('kind', ('box', 'gauss'))
def test_an_fp32_emulation_stays_below_six_tenths_of_the_bounds(kind):
    """The bounds the GPU tests hold the kernel to count the roundings of its chain; the same chain in numpy fp32 on N(0,1) data
    uses at most 0.6 of each, for every L."""
    g = np.random.default_rng(11)
    n, worst = 4096, [0.0, 0.0]
    for L in range(1, 17):
        w = R.profile(L, kind).astype(np.float32)
        gn = R.gains(w)
        members = np.arange(L)[None]
        x, eta, k = (g.standard_normal((L, n)).astype(np.float32) for _ in range(3))
        y = R.average(k, members, w).astype(np.float32)
        a, s = np.float32(0.8), np.float32(0.6)
        for clean in (False, True):
            got = R.emulate_fp32(x, y[0], w, gn, eta, a, s, clean)
            ref = R.constrain(x, y, members, w, gn, eta, np.zeros(L, np.int64), 0, [a], [s], clean)
            bound = R.bound_out(x, y, members, w, gn, eta, np.zeros(L, np.int64), 0, [a], [s], clean)
            worst[0] = max(worst[0], float((np.abs(got - ref) / bound).max()))
            if clean:
                res = np.abs(R.average(got, members, w) - y.astype(np.float64))
                worst[1] = max(worst[1], float((res / R.bound_residual(x, y, members, w)).max()))
    print(f'{kind}: worst |out - ref| / bound {worst[0]:.3f}, worst clean residual / bound {worst[1]:.3f}')
    assert worst[0] <= 0.6 and worst[1] <= 0.6


def test_the_interpolated_baseline_of_the_restatement():
    y = np.array([[1.0], [3.0], [-1.0]])
    got = R.interpolate(y, [0, 4, 8], 3, 12)[:, 0]                  # centres 1, 5, 9
    assert np.allclose(got, [1, 1, 1.5, 2, 2.5, 3, 2, 1, 0, -1, -1, -1], atol=1e-15)
    m = _measurement(12, [0, 4, 8], 3)
    assert np.abs(m.interpolated().numpy() - R.interpolate(m.y.numpy(), [0, 4, 8], 3, 12)).max() <= 1e-5
    one = _measurement(6, [2], 3)
    assert np.array_equal(one.interpolated().numpy(), np.broadcast_to(one.y.numpy(), (6, 2, 2)))
