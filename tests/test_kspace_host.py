"""CPU: the k-space measurement of a partly acquired target (mudiff_hip.kspace): the mask builders, the flag
checks, and the fp64 restatement of the data-consistency step (tests/kspace_ref.py) the GPU tests compare with."""
import re

import numpy as np
import pytest

import kspace_ref as R
import volume_support as VS

SYMBOLS = ('mud_fft2_c2c', 'mud_fft2_r2c', 'mud_kspace_constrain')


def test_symbols_are_declared_and_bound():
    import mudiff_hip
    from mudiff_hip import ops
    assert all(s in mudiff_hip.EXPORTED_SYMBOLS for s in SYMBOLS)
    assert ops.KIND_KSPACE == 5 and len({ops.KIND_X_INIT, ops.KIND_Z, ops.KIND_NOISE, ops.KIND_KNOWN, ops.KIND_RENOISE, ops.KIND_KSPACE}) == 6
    assert [S for S in range(1, 2049) if ops.kspace_size_ok(S)] == [16, 32, 64, 128, 256, 512]


@pytest.mark.parametrize('accel', (1, 4, 8))
@pytest.mark.parametrize('pattern', ('equispaced', 'random'))
def test_line_masks_have_the_centre_block_and_the_expected_line_count(pattern, accel):
    from mudiff_hip import kspace as KS
    S, F = 256, 0.08
    for axis in (0, 1):
        m = KS.build_mask(S, pattern, accel, F, axis, seed=7)
        assert m.dtype == np.uint8 and m.shape == (S, S) and set(np.unique(m)) <= {0, 1}
        lines = R.lines_of(m, axis)                                   # (asserts that whole lines of the other axis are measured)
        centre = R.center_lines(S, F)
        assert int(centre.sum()) == 20 and centre[S // 2] and (lines & centre).sum() == 20
        outside = int((lines & ~centre).sum())
        if accel == 1:
            assert lines.all()
        elif pattern == 'equispaced':                                 # every accel-th line, from one offset below accel
            picked = np.flatnonzero(lines & ~centre)
            assert len({int(v) % accel for v in picked}) == 1 and outside == S // accel - int(centre[picked[0] % accel::accel].sum())
        else:                                                         # S / accel lines in expectation: binomial, 5 sigma
            p = (S / accel - 20) / (S - 20)
            assert abs(outside - p * (S - 20)) <= 5 * np.sqrt(p * (1 - p) * (S - 20))
        assert m[0, 0] == 1                                           # DC is measured, and it sits at [0, 0]
        assert np.array_equal(m, KS.build_mask(S, pattern, accel, F, axis, seed=7))
    if accel > 1:
        seeds = [KS.build_mask(S, pattern, accel, F, 0, seed=s).tobytes() for s in range(8)]
        assert len(set(seeds)) > 1                                    # the seed matters, and only the seed


def test_lowres_and_file_masks_put_dc_at_the_origin():
    from mudiff_hip import kspace as KS
    S = 32
    m = KS.build_mask(S, 'lowres', center=0.25)
    assert int(m.sum()) == 64 and m[0, 0] == 1
    c = np.fft.fftshift(m)
    assert c[12:20, 12:20].all() and int(c.sum()) == 64
    centred = np.zeros((S, S), np.uint8)
    centred[S // 2, S // 2] = 1                                       # DC alone ...
    centred[S // 2 + 3, S // 2 - 2] = 5                               # ... and frequency (+3, -2); non-zero = measured
    m = KS.build_mask(S, 'file', mask_file=centred)
    assert m[0, 0] == 1 and m[3, S - 2] == 1 and int(m.sum()) == 2
    with pytest.raises(ValueError, match='--kspace_mask_file'):
        KS.build_mask(16, 'file', mask_file=centred)


def test_file_mask_is_read_from_npy(tmp_path):
    from mudiff_hip import kspace as KS
    centred = (np.random.default_rng(0).random((16, 16)) < 0.3).astype(np.uint8)
    np.save(tmp_path / 'm.npy', centred)
    assert np.array_equal(KS.build_mask(16, 'file', mask_file=str(tmp_path / 'm.npy')), np.fft.ifftshift(centred))


def test_symmetrisation_is_idempotent_and_never_loses_a_coefficient():
    from mudiff_hip import kspace as KS
    g = np.random.default_rng(3)
    for S in (16, 32):
        for density in (0.05, 0.4):
            m = (g.random((S, S)) < density).astype(np.uint8)
            e = KS.symmetrise(m)
            assert np.array_equal(e, R.symmetrise(m)) and np.array_equal(KS.symmetrise(e), e)
            assert (e >= m).all() and e.mean() >= m.mean()
            u, v = np.nonzero(e)
            assert e[(-u) % S, (-v) % S].all()
    for axis in (0, 1):                                               # a line mask's mirror lines join it
        m = KS.build_mask(64, 'equispaced', 4, 0.08, axis, seed=1)
        assert KS.symmetrise(m).mean() >= m.mean()


def test_flags_are_parsed_and_checked():
    from mudiff_hip import cohort as Co, kspace as KS, volume as V
    a = V.build_argparser(VS.cli_argv())
    assert KS.options_from(a) is None and KS.suffix(None) == '' and V._done_tail(a, 'auto') == ''
    a = V.build_argparser(VS.cli_argv('--known_volume', 'k.nii.gz', '--known_kspace', 'equispaced'))
    assert KS.options_from(a) == dict(pattern='equispaced', accel=4, center=0.08, axis=0, mask_file=None, zero_filled=False)
    a = V.build_argparser(VS.cli_argv('--known_volume', 'k.nii.gz', '--known_kspace', 'lowres', '--kspace_center', '0.25', '--kspace_axis', '1',
                                      '--kspace_accel', '8', '--kspace_zero_filled', '--known_drop_slices', '2:3', '--image_size', '64'))
    assert KS.options_from(a) == dict(pattern='lowres', accel=8, center=0.25, axis=1, mask_file=None, zero_filled=True)
    known = ['--known_volume', 'k.nii.gz']
    bad = [(['--kspace_accel', '2'], '--kspace_accel needs --known_kspace'), (['--kspace_center', '0.1'], '--kspace_center needs --known_kspace'),
           (['--kspace_axis', '1'], '--kspace_axis needs'), (['--kspace_mask_file', 'm.npy'], '--kspace_mask_file needs'),
           (['--kspace_zero_filled'], '--kspace_zero_filled needs'), (['--known_kspace', 'random'], '--known_kspace needs --known_volume'),
           (known + ['--known_kspace', 'random', '--known_mask', 'm.nii.gz'], '--known_kspace cannot be combined with --known_mask'),
           (known + ['--known_kspace', 'random', '--image_size', '24'], '--image_size that is a power of two'),
           (known + ['--known_kspace', 'random', '--image_size', '1024'], '--image_size that is a power of two'),
           (known + ['--known_kspace', 'random', '--kspace_accel', '0'], '--kspace_accel must'),
           (known + ['--known_kspace', 'random', '--kspace_center', '1.5'], '--kspace_center must'),
           (known + ['--known_kspace', 'file'], '--kspace_mask_file'),
           (known + ['--known_kspace', 'random', '--kspace_mask_file', 'm.npy'], '--kspace_mask_file')]
    for argv, msg in bad:
        ns = V.make_parser().parse_args(VS.cli_argv(*argv))
        with pytest.raises(ValueError, match=re.escape(msg)):
            KS.options_from(ns)
        with pytest.raises(SystemExit):                               # the command line refuses it before anything is read
            V.build_argparser(VS.cli_argv(*argv))
    # a cohort takes K from its manifest and the --kspace_* flags from the command line
    c = Co.build_argparser(VS.cli_argv('--manifest', 'c.tsv', '--known_kspace', 'random', '--kspace_accel', '8'))
    assert KS.options_from(c)['accel'] == 8


def test_the_restatements_clean_step_meets_the_measurements():
    g = np.random.default_rng(5)
    for S, rows in ((16, 3), (32, 2)):
        k = np.tanh(g.standard_normal((rows, S, S)))
        x = g.standard_normal((rows, S, S))
        m = R.symmetrise((g.random((1, S, S)) < 0.3).astype(np.uint8))
        y = R.measure(k, m)
        out = R.constrain(x, y, m, None, None, 0, None, None, True)
        F = R.fft2(out)
        assert np.abs(np.where(m != 0, F - y, 0)).max() <= 1e-12
        assert np.abs(np.where(m == 0, F - R.fft2(x), 0)).max() <= 1e-12
        # at a noise level the measured coefficients are those of q_sample(k), the others those of x
        a_tab, s_tab = np.array([1.0, 0.8, 0.3]), np.array([0.0, 0.6, np.sqrt(1 - 0.09)])
        eta, t = g.standard_normal((rows, S, S)), np.arange(rows) % 3
        out = R.constrain(x, y, m, eta, t, 0, a_tab, s_tab, False)
        q = a_tab[t][:, None, None] * k + s_tab[t][:, None, None] * eta
        assert np.abs(np.where(m != 0, R.fft2(out) - R.fft2(q), 0)).max() <= 1e-12
        assert np.abs(np.where(m == 0, R.fft2(out) - R.fft2(x), 0)).max() <= 1e-12
        # an all-zero mask changes nothing, an all-one clean mask returns k
        assert np.array_equal(R.constrain(x, y, np.zeros_like(m), None, None, 0, None, None, True), x)
        ones = np.ones_like(m)
        assert np.abs(R.constrain(x, R.measure(k, ones), ones, None, None, 0, None, None, True) - k).max() <= 1e-12
