"""CPU: the host side of --bias_correct (mudiff_hip.volume_bias) and its fp64 restatement
(tests/volume_bias_ref.py): N3's histogram sharpening, the B-spline weights and lattices, the fixed-point scale of the fit's integer
sums, the flags, the [done] suffix, and the recovery of a known bias field by the restatement alone."""
import numpy as np
import pytest

import volume_bias_ref as B
from volume_support import cli_argv


def _two_classes(n=60000, seed=3):
    """Log intensities of two tissue classes (centres 6.0 and 6.5, own spread 0.02) blurred by a Gaussian of FWHM 0.15."""
    rng = np.random.default_rng(seed)
    centre = np.where(rng.random(n) < 0.45, 6.0, 6.5)
    sigma = np.hypot(0.02, 0.15 / (2.0 * np.sqrt(2.0 * np.log(2.0))))
    return centre, (centre + rng.standard_normal(n) * sigma).astype(np.float32)


def test_sharpen_moves_each_class_towards_its_centre_and_is_monotone():
    from mudiff_hip import volume_bias as VB
    centre, c = _two_classes()
    lo, hi, bins = float(c.min()), float(c.max()), 200
    scale = bins / (hi - lo)
    h = B.hist(c, lo, scale, bins)
    table = VB.sharpen(h, lo, hi, 0.15, 0.01)
    assert table.shape == (bins,) and table.dtype == np.float64 and np.isfinite(table).all()
    e = B.table_at(c, table, lo, scale)
    for v in (6.0, 6.5):
        sel = centre == v
        before, after = np.abs(c[sel].astype(np.float64) - v).mean(), np.abs(e[sel] - v).mean()
        print('class', v, 'mean |c - centre|', before, '-> mean |E(c) - centre|', after)
        assert after < 0.6 * before
    populated = np.nonzero(h)[0]
    assert populated.size > 100 and (np.diff(table[populated]) >= 0).all()
    # the bound choose_k relies on
    assert np.abs(c.astype(np.float64) - e).max() <= 3.0 * (hi - lo)


def test_sharpen_of_an_empty_and_of_a_single_bin_histogram_returns_the_bin_centres():
    """A single-bin histogram is what a flat image gives: lo and hi are the extremes of the very samples that are counted, so with hi > lo
    the first and the last bin are both populated, and one bin holds everything only when hi == lo (scale 0)."""
    from mudiff_hip import volume_bias as VB
    centres = VB.bin_centres(2.0, 5.0, 200)
    assert centres[0] == 2.0 + 0.5 * 3.0 / 200 and np.allclose(np.diff(centres), 3.0 / 200, rtol=1e-12, atol=0)
    assert np.array_equal(VB.sharpen(np.zeros(200, np.int64), 2.0, 5.0), centres)
    one = np.zeros(200, np.int64)
    one[0] = 12345
    assert np.array_equal(VB.sharpen(one, 4.25, 4.25), np.full(200, 4.25))
    assert np.array_equal(B.table_at(np.float32([4.25]), VB.sharpen(one, 4.25, 4.25), 4.25, 0.0), [4.25])      # residual 0: nothing to fit


def test_weights_sum_to_one():
    t = np.random.default_rng(0).random(1000)
    b = B.bspline(np.concatenate([t, [0.0, 0.5, 1.0 - 2.0 ** -53]]))
    assert b.shape == (4, 1003) and (b >= 0).all()
    assert np.abs(b.sum(0) - 1.0).max() <= 4 * np.finfo(np.float64).eps
    assert np.array_equal(B.bspline(0.0), [1 / 6, 4 / 6, 1 / 6, 0.0])


@pytest.mark.parametrize('levels', [1, 2, 3])
def test_lattices_of_a_constant_and_of_a_linear_ramp(levels):
    from mudiff_hip import volume_bias as VB
    shape = (37, 29, 23)
    lat = VB.new_lattices(levels)
    assert [L.shape[0] for L in lat] == [(1 << l) + 3 for l in range(levels)]
    lat[-1][...] = 2.5
    for stride in (1, 3):
        assert np.abs(B.field(lat, shape, stride) - 2.5).max() <= 1e-14
    # control point j of an axis sits at span coordinate j - 1; cubic B-splines reproduce what is linear in it
    n = 1 << (levels - 1)
    cz, cy, cx = np.meshgrid(*[np.arange(n + 3) - 1.0] * 3, indexing='ij')
    lat[-1] = 0.3 * cx - 0.2 * cy + 0.7 * cz + 1.0
    x, y, z = np.meshgrid(*[(np.arange(S) + 0.5) * n / S for S in shape], indexing='ij')
    assert np.abs(B.field(lat, shape, 1) - (0.3 * x - 0.2 * y + 0.7 * z + 1.0)).max() <= 1e-13
    # levels add up
    if levels > 1:
        lat[0][...] = -1.25
        assert np.abs(B.field(lat, shape, 1) - (0.3 * x - 0.2 * y + 0.7 * z - 0.25)).max() <= 1e-13


def test_choose_k_leaves_no_room_for_an_overflow():
    from mudiff_hip import volume_bias as VB
    for n, lo, hi in ((1, 0.0, 0.1), (7920, 5.0, 7.5), (60 * 60 * 39, -3.0, 9.0), (240 * 240 * 155, 0.0, 88.0), (2 ** 31 - 1, -100.0, 100.0)):
        k = VB.choose_k(n, lo, hi)
        assert 0 <= k <= VB.MAX_K
        assert n * (max(hi - lo, 1.0) * 2.0 ** k + 0.5) < 2.0 ** 63
    assert VB.choose_k(7920, 5.0, 7.5) == VB.MAX_K and VB.choose_k(2 ** 31 - 1, -100.0, 100.0) == 23
    assert VB.choose_k(100, None, None) == VB.MAX_K


def test_integer_fit_is_the_floating_point_fit():
    """delta / omega of the integer sums against the same multilevel-B-spline quotient summed in fp64.  Each of the n terms of either sum
    is rounded by at most 2^-(k+1), so |delta / omega - num / den| den <= n 2^-(k+1) (1 + |num / den|) to first order (doubled here
    for the second order and the fp64 sums' own rounding)."""
    from mudiff_hip import volume_bias as VB
    vol, _, _ = B.shaded_head()
    shape, shrink = vol.shape, 2
    c = B.log_image(vol, shrink)
    fin = c[np.isfinite(c)]
    lo, hi = float(fin.min()), float(fin.max())
    scale = 200 / (hi - lo)
    table = VB.sharpen(B.hist(c, lo, scale, 200), lo, hi)
    k = VB.choose_k(c.size, lo, hi)
    delta, omega = B.fit(c, table, lo, scale, 1, shape, shrink, k)
    assert delta.dtype == np.int64 and omega.dtype == np.int64 and delta.shape == (5, 5, 5) and (omega >= 0).all() and omega.any()
    (sx, bx), (sy, by), (sz, bz) = B._axes(shape, shrink, 2)
    ix, iy, iz = np.nonzero(np.isfinite(c))
    r = c[ix, iy, iz].astype(np.float64) - B.table_at(c[ix, iy, iz], table, lo, scale)
    S2 = (bx ** 2).sum(0)[ix] * (by ** 2).sum(0)[iy] * (bz ** 2).sum(0)[iz]
    num, den = np.zeros(125), np.zeros(125)
    for dz in range(4):
        for dy in range(4):
            for dx in range(4):
                w = bx[dx][ix] * by[dy][iy] * bz[dz][iz]
                cp = ((sz[iz] + dz) * 5 + sy[iy] + dy) * 5 + sx[ix] + dx
                np.add.at(num, cp, w ** 3 * r / S2)
                np.add.at(den, cp, w ** 2)
    some = den > 1e-6
    got = (delta.reshape(-1) / np.maximum(omega.reshape(-1), 1))[some]
    want = (num / np.where(den > 0, den, 1.0))[some]
    assert some.sum() > 60 and (np.abs(got - want) * den[some] <= 2.0 * ix.size * 2.0 ** -(k + 1) * (1.0 + np.abs(want))).all()
    assert np.abs(got - want).max() <= 1e-6 and np.abs(want).max() > 1e-3


def test_flags_defaults_and_refusals(capsys):
    from mudiff_hip import volume as V
    from mudiff_hip.volume_prepare import IntakeOptions
    options = lambda args: IntakeOptions.from_args(args).bias      # noqa: E731
    args = V.build_argparser(cli_argv())
    assert args.bias_correct is False and args.bias_field_out is False and options(args) is None
    args = V.build_argparser(cli_argv('--bias_correct'))
    assert options(args) == dict(shrink=4, levels=4, iters=50, tol=1e-3, bins=200, fwhm=0.15, wiener=0.01, field=False)
    args = V.build_argparser(cli_argv('--bias_correct', '--bias_shrink', '2', '--bias_levels', '3', '--bias_iters', '7', '--bias_tol', '0.01',
                                   '--bias_bins', '64', '--bias_fwhm', '0.2', '--bias_wiener', '0.1', '--bias_field_out'))
    assert options(args) == dict(shrink=2, levels=3, iters=7, tol=0.01, bins=64, fwhm=0.2, wiener=0.1, field=True)
    for bad, word in ((['--bias_shrink', '0'], 'bias_shrink'), (['--bias_levels', '0'], 'bias_levels'), (['--bias_levels', '6'], 'bias_levels'),
                      (['--bias_iters', '0'], 'bias_iters'), (['--bias_tol', '-1'], 'bias_tol'), (['--bias_tol', 'nan'], 'bias_tol'),
                      (['--bias_bins', '1'], 'bias_bins'), (['--bias_bins', '1025'], 'bias_bins'), (['--bias_fwhm', '0'], 'bias_fwhm'),
                      (['--bias_fwhm', 'inf'], 'bias_fwhm'), (['--bias_wiener', '0'], 'bias_wiener'), (['--bias_wiener', '-0.01'], 'bias_wiener'),
                      (['--bias_field_out'], 'bias_correct')):
        with pytest.raises(SystemExit):
            V.build_argparser(cli_argv('--bias_correct', *bad) if bad != ['--bias_field_out'] else cli_argv(*bad))
        assert word in capsys.readouterr().err
    from mudiff_hip import cohort
    assert cohort.build_argparser(cli_argv('--manifest', 'm.tsv', '--bias_correct', '--bias_shrink', '3')).bias_shrink == 3


def test_bias_suffix_and_reports(tmp_path):
    import json
    import os
    from mudiff_hip import volume as V
    from mudiff_hip import volume_bias as VB
    assert VB.bias_suffix([]) == '' and VB.bias_suffix(None) == ''
    field = np.asfortranarray(np.full((4, 3, 2), 1.5, np.float32))
    reports = [('FLAIR', dict(iterations=[3, 2], dmax=0.5), None), ('T2', dict(iterations=[1, 1], dmax=0.25), field)]
    assert VB.bias_suffix(reports) == ' | bias=FLAIR,T2'
    path = VB.write_reports(reports, str(tmp_path / 'o'), 'T1CE', np.eye(4), None)
    assert os.path.basename(path) == 'bias_t1ce.json'
    assert json.load(open(path)) == {'FLAIR': dict(iterations=[3, 2], dmax=0.5), 'T2': dict(iterations=[1, 1], dmax=0.25)}
    assert sorted(os.listdir(tmp_path / 'o')) == ['bias_field_t2_t1ce.nii.gz', 'bias_t1ce.json']
    assert np.array_equal(V.read_nifti(str(tmp_path / 'o' / 'bias_field_t2_t1ce.nii.gz'))[0], field)


def test_the_restatement_recovers_a_known_field():
    """the figure of merit the restatement alone reaches on the recovery volume is RECORDED_RATIO = 0.02304
    (iterations 50 / 46 / 11 / 7); it must stay below 0.5 and within 1.5 x the recorded value."""
    from mudiff_hip import volume_bias as VB
    vol, true_field, mask = B.shaded_head()
    opts = dict(B.RECOVERY)
    shrink = opts.pop('shrink')
    assert opts == {k: v for k, v in VB.DEFAULTS.items() if k != 'shrink'}
    engine = B.Engine(B.log_image(vol, shrink), vol.shape, shrink)
    lattices, iterations, dmax = VB.loop(engine, **opts)
    ratio = B.recovery_ratio(lattices, true_field, mask)
    print('iterations', iterations, 'dmax', dmax, 'ratio', ratio, 'bar', B.BAR)
    assert ratio < 0.5 and ratio <= B.BAR
    assert len(iterations) == 4 and all(1 <= i <= 50 for i in iterations)
    # and the corrected volume is flatter than the shaded one within each tissue class
    out = B.apply(vol, lattices)
    assert np.array_equal(out == 0, vol == 0)
    spread = lambda v: float(np.std(np.log(v[mask & (vol > 0)])))      # noqa: E731
    assert spread(out) < spread(vol)
