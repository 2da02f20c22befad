"""Host: slice-coupled sampling noise (mudiff_hip.slice_coupling, the volume pipeline's --slice_coupling / --through_plane): the taps and
their correlation, the flags and their refusals, the statistics of the numpy restatement of the coupled draw (tests/slice_coupling_ref.py),
the through-plane restatement on a volume with closed-form values, and the two new symbols of the C ABI.  DESIGN.md section 5.23."""
import argparse
import math
import os
import re

import numpy as np
import pytest

from conftest import REPO
import slice_coupling_ref as R

MINIMAL = ['--target_modality', 'T1CE', '--output_dir', 'o', '--exp', 'e']


# ---------------------------------------------------------------------------------------------------
# taps
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('sigma', [0.25, 0.5, 1.0, 1.5, 2.0, 4.0, 7.3, 10.0])
def test_taps_have_unit_square_sum_and_the_stated_radius(sigma):
    from mudiff_hip import slice_coupling as SC
    w, radius = SC.coupling_taps(sigma)
    assert radius == math.ceil(3 * sigma) and w.shape == (radius + 1,) and w.dtype == np.float64
    assert abs(float(w[0] ** 2 + 2 * np.sum(w[1:] ** 2)) - 1.0) <= 1e-15
    assert np.all(np.diff(w) < 0) and w[-1] > 0
    want, r2 = R.taps(sigma)
    assert r2 == radius and np.allclose(w, want, rtol=0, atol=1e-15)
    assert radius <= SC.MAX_RADIUS
    # lag 0 is the variance of a draw, lags beyond 2R share no white-noise slice
    assert abs(SC.coupling_correlation(sigma, 0) - 1.0) <= 1e-15
    assert SC.coupling_correlation(sigma, 2 * radius + 1) == 0.0 and SC.coupling_correlation(sigma, 1000) == 0.0
    assert SC.coupling_correlation(sigma, 2 * radius) > 0.0
    for lag in (1, 2, radius):
        assert abs(SC.coupling_correlation(sigma, lag) - R.correlation(want, lag)) <= 1e-14
        assert SC.coupling_correlation(sigma, -lag) == SC.coupling_correlation(sigma, lag)


def test_lag_one_correlation_is_close_to_the_continuous_gaussian():
    from mudiff_hip import slice_coupling as SC
    for sigma in (1.0, 1.5, 2.0, 4.0, 10.0):
        assert abs(SC.coupling_correlation(sigma, 1) - math.exp(-1.0 / (4 * sigma * sigma))) <= 1e-3, sigma
    assert round(SC.coupling_correlation(1.0, 1), 4) == 0.7786 and round(SC.coupling_correlation(4.0, 1), 4) == 0.9845


@pytest.mark.parametrize('bad', [0, -1.0, 10.5, float('nan'), float('inf'), 'wide'])
def test_taps_refuse_a_sigma_outside_the_range(bad):
    from mudiff_hip import slice_coupling as SC
    with pytest.raises(ValueError):
        SC.coupling_taps(bad)


def test_check_coupling():
    from mudiff_hip import slice_coupling as SC
    assert SC.check_coupling(None) is None and SC.check_coupling('shared') == 'shared'
    half, radius = SC.check_coupling(([1.0], 0))
    assert radius == 0 and half.tolist() == [1.0]
    for bad in ('Shared', ([1.0, 0.5], 0), ([1.0], 33), ([float('nan')], 0), 4.0, ([1.0] * 34, 33)):
        with pytest.raises(ValueError):
            SC.check_coupling(bad)


# ---------------------------------------------------------------------------------------------------
# flags
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('bad', ['0', '-2', '10.01', 'nan', 'both', ''])
def test_flag_refusals_leave_through_the_parser(bad, capsys):
    from mudiff_hip import cohort, volume as V
    for build in (lambda: V.build_argparser(MINIMAL + ['--slice_coupling', bad]),
                  lambda: cohort.build_argparser(MINIMAL + ['--manifest', 'm.tsv', '--slice_coupling', bad])):
        with pytest.raises(SystemExit) as e:
            build()
        assert e.value.code == 2 and '--slice_coupling' in capsys.readouterr().err


def test_flag_values_and_the_done_tail():
    from mudiff_hip import cohort, volume as V, slice_coupling as SC
    plain = V.build_argparser(MINIMAL)
    assert plain.slice_coupling is None and plain.through_plane is False
    assert V._done_tail(plain, 'auto') == '' and V._coupling(plain) is None
    bare = argparse.Namespace(norm='percentile')                              # a namespace from before the flag
    assert V._done_tail(bare, 'auto') == '' and V._coupling(bare) is None
    a = V.build_argparser(MINIMAL + ['--slice_coupling', '4', '--through_plane'])
    assert a.through_plane is True and V._done_tail(a, 'auto') == ' | slice_coupling=4'
    half, radius = V._coupling(a)
    assert radius == 12 and np.array_equal(half, SC.coupling_taps(4.0)[0])
    b = V.build_argparser(MINIMAL + ['--slice_coupling', 'shared', '--norm', 'zscore'])
    assert V._coupling(b) == 'shared' and V._done_tail(b, '16x1') == ' | prec_plan=16x1 | norm=zscore | slice_coupling=shared'
    c = cohort.build_argparser(MINIMAL + ['--manifest', 'm.tsv', '--slice_coupling', '0.5'])
    assert V._done_tail(c, 'auto') == ' | slice_coupling=0.5' and V._coupling(c)[1] == 2
    assert '--slice_coupling' in V.make_parser().format_help() and '--through_plane' in V.make_parser().format_help()


def test_a_negative_seed_is_refused_with_the_flag(capsys):
    from mudiff_hip import volume as V
    with pytest.raises(SystemExit):
        V.build_argparser(MINIMAL + ['--slice_coupling', '2', '--seed', '-1'])
    assert '--slice_coupling needs a --seed' in capsys.readouterr().err
    assert V.build_argparser(MINIMAL + ['--seed', '-1']).seed == -1              # without the flag: as before


def test_injected_draws_and_a_coupling_are_refused():
    from mudiff_hip import volume as V
    args = V.build_argparser(MINIMAL)
    stacks = [np.zeros((2, 16, 16), np.float32)] * 3
    with pytest.raises(ValueError, match='coupling'):
        V.predict_slices(args, None, None, stacks, 'cpu', x_inits=np.zeros((2, 1, 16, 16), np.float32), seed=1, coupling='shared')
    with pytest.raises(ValueError, match='coupling'):
        V.predict_slices(args, None, None, stacks, 'cpu', zs=[], noises=[], seed=1, coupling=([1.0], 0))
    with pytest.raises(ValueError, match='seed'):
        V.predict_slices(args, None, None, stacks, 'cpu', coupling='shared')


# ---------------------------------------------------------------------------------------------------
# the restatement's own statistics
# ---------------------------------------------------------------------------------------------------
def test_restated_draws_are_standard_normal_and_correlate_as_stated():
    """24 consecutive slices x 16384 elements at sigma = 1 (R = 3), seed 1024: per row the mean within 5 / sqrt(L); the variance within
    6 sqrt(2 / L) and every pair's lag-d correlation within 6 / sqrt(L) of coupling_correlation (the product estimators' own deviation
    is up to sqrt(1 + rho^2) above that of a mean, hence 6 and not 5), for d = 1..2R + 2."""
    n, L, sigma = 24, 16384, 1.0
    half, radius = R.taps(sigma)
    x = R.randn_keyed_coupled([[s, 0] for s in range(n)], L, 1024, 0, R.E.KIND_X, half, radius).astype(np.float64)
    mean, var = x.mean(1), x.var(1)
    print('max |mean|', np.abs(mean).max(), 'max |var - 1|', np.abs(var - 1).max())
    assert np.abs(mean).max() <= 5 / math.sqrt(L)
    assert np.abs(var - 1).max() <= 6 * math.sqrt(2 / L)
    worst = 0.0
    for d in range(1, 2 * radius + 3):
        rho = R.correlation(half, d)
        assert (rho == 0.0) == (d > 2 * radius)
        got = (x[:-d] * x[d:]).mean(1)
        worst = max(worst, float(np.abs(got - rho).max()))
    print('max |corr - rho|', worst)
    assert worst <= 6 / math.sqrt(L)
    # radius 0 with w_0 = 1 is the uncoupled draw
    assert np.array_equal(R.randn_keyed_coupled([[5, 1]], 10, 3, 1, 2, np.array([1.0]), 0), R.E.randn_keyed([[5, 1]], 10, 3, 1, 2))


def test_restated_taps_below_slice_zero_wrap():
    """Slice 0 at R = 1 reads the white noise of slice 2^64 - 1: the Philox counter word wraps."""
    half = np.array([0.5, 0.25])
    got = R.randn_keyed_coupled([[0, 2]], 8, 9, 1, 1, half, 1)
    eta = lambda s: R.E.randn_keyed(np.array([[s, 2]], np.int64), 8, 9, 1, 1).astype(np.float64)      # noqa: E731
    below = np.array([R.E.block_normals(R.E.philox4x64(R.E.counter(b, R.E.M64, 2, 1, 1), R.E.key(9))) for b in range(2)]).reshape(1, 8)
    want = (0.25 * below.astype(np.float32).astype(np.float64) + 0.5 * eta(0)) + 0.25 * eta(1)
    assert np.array_equal(got, want.astype(np.float32))


# ---------------------------------------------------------------------------------------------------
# through-plane restatement
# ---------------------------------------------------------------------------------------------------
def test_through_plane_restatement_on_a_ramp():
    z, x, y = np.meshgrid(np.arange(6), np.arange(5), np.arange(7), indexing='ij')
    vol = (0.5 * z + 0.125 * x + 0.25 * y).astype(np.float32)
    r = R.through_plane(vol)
    assert r['mean_dz'] == 0.5 and r['mean_dx'] == 0.125 and r['mean_dy'] == 0.25 and r['mean_dzz'] == 0.0
    assert r['anisotropy'] == 0.5 / 0.1875 and r['dz'] == [0.5] * 5
    s = R.through_plane_sums(vol)
    assert s[:, 0].tolist() == [35] * 5 + [0] and s[:, 2].tolist() == [0] + [35] * 4 + [0]
    assert s[:, 4].tolist() == [28] * 6 and s[:, 6].tolist() == [30] * 6
    # a quadratic in z: the second difference is its constant, a clipped range drops the outer planes
    quad = (0.25 * z * z).astype(np.float32)
    assert R.through_plane(quad)['mean_dzz'] == 0.5 and R.through_plane(quad, z0=-3, z1=99)['mean_dzz'] == 0.5
    assert R.through_plane(quad, z0=2, z1=3) == dict(mean_dz=1.25, mean_dzz=None, mean_dx=0.0, mean_dy=0.0, anisotropy=None, dz=[1.25])
    # a mask that empties plane 2: its pairs and the triples around it vanish
    mask = np.ones(vol.shape, np.uint8)
    mask[2] = 0
    m = R.through_plane(vol, mask)
    assert m['dz'] == [0.5, None, None, 0.5, 0.5] and m['mean_dz'] == 0.5
    assert R.through_plane_sums(vol, mask)[:, 2].tolist() == [0, 0, 0, 0, 35, 0]


def test_summarize_matches_the_restatement():
    from mudiff_hip import volume_through_plane as TP
    rng = np.random.default_rng(0)
    vol = rng.random((6, 5, 7), dtype=np.float32)
    mask = (rng.random(vol.shape) < 0.7).astype(np.uint8)
    mask[3] = 0
    rep = TP.summarize(R.through_plane_sums(vol, mask), first_plane=4)
    want = R.through_plane(vol, mask)
    assert {k: rep[k] for k in want} == want and rep['planes'] == [4, 9] and None in rep['dz']
    empty = TP.summarize(np.zeros((3, 8)))
    assert empty['mean_dz'] is None and empty['anisotropy'] is None and empty['dz'] == [None, None]


# ---------------------------------------------------------------------------------------------------
# C ABI
# ---------------------------------------------------------------------------------------------------
def test_the_new_symbols_are_declared_bound_and_exported():
    import mudiff_hip
    if not os.path.isfile(mudiff_hip.lib_path()):
        import __graft_entry__
        __graft_entry__.build()
    txt = re.sub(r'/\*.*?\*/', '', open(os.path.join(REPO, 'include', 'mudiff_hip.h')).read(), flags=re.S)
    declared = set(re.findall(r'\b(mud_[a-z0-9_]+)\s*\(', txt))
    lib = mudiff_hip.load()
    for name in ('mud_randn_keyed_coupled', 'mud_volume_through_plane'):
        assert name in declared and name in mudiff_hip.EXPORTED_SYMBOLS and hasattr(lib, name), name
    assert re.search(r'#define MUD_COUPLING_MAX_RADIUS 32\b', txt) and re.search(r'#define MUD_TP_NQ 8\b', txt)
    from mudiff_hip import ops, slice_coupling as SC
    assert SC.MAX_RADIUS == ops.COUPLING_MAX_RADIUS == 32 and (ops.TP_NQ, ops.TP_PARTS) == (8, 16)
