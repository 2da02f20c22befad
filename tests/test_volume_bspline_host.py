"""CPU: the numpy restatement of --regrid_interp cubic (tests/volume_bspline_ref.py) against scipy, the
properties the resampler is built for - it interpolates, it leaves zero background exactly zero, it stays inside the source's value
range, it is sharper than trilinear resampling - and the flag's way through the parsers, IntakeOptions and the [done] line."""
import numpy as np
import pytest

import volume_bspline_ref as S
import volume_regrid_ref as G
from volume_support import cli_argv

SCIPY_BOUND = 1e-12                                      # of max |v|: about 100 x what the recursion differs from scipy's by (8e-15, 9 x 7 x 5)


def _rotation(deg, shape, out_shape, shift=(0.0, 0.0, 0.0), scale=(1.0, 1.0, 1.0)):
    """Reference index -> source coordinate: a rotation about z by `deg` (and a third of it about x) around the grids' centres, scaled
    per axis and shifted."""
    a, b = np.deg2rad(deg), np.deg2rad(deg / 3.0)
    rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1.0]])
    rx = np.array([[1.0, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
    lin = rz @ rx @ np.diag(scale)
    M = np.eye(4)
    M[:3, :3] = lin
    M[:3, 3] = (np.array(shape) - 1) / 2.0 - lin @ ((np.array(out_shape) - 1) / 2.0) + np.array(shift)
    return M


@pytest.mark.parametrize('shape', [(9, 7, 5), (2, 3, 1), (5, 240, 3)])
def test_the_restatement_is_scipys_spline(shape):
    from scipy import ndimage
    rng = np.random.default_rng(shape[0])
    v = (rng.standard_normal(shape) * 100).astype(np.float32)
    c, bad = S.coefficients(v)
    want = ndimage.spline_filter(v.astype(np.float64), order=3, output=np.float64, mode='mirror')
    top = float(np.abs(v).max())
    print('coefficients', np.abs(c - want).max() / top)
    assert bad == 0 and c.dtype == np.float64 and np.abs(c - want).max() <= SCIPY_BOUND * top
    out_shape = tuple(max(n, 2) + 1 for n in shape)
    M = np.eye(4)                                         # a shear between the axes that have an extent; an axis of one voxel stays at 0
    for a in range(3):
        for b in range(3):
            M[a, b] = 0.0 if shape[a] == 1 else 0.8 * (shape[a] - 1) / (out_shape[a] - 1) if a == b else 0.03 * (a - b)
        M[a, 3] = (shape[a] - 1) / 2.0 - M[a, :3] @ ((np.array(out_shape) - 1) / 2.0)
    inside, _ = S.in_range(M, shape, out_shape)
    got = S.interpolate(c, v, M, out_shape, 0.0, 0.0, guard=False, clamp=False, rounded=False)
    want = ndimage.affine_transform(v.astype(np.float64), M[:3, :3], M[:3, 3], out_shape, order=3, mode='mirror', output=np.float64)
    print('interpolation', int(inside.sum()), 'points', np.abs(got - want)[inside].max() / top)
    assert inside.sum() >= 0.2 * inside.size and np.abs(got - want)[inside].max() <= SCIPY_BOUND * top


def test_it_interpolates():
    v = (np.random.default_rng(3).standard_normal((11, 6, 7)) * 300).astype(np.float32)
    v[v < -100] = 0
    got = S.regrid(v, np.eye(4), v.shape)
    assert got.dtype == np.float32 and np.array_equal(got, v) and not np.signbit(got[v == 0]).any()
    line = S.filter_axis(np.array([1.0, 4.0, 2.0]), 0)
    assert line.shape == (3,) and np.array_equal(S.filter_axis(np.array([[5.0]]), 1), [[5.0]])      # a line of one voxel is its coefficient
    assert S.coefficients(np.array([[[np.nan, 1.0, np.inf]]], np.float32).reshape(3, 1, 1))[1] == 2


@pytest.fixture(scope='module')
def ball():
    shape = (24, 22, 18)
    g = np.meshgrid(*[np.arange(n) - (n - 1) / 2.0 for n in shape], indexing='ij')
    inside = g[0] ** 2 + g[1] ** 2 + (1.2 * g[2]) ** 2 <= 7.5 ** 2
    v = np.where(inside, 400 + 100 * np.random.default_rng(5).random(shape), 0).astype(np.float32)
    return v


def test_background_stays_zero_and_values_in_range(ball):
    out_shape = (26, 20, 21)
    M = _rotation(11.0, ball.shape, out_shape, shift=(0.3, -0.4, 0.2), scale=(0.9, 1.1, 0.8))
    lo, hi = S.value_range(ball)
    assert (lo, hi) == (0.0, float(ball.max()))
    c, _ = S.coefficients(ball)
    got = S.interpolate(c, ball, M, out_shape, lo, hi)
    linear = G.trilinear(ball, M, out_shape)
    air = linear == 0
    assert air.sum() >= 0.3 * air.size and (~air).sum() >= 0.1 * air.size
    assert (got[air] == 0).all() and not np.signbit(got[air]).any()                  # exact +0 wherever trilinear gives exact 0
    assert got.min() >= lo and got.max() <= hi
    free = S.interpolate(c, ball, M, out_shape, lo, hi, guard=False, clamp=False)    # (both are needed: the spline rings and overshoots)
    print('ringing voxels', int((free[air] != 0).sum()), 'overshoot', float(free.max()) - hi, 'undershoot', float(free.min()))
    assert (free[air] != 0).any() and (free.max() > hi or free.min() < lo)


def test_it_is_sharper_than_trilinear():
    shape, out_shape = (30, 28, 26), (30, 28, 26)
    x, y, z = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing='ij')

    def f(x, y, z):
        return 500.0 + 300.0 * np.sin(2 * np.pi * x / 6.0 + 0.3) * np.sin(2 * np.pi * y / 7.5 + 1.1) * np.sin(2 * np.pi * z / 9.0 + 0.7)

    v = f(x, y, z).astype(np.float32)
    M = _rotation(7.0, shape, out_shape, shift=(0.37, 0.37, 0.37))
    inside, p = S.in_range(M, shape, out_shape)
    truth = f(*p)
    rms = lambda a: float(np.sqrt(np.mean((a.astype(np.float64) - truth)[inside] ** 2)))      # noqa: E731
    cubic, linear = rms(S.regrid(v, M, out_shape)), rms(G.trilinear(v, M, out_shape))
    print(f'RMS error over {int(inside.sum())} in-range points: cubic {cubic:.4f}, trilinear {linear:.4f}, ratio {cubic / linear:.4f}')
    assert inside.sum() >= 0.5 * inside.size and cubic < linear


def test_the_flag_the_options_and_the_done_line(capsys):
    from mudiff_hip import cohort
    from mudiff_hip import volume as V
    from mudiff_hip import volume_metrics as VM
    from mudiff_hip import volume_regrid as VR
    from mudiff_hip.volume_prepare import IntakeOptions, IntakeReport
    assert VR.MODES == {'linear': 0, 'nearest': 1} and VR.MODES_HIGH == ('cubic',) and VR.INTERPS == ('linear', 'cubic')
    args = V.build_argparser(cli_argv())
    assert args.regrid_interp == 'linear'
    assert IntakeOptions.from_args(args).interp == 'linear' and IntakeOptions.from_args(args) == IntakeOptions('percentile', False, None, None, 80)
    assert IntakeOptions._fields[-1] == 'denoise' and IntakeOptions._fields.index('half_range') == 4 and IntakeOptions().interp == 'linear'
    options = IntakeOptions.from_args(V.build_argparser(cli_argv('--regrid', '--regrid_interp', 'cubic')))
    assert options.interp == 'cubic' and options.regrid is True and options.coreg is None
    assert cohort.build_argparser(cli_argv('--manifest', 'm.tsv', '--coregister', '--regrid_interp', 'cubic')).regrid_interp == 'cubic'
    assert cohort.build_argparser(cli_argv('--manifest', 'm.tsv')).regrid_interp == 'linear'
    metrics = VM.build_parser()
    assert metrics.parse_args(['--pred', 'p', '--gt', 'g']).regrid_interp == 'linear'
    assert metrics.parse_args(['--pred', 'p', '--gt', 'g', '--regrid', '--regrid_interp', 'cubic']).regrid_interp == 'cubic'
    for build in (lambda: V.build_argparser(cli_argv('--regrid_interp', 'sinc')), lambda: metrics.parse_args(['--pred', 'p', '--gt', 'g', '--regrid_interp', 'nearest'])):
        with pytest.raises(SystemExit):
            build()
        assert 'regrid_interp' in capsys.readouterr().err
    # the [done] line: nothing by default, ` | interp=cubic` after the regrid part, the non-finite count only when there is one
    assert IntakeReport().suffix() == '' and IntakeReport(['T2']).suffix() == ' | regrid=T2'
    assert IntakeReport(['T2', 'T1'], interp='cubic').suffix() == ' | regrid=T2,T1 | interp=cubic'
    assert IntakeReport(interp='cubic', nonfinite=3).suffix() == ' | interp=cubic nonfinite=3'
    assert VR.interp_suffix('linear', 5) == ''
    with pytest.raises(ValueError, match='mode must be one of'):
        VR.regrid(_FakeGpuTensor(), 16, (1, 1, 1), 1.0, 0.0, np.eye(4), (1, 1, 1), mode='sinc')


class _FakeGpuTensor:
    is_cuda, device = True, 'cuda:0'
