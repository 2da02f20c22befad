"""CPU: the host side of --known_lowres_volume (mudiff_hip.lowres_volume, ops.lowres_tables): the Kronecker
factorisation itself on the restatements of tests/lowres_ref.py alone, the geometry of each axis from the two affines in closed form, the
rows, the product-condition refusal, the measured product set, the flags' refusals on both command lines, and the symbols."""
import argparse
import os
import re

import numpy as np
import pytest

import band_ref
import lowres_ref as R
import volume_support as VS
from conftest import REPO

SYMBOLS = ('mud_lowres_constrain', 'mud_lowres_measure', 'mud_lowres_ws_floats')
SHAPES = ((7, 12, 8), (5, 10, 6))
SPECS = {'aligned2': (0.5, 2.0, 2.0, 'box'), 'ratio2.5+0.3': (1.05, 2.5, 2.5, 'box'), 'overlap1.5': (1.0, 2.0, 3.0, 'box'),
         'gauss': (1.5, 2.0, 2.0, 'gauss')}


def _matrices(shape, spec):
    return tuple(band_ref.weights(size, *spec)[0] for size in shape)


def test_symbols_are_declared_and_bound():
    import mudiff_hip
    from mudiff_hip import ops
    txt = re.sub(r'/\*.*?\*/', '', open(os.path.join(REPO, 'include', 'mudiff_hip.h')).read(), flags=re.S)
    for name in SYMBOLS:
        assert re.search(r'\b' + name + r'\s*\(', txt), name
        assert name in mudiff_hip._SIGNATURES and name in mudiff_hip.EXPORTED_SYMBOLS, name
    lib = mudiff_hip.load()
    assert lib.mud_version() >= 122
    assert lib.mud_lowres_ws_floats(2, 7, 3, 6, 4) == 2 * (7 + 3) * 6 * 4 and lib.mud_lowres_ws_floats(1, 7, 0, 6, 4) == -1
    kinds = {ops.KIND_X_INIT, ops.KIND_Z, ops.KIND_NOISE, ops.KIND_KNOWN, ops.KIND_RENOISE, ops.KIND_KSPACE, ops.KIND_THICK, ops.KIND_MULTISLICE,
             ops.KIND_BAND, ops.KIND_LOWRES}
    assert ops.KIND_LOWRES == 9 and len(kinds) == 10 and max(kinds) <= 15
    assert 'lowres_constrain' in ops.randn_keyed.__doc__
    readme = open(os.path.join(REPO, 'README.md')).read()
    assert f'C ABI ({len(mudiff_hip.EXPORTED_SYMBOLS)} entry points)' in readme and '--known_lowres_volume' in readme


@pytest.mark.parametrize('shape', SHAPES)
@pytest.mark.parametrize('name', list(SPECS))
def test_the_separable_projection_is_the_dense_one(shape, name):
    """A A^T = G_z (x) G_y (x) G_x: (a) and (b) of tests/lowres_ref.py agree to 1e-12, noisy and clean."""
    Az, Ay, Ax = _matrices(shape, SPECS[name])
    g = np.random.default_rng(len(name) + shape[0])
    x = g.standard_normal(shape).astype(np.float32)
    eta = g.standard_normal(shape).astype(np.float32)
    y = R.measure_dense(np.tanh(g.standard_normal(shape)).astype(np.float32), Az, Ay, Ax).astype(np.float32)
    A = R.kron3(Az, Ay, Ax)
    G = np.kron(np.kron(band_ref.as_kernel(Az) @ band_ref.as_kernel(Az).T, band_ref.as_kernel(Ay) @ band_ref.as_kernel(Ay).T),
                band_ref.as_kernel(Ax) @ band_ref.as_kernel(Ax).T)
    assert np.abs(A @ A.T - G).max() <= 1e-15
    for args in ((None, 1.0, 0.0, True), (eta, 0.81, 0.5864, False)):
        dense, sep = R.constrain_dense(x, y, Az, Ay, Ax, *args), R.constrain_separable(x, y, Az, Ay, Ax, *args)
        assert np.abs(dense - sep).max() <= 1e-12
        d = dense if args[3] else dense - args[2] * eta.astype(np.float64)
        assert np.abs(R.measure_dense(d, Az, Ay, Ax) - args[1] * y.astype(np.float64)).max() <= 1e-12       # A (out - s eta) = a y
        N = R.null_basis(Az, Ay, Ax)
        assert N.shape[1] == A.shape[1] - A.shape[0] and np.abs(N.T @ (dense - x).reshape(-1)).max() <= 1e-12


def test_the_fp32_emulation_follows_the_tables_and_keeps_free_pixels():
    from mudiff_hip import ops
    for shape in SHAPES:
        for name, spec in SPECS.items():
            Az, Ay, Ax = _matrices(shape, spec)
            tabs = ops.lowres_tables(Az, Ay, Ax)
            assert tabs.shape == (Az.shape[0], Ay.shape[0], Ax.shape[0]) and tabs.cond == pytest.approx(tabs.z.cond * tabs.y.cond * tabs.x.cond)
            g = np.random.default_rng(3)
            x = g.standard_normal(shape).astype(np.float32)
            y = R.measure_dense(np.tanh(g.standard_normal(shape)).astype(np.float32), Az, Ay, Ax).astype(np.float32)
            out = R.constrain_fp32(x, y, tabs)
            err = np.abs(out.astype(np.float64) - R.constrain_dense(x, y, Az, Ay, Ax)).max()
            assert err <= 64 * R.EPS32 * np.abs(x).max() * max(tabs.cond, 1.0), (shape, name, err)
            cover = [(band_ref.as_kernel(A) != 0).any(0) for A in (Az, Ay, Ax)]
            covered = cover[0][:, None, None] & cover[1][None, :, None] & cover[2][None, None, :]
            assert np.array_equal(out[~covered].view(np.int32), x[~covered].view(np.int32)) and (~covered).any()
            assert np.abs(R.measure_fp32(x, tabs).astype(np.float64) - R.measure_dense(x, Az, Ay, Ax)).max() <= 8 * R.EPS32 * np.abs(x).max()


def _affines():
    """A 1 mm 240 x 240 x 155 grid and a 2 x 2 x 5 mm Y whose first voxel starts where the grid's does."""
    grid = np.array([[1.0, 0, 0, -120.0], [0, 1.0, 0, -110.0], [0, 0, 1.0, -70.0], [0, 0, 0, 1.0]])
    y = np.diag([2.0, 2.0, 5.0, 1.0])
    y[:3, 3] = grid[:3, 3] + [0.5, 0.5, 2.0]
    return grid, y


def test_geometry_in_closed_form_and_its_refusals():
    from mudiff_hip import lowres_volume as LV
    grid, y = _affines()
    geo = LV.voxel_geometry((240, 240, 155), grid, (120, 120, 31), y)
    assert geo['c0'] == [0.5, 0.5, 2.0] and geo['step'] == [2.0, 2.0, 5.0] and geo['fine_mm'] == [1.0] * 3 and geo['coarse_mm'] == [2.0, 2.0, 5.0]
    assert geo['m'] == [120, 120, 31]
    # onto the sampler's 256 pixels: coarse voxel j of 2 fine voxels covers pixels [j, j + 1) * 2 * 256 / 240 - 1/2
    c, w, step = LV.to_sampler(geo['c0'][0] + geo['step'][0] * np.arange(120), 2.0, 2.0, 256, 240)
    k = 256 / 240
    assert w == pytest.approx(2 * k, abs=1e-15) and step == pytest.approx(2 * k, abs=1e-15)
    assert np.abs(c - ((2 * np.arange(120) + 1) * k - 0.5)).max() <= 1e-12
    assert c[0] - w / 2 == pytest.approx(-0.5, abs=1e-12) and c[-1] + w / 2 == pytest.approx(255.5, abs=1e-12)
    assert LV.kept(c, w, 'box', -0.5, 255.5).all() and LV.kept(c, w, 'gauss', -0.5, 255.5).tolist() == [False] + [True] * 118 + [False]
    A = LV.weight_rows(256, c, w, 'box')
    assert np.abs(A.sum(1) - 1).max() <= 1e-14 and int((A != 0).sum(1).max()) <= 4
    # a shifted origin, a voxel size of its own, and both grids turned the same way
    moved = y.copy()
    moved[:3, 3] += [0.3, -1.25, 2.5]
    geo = LV.voxel_geometry((240, 240, 155), grid, (100, 100, 20), moved)
    assert geo['c0'] == pytest.approx([0.8, -0.75, 4.5], abs=1e-12) and geo['step'] == [2.0, 2.0, 5.0]
    rot = np.eye(4)
    a = 0.3
    rot[:3, :3] = [[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]
    geo = LV.voxel_geometry((240, 240, 155), rot @ grid, (100, 100, 20), rot @ moved)
    assert geo['c0'] == pytest.approx([0.8, -0.75, 4.5], abs=1e-10) and geo['step'] == pytest.approx([2.0, 2.0, 5.0], abs=1e-12)
    scaled = np.diag([0.9, 0.9, 1.2, 1.0]) @ grid
    geo = LV.voxel_geometry((240, 240, 155), scaled, (100, 100, 20), np.diag([0.9, 0.9, 1.2, 1.0]) @ moved)
    assert geo['fine_mm'] == pytest.approx([0.9, 0.9, 1.2]) and geo['coarse_mm'] == pytest.approx([1.8, 1.8, 6.0])
    assert geo['c0'] == pytest.approx([0.8, -0.75, 4.5], abs=1e-12)

    def refused(b, shape=(120, 120, 31)):
        with pytest.raises(ValueError, match='--known_lowres_volume.*out of scope'):
            LV.voxel_geometry((240, 240, 155), grid, shape, b)

    turned = y.copy()
    turned[:3, :3] = rot[:3, :3] @ y[:3, :3]
    refused(turned)                                                                      # a rotated Y
    tilt = y.copy()
    tilt[:3, 0] = [2 * np.cos(2e-3), 2 * np.sin(2e-3), 0]
    refused(tilt)                                                                        # one axis tilted by 2e-3 rad
    for k in range(3):
        flipped = y.copy()
        flipped[:3, k] = -flipped[:3, k]
        refused(flipped)                                                                 # a flipped axis
    swapped = y.copy()
    swapped[:3, [0, 1]] = swapped[:3, [1, 0]]
    refused(swapped)
    LV.voxel_geometry((240, 240, 155), grid, (120, 120, 31), y + 1e-4 * np.eye(4))        # inside the tolerance
    with pytest.raises(ValueError, match='3D'):
        LV.voxel_geometry((240, 240, 155), grid, (120, 120), y)


def test_rows_sum_to_one_on_every_axis_and_the_product_condition_cap():
    from mudiff_hip import lowres_volume as LV, ops
    for profile in ('box', 'gauss'):
        for size, c0, step, width in ((155, 2.0, 5.0, 5.0), (256, 0.5667, 2.1333, 2.1333), (256, 1.0, 2.1333, 3.2)):
            c = c0 + step * np.arange(int(size / step) - 2) + (step if profile == 'gauss' else 0.0)
            A = LV.weight_rows(size, c, width, profile)
            assert np.abs(A.sum(1) - 1).max() <= 1e-14 and (A >= 0).all()
    # coarse voxels 0.99 of their extent apart overlap by 1 %: every axis is well conditioned, and so is the product
    near = [band_ref.weights(size, 1.0, 1.98, 2.0, 'box')[0] for size in (24, 24, 24)]
    tabs = ops.lowres_tables(*near)
    print(f'overlap at 0.99 of the extent: cond {tabs.z.cond:.4g} per axis, {tabs.cond:.4g} as a product')
    assert tabs.cond <= ops.BAND_MAX_COND and tabs.cond == pytest.approx(tabs.z.cond ** 3)
    # coincident voxels on one axis: that axis's own refusal
    twice = np.stack([near[0][0], near[0][0]])
    with pytest.raises(ValueError, match='cond'):
        ops.lowres_tables(twice, near[1], near[2])
    # every axis passes on its own, the product does not
    axis = band_ref.weights(24, 1.0, 1.5, 3.0, 'box')[0]
    one = ops.band_tables(axis)
    assert one.cond <= ops.BAND_MAX_COND < one.cond ** 3
    with pytest.raises(ValueError, match='lowres_tables: cond'):
        ops.lowres_tables(axis, axis, axis)
    with pytest.raises(ValueError, match='256'):
        ops.lowres_tables(np.eye(257), near[1], near[2])


def _inputs(values, y_affine, grid_shape=(16, 16, 9), **options):
    from mudiff_hip import lowres_volume as LV
    opt = dict(dict(volume='y', extent=None, profile='box', drop=[], baseline=False, resample=1), **options)
    geo = LV.voxel_geometry(grid_shape, np.eye(4), values.shape, y_affine)
    return LV.LowresInputs(values, geo, grid_shape, opt, y_affine, np.eye(4), 'linear')


def test_the_measured_product_set_with_a_dropped_slice_and_a_nan_voxel():
    """16 x 16 x 9 at 1 mm, S = 16, slab 1..7; Y of 2 x 2 x 3 mm voxels that start one fine voxel before the grid's corner: 9 x 9 x 4 coarse
    voxels, of which the first in-plane and the last reach outside, and along z those that leave the slab."""
    import torch
    from mudiff_hip import lowres_volume as LV
    aff = np.diag([2.0, 2.0, 3.0, 1.0])
    aff[:3, 3] = [-0.5, -0.5, 0.0]                        # coarse voxel 0 covers fine voxels -1, 0 in-plane and slices -1, 0, 1 along z: outside
    g = np.random.default_rng(0)
    vals = 100 + 50 * g.random((9, 9, 4))
    ref = ((16, 16, 9), np.eye(4), None, 1, 7)

    def run(values, **options):
        m = LV.measure(_inputs(values, aff, **options), ref, 16, 'percentile', torch.device('cpu'))
        return m, m.report

    m, rep = run(vals)
    assert [rep['axes'][k]['measured'] for k in 'zyx'] == [2, 7, 7] and [rep['axes'][k]['first'] for k in 'zyx'] == [1, 1, 1]
    assert [s['measured'] for s in rep['slices']] == [False, True, True, False] and rep['measured_slices'] == 2
    assert m.shape == (2, 7, 7) and tuple(m.y.shape) == (2, 7, 7) and (m.n, m.H, m.W) == (7, 16, 16)
    assert rep['axes']['z']['c0'] == -1.0 and rep['axes']['z']['step'] == 3.0 and rep['axes']['z']['width'] == 3.0
    assert rep['axes']['y']['c0'] == -0.5 and rep['axes']['y']['width'] == 2.0 and rep['extent_mm'] == [2.0, 2.0, 3.0]
    for A in m.A:
        assert np.abs(A.sum(1) - 1).max() <= 1e-14
    # coarse slice 1 covers fine slices 2..4 = local 1..3, whole thin slices; in-plane coarse j covers pixels 2 j - 1, 2 j
    assert np.array_equal(m.A[0], np.array([[0, 1, 1, 1, 0, 0, 0], [0, 0, 0, 0, 1, 1, 1]]) / 3.0)
    assert np.array_equal(np.flatnonzero(m.A[1][0]), [1, 2]) and np.array_equal(np.flatnonzero(m.A[2][6]), [13, 14])
    assert rep['cond'] == pytest.approx(1.0) and [rep['axes'][k]['bandwidth'] for k in 'zyx'] == [0, 0, 0]
    assert m.done_suffix() == ' | lowres_volume=2x2x3mm on 1x1x1mm box (2/4 slices, bw 0/0/0)'
    # y holds Y's own values, normalised, rows = volume axis 0: nothing is resampled
    from mudiff_hip.volume import normalise_volume
    want = np.moveaxis(np.asarray(normalise_volume(vals, 'percentile'), np.float32)[1:8, 1:8, 1:3], 2, 0)
    assert np.array_equal(m.y.numpy(), want)
    # a dropped slice and a non-finite voxel: inside J_y x J_x it takes its slice out, outside it does not
    _, rep = run(vals, drop=[(2, 3)])
    assert [s['measured'] for s in rep['slices']] == [False, True, False, False] and rep['drop'] == [[2, 3]]
    bad = vals.copy()
    bad[3, 4, 1] = np.nan
    bad[0, 0, 2] = np.inf                                   # outside J_y x J_x
    m2, rep = run(bad)
    assert [s['measured'] for s in rep['slices']] == [False, False, True, False] and m2.shape == (1, 7, 7) and np.isfinite(m2.y.numpy()).all()
    # overlapping extents: fewer voxels fit, the bandwidth grows
    _, rep = run(vals, extent=[3.0, 3.0, 3.0])
    assert [rep['axes'][k]['bandwidth'] for k in 'zyx'] == [0, 1, 1] and rep['cond'] > 1 and [rep['axes'][k]['measured'] for k in 'zyx'] == [2, 7, 7]
    # nothing measured: sampled freely
    m3, rep = run(vals, drop=[(0, 3)])
    assert not m3.measured and m3.tables is None and m3.m == 0 and rep['measured_slices'] == 0 and m3.finish()['max_residual'] is None


def test_the_two_in_plane_axes_keep_their_roles_on_a_grid_that_is_not_square():
    """20 x 12 x 9 at 1 mm sampled at S = 16, so the two in-plane scales differ (0.8 and 4/3) and neither is 1; Y of 4 x 2 x 3 mm voxels
    with another origin on each axis: volume x must land on the image rows (A_y, the tables' second axis), volume y on the columns."""
    import torch
    from mudiff_hip import lowres_volume as LV
    from mudiff_hip.volume import normalise_volume
    aff = np.diag([4.0, 2.0, 3.0, 1.0])
    aff[:3, 3] = [1.5, 1.0, 1.0]                          # x: voxel j covers fine [4 j - 0.5, 4 j + 3.5]; y: [2 j, 2 j + 2]; z: slices 3 j .. 3 j + 2
    vals = 100 + 50 * np.random.default_rng(1).random((5, 6, 3))
    m = LV.measure(_inputs(vals, aff, grid_shape=(20, 12, 9)), ((20, 12, 9), np.eye(4), None, 0, 8), 16, 'percentile', torch.device('cpu'))
    rep = m.report
    # rows: centres (1.5 + 4 j + 0.5) 0.8 - 0.5 = 1.1 + 3.2 j, width 3.2, all 5 inside [-0.5, 15.5]
    # columns: centres (1 + 2 j + 0.5) 4/3 - 0.5 = 1.5 + 8 j / 3, width 8/3, supports [1/6 + 8 j / 3, 17/6 + 8 j / 3]: j = 0..4 inside, j = 5 ends at 16.17
    assert (rep['axes']['y']['volume_axis'], rep['axes']['x']['volume_axis']) == ('x', 'y')
    assert (rep['axes']['y']['c0'], rep['axes']['y']['step'], rep['axes']['y']['width']) == pytest.approx((1.1, 3.2, 3.2), abs=1e-12)
    assert (rep['axes']['x']['c0'], rep['axes']['x']['step'], rep['axes']['x']['width']) == pytest.approx((1.5, 8 / 3, 8 / 3), abs=1e-12)
    assert [rep['axes'][k]['measured'] for k in 'zyx'] == [3, 5, 5] and [rep['axes'][k]['coarse'] for k in 'zyx'] == [3, 5, 6]
    assert m.shape == (3, 5, 5) and [M.shape for M in m.A] == [(3, 9), (5, 16), (5, 16)]
    assert np.abs(m.A[1] - band_ref.weights(16, 1.1, 3.2, 3.2, 'box', count=5)[0]).max() <= 1e-14
    assert np.abs(m.A[2] - band_ref.weights(16, 1.5, 8 / 3, 8 / 3, 'box', count=5)[0]).max() <= 1e-14
    want = np.moveaxis(np.asarray(normalise_volume(vals, 'percentile'), np.float32)[:, :5, :], 2, 0)      # [z, volume x, volume y]
    assert np.array_equal(m.y.numpy(), want) and not np.array_equal(m.y.numpy(), np.swapaxes(want, 1, 2))
    assert m.done_suffix().startswith(' | lowres_volume=4x2x3mm on 1x1x1mm box (3/3 slices')


def _ns(**kw):
    return argparse.Namespace(**{**dict(seed=31, known_resample=1), **kw})


def test_flags_and_their_refusals_on_both_command_lines(capsys):
    from mudiff_hip import cohort as Co, lowres_volume as LV, thick_volume as TV, volume as V
    assert LV.options_from(_ns()) is None and LV.options_from(argparse.Namespace()) is None
    assert LV.options_from(_ns(known_lowres_volume='y.nii.gz')) == dict(volume='y.nii.gz', extent=None, profile='box', drop=[], baseline=False, resample=1)
    got = LV.options_from(_ns(known_lowres_volume='y.nii.gz', lowres_volume_extent_mm=[2, 2.5, 5], lowres_volume_profile='gauss',
                              lowres_volume_drop=['1:2', '7:7'], lowres_volume_baseline=True, known_resample=3))
    assert got == dict(volume='y.nii.gz', extent=[2.0, 2.5, 5.0], profile='gauss', drop=[(1, 2), (7, 7)], baseline=True, resample=3)
    for flag, kw in (('--lowres_volume_extent_mm', dict(lowres_volume_extent_mm=[2, 2, 5])), ('--lowres_volume_profile', dict(lowres_volume_profile='box')),
                     ('--lowres_volume_drop', dict(lowres_volume_drop=['1:2'])), ('--lowres_volume_baseline', dict(lowres_volume_baseline=True))):
        with pytest.raises(ValueError, match=f'{flag} needs --known_lowres_volume'):
            LV.options_from(_ns(**kw))
    others = (('known_volume', 'k.nii.gz'), ('known_kspace', 'equispaced'), ('known_thick', 5), ('known_multislice', 'equispaced'),
              ('known_mask', 'm.nii.gz'), ('known_drop_slices', ['1:2']), ('known_thick_volume', 't.nii.gz'))
    for other, value in others:
        with pytest.raises(ValueError, match=f'--known_lowres_volume cannot be combined with --{other}'):
            LV.options_from(_ns(known_lowres_volume='y.nii.gz', **{other: value}))
    for flag, kw in (('--lowres_volume_extent_mm', dict(lowres_volume_extent_mm=[2, 0, 5])), ('--lowres_volume_extent_mm', dict(lowres_volume_extent_mm=[2, float('nan'), 5])),
                     ('--lowres_volume_profile', dict(lowres_volume_profile='sinc')), ('--lowres_volume_drop', dict(lowres_volume_drop=['3'])),
                     ('--lowres_volume_drop', dict(lowres_volume_drop=['4:2'])), ('--known_resample', dict(known_resample=0)),
                     ('--seed', dict(seed=-1)), ('manifest', dict(known_lowres_volume='manifest'))):
        with pytest.raises(ValueError, match=flag):
            LV.options_from(_ns(**{**dict(known_lowres_volume='y.nii.gz'), **kw}))
    assert LV.options_from(_ns(known_lowres_volume='manifest', manifest='cohort.tsv'))['volume'] == 'manifest'
    assert TV._OTHERS == ('known_volume', 'known_kspace', 'known_thick', 'known_multislice', 'known_mask', 'known_drop_slices')      # as they were
    # through the volume parser: a parser of its own, before the pinned ones; --known_resample goes with Y
    args = V.build_argparser(VS.cli_argv('--known_lowres_volume', 'y.nii.gz', '--known_resample', '2', '--lowres_volume_extent_mm', '2', '2', '5',
                                         '--lowres_volume_drop', '0:1', '--lowres_volume_baseline'))
    assert (args.known_lowres_volume, args.known_resample, args.lowres_volume_extent_mm, args.lowres_volume_drop, args.lowres_volume_baseline) == \
        ('y.nii.gz', 2, [2.0, 2.0, 5.0], ['0:1'], True)
    p = V.make_parser()
    new = ['--known_lowres_volume', '--lowres_volume_extent_mm', '--lowres_volume_profile', '--lowres_volume_drop', '--lowres_volume_baseline']
    mine = [late for late in p.lates if [o for a in late._actions for o in a.option_strings] == new]
    assert len(mine) == 1 and not any(o in new for late in [p] + [q for q in p.lates if q is not mine[0]] for a in late._actions for o in a.option_strings)
    assert V.sampling_modes()[:-1] == V.measurement_modes() and V.sampling_modes()[-1] is LV
    refusals = [(['--known_lowres_volume', 'y.nii.gz', '--' + other] + ([str(v) for v in value] if isinstance(value, list) else [str(value)]),
                 f'--known_lowres_volume cannot be combined with --{other}') for other, value in others]
    refusals += [(['--lowres_volume_baseline'], '--lowres_volume_baseline needs --known_lowres_volume'),
                 (['--lowres_volume_profile', 'gauss'], '--lowres_volume_profile needs --known_lowres_volume'),
                 (['--lowres_volume_drop', '1:2'], '--lowres_volume_drop needs --known_lowres_volume'),
                 (['--lowres_volume_extent_mm', '2', '2', '5'], '--lowres_volume_extent_mm needs --known_lowres_volume'),
                 (['--known_lowres_volume', 'y.nii.gz', '--lowres_volume_extent_mm', '2', '-2', '5'], '--lowres_volume_extent_mm'),
                 (['--known_lowres_volume', 'y.nii.gz', '--lowres_volume_drop', '5'], '--lowres_volume_drop'),
                 (['--known_lowres_volume', 'manifest'], 'needs a cohort'), (['--known_resample', '2'], '--known_resample needs --known_volume')]
    for argv, text in refusals:
        with pytest.raises(SystemExit):
            V.build_argparser(VS.cli_argv(*argv))
        assert text in capsys.readouterr().err, argv
    # ... and through the cohort's
    cohort = lambda *extra: Co.build_argparser(['--manifest', 'cohort.tsv'] + VS.cli_argv(*extra))      # noqa: E731
    assert cohort('--known_lowres_volume', 'manifest', '--lowres_volume_profile', 'gauss').known_lowres_volume == 'manifest'
    for argv, text in refusals[:-2]:
        with pytest.raises(SystemExit):
            cohort(*argv)
        assert text in capsys.readouterr().err, argv


def test_without_the_flag_the_namespace_and_the_done_tail_are_what_they_were():
    from mudiff_hip import constraints as Cn, lowres_volume as LV, volume as V
    args = V.build_argparser(VS.cli_argv())
    new = dict(known_lowres_volume=None, lowres_volume_extent_mm=None, lowres_volume_profile=None, lowres_volume_drop=None, lowres_volume_baseline=False)
    assert {k: getattr(args, k) for k in new} == new
    plain = argparse.Namespace(**{k: v for k, v in vars(args).items() if k not in new})
    for module in V.sampling_modes():
        assert module.options_from(plain) == module.options_from(args)                   # every mode reads the namespace as before
    assert LV.options_from(args) is None
    assert V._done_tail(args, 'auto') == V._done_tail(plain, 'auto') == ''
    args.constraint = Cn.FREE
    assert V._done_tail(args, 'auto') == ''
    assert Cn.Constraint.lockstep is False
    assert LV.LowresMeasurement.lockstep is True and LV.LowresMeasurement.tag == 'lowres_volume' and LV.LowresMeasurement.baseline_through_plane
