"""CPU: the host side of --known_thick_volume (mudiff_hip.thick_volume, ops.band_tables): the geometry and the
weights against the independent restatement in tests/band_ref.py, the tables and their limits, the flags' refusals, and the rounding
bounds the GPU tests hold csrc/band.hip to - the fp32 emulation of the kernel's chain stays below 0.6 of each, and a weight that is
wrong by 1e-3 breaks them."""
import argparse
import copy
import os
import re

import numpy as np
import pytest

import band_ref as R
import volume_support as VS
from conftest import REPO

SYMBOLS = ('mud_band_constrain', 'mud_band_measure')
# (n, first centre, spacing, thickness in thin slices, profile) -> (m, bandwidth, most members, cond(A A^T))
GEOMETRIES = {(12, 1.25, 2.5, 3.0, 'box'): (4, 1, 4, 2.0), (24, 3.25, 2.5, 3.0, 'gauss'): (7, 2, 7, 5.5),
              (24, 1.7, 1.0, 3.0, 'box'): (21, 3, 4, 478.0), (24, 1.0, 1.5, 3.0, 'box'): (15, 2, 4, 154.0)}


def test_symbols_are_declared_bound_and_the_struct_matches_the_header(tmp_path):
    import ctypes as C
    import subprocess
    import mudiff_hip
    from mudiff_hip import ops
    txt = re.sub(r'/\*.*?\*/', '', open(os.path.join(REPO, 'include', 'mudiff_hip.h')).read(), flags=re.S)
    for name in SYMBOLS:
        assert re.search(r'\b' + name + r'\s*\(', txt), name
        assert name in mudiff_hip._SIGNATURES and name in mudiff_hip.EXPORTED_SYMBOLS, name
    assert mudiff_hip.load().mud_version() >= 121
    assert ops.KIND_BAND == 8 and len({ops.KIND_X_INIT, ops.KIND_Z, ops.KIND_NOISE, ops.KIND_KNOWN, ops.KIND_RENOISE, ops.KIND_KSPACE,
                                       ops.KIND_THICK, ops.KIND_MULTISLICE, ops.KIND_BAND}) == 9
    for name, value in (('MEMBERS', ops.BAND_MAX_MEMBERS), ('BW', ops.BAND_MAX_BW), ('M', ops.BAND_MAX_M), ('N', ops.BAND_MAX_N)):
        assert re.search(rf'#define MUD_BAND_MAX_{name} {value}\b', txt), name
    cls = mudiff_hip.BandTables
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{os.path.join(REPO, "include", "mudiff_hip.h")}"', 'int main(void) {',
             '  printf("size %zu\\n", sizeof(mud_band_tables));']
    lines += [f'  printf("{f} %zu\\n", offsetof(mud_band_tables, {f}));' for f, _ in cls._fields_] + ['  return 0;', '}']
    (tmp_path / 'layout.c').write_text('\n'.join(lines))
    subprocess.run(['gcc', '-std=c11', '-o', str(tmp_path / 'layout'), str(tmp_path / 'layout.c')], check=True)
    out = subprocess.run([str(tmp_path / 'layout')], check=True, stdout=subprocess.PIPE, text=True).stdout
    for ln in out.strip().splitlines():
        field, val = ln.split()
        assert int(val) == (C.sizeof(cls) if field == 'size' else getattr(cls, field).offset), ln


@pytest.mark.parametrize('geom', list(GEOMETRIES))
def test_geometries_weights_and_tables(geom):
    from mudiff_hip import ops, thick_volume as TV
    m, bw, members, cond = GEOMETRIES[geom]
    n, c0, step, width, profile = geom
    A, centres, idx = R.weights(*geom)
    assert A.shape == (m, n) and idx == list(range(m)) and np.allclose(A.sum(1), 1.0, atol=1e-15) and (A >= 0).all()
    assert np.array_equal(centres, c0 + step * np.arange(m))
    assert np.abs(TV.weight_rows(n, centres, width, profile) - A).max() <= 1e-15          # the module's rows: the restatement's
    for j, c in enumerate(centres):                                                      # ... and its support rule
        lo, hi = TV.support(c, width, profile)
        assert (lo, hi) == R.support(c, width, profile) and lo >= -0.5 and hi <= n - 0.5
        assert set(np.flatnonzero(A[j])) == {i for i in range(n) if min(hi, i + 0.5) - max(lo, i - 0.5) > 0}
    tab = ops.band_tables(A)
    assert (tab.m, tab.n, tab.bw, tab.nnz) == (m, n, bw, int((A != 0).sum())) and int((A != 0).sum(1).max()) == members
    assert tab.bw == R.bandwidth(A) and tab.cond == pytest.approx(R.cond(A), rel=1e-9) and tab.cond == pytest.approx(cond, rel=0.02)
    # the CSR of A by thick slice and of A^T by thin slice, in ascending order, hold the fp32 weights
    A32 = R.as_kernel(A)
    for j in range(m):
        s = slice(tab.start[j], tab.start[j + 1])
        assert list(tab.member[s]) == list(np.flatnonzero(A32[j])) and np.array_equal(tab.w[s], A32[j, tab.member[s]].astype(np.float32))
    for i in range(n):
        s = slice(tab.tstart[i], tab.tstart[i + 1])
        assert list(tab.tmember[s]) == list(np.flatnonzero(A32[:, i])) and np.array_equal(tab.tw[s], A32[tab.tmember[s], i].astype(np.float32))
    # the banded Cholesky tables times their transpose reproduce G
    L = np.zeros((m, m))
    for j in range(m):
        L[j, j] = 1.0 / float(tab.lc[j, 0])
        for k in range(1, bw + 1):
            if j - k >= 0:
                L[j, j - k] = float(tab.lc[j, k])
    G = A32 @ A32.T
    assert np.abs(L @ L.T - G).max() <= 1e-6 * np.abs(G).max()
    # the same tables from the CSR form
    st = np.concatenate([[0], np.cumsum((A != 0).sum(1))])
    rows, cols = np.nonzero(A)
    again = ops.band_tables((st, cols, A[rows, cols], n))
    assert all(np.array_equal(getattr(again, f), getattr(tab, f)) for f in ('start', 'member', 'w', 'tstart', 'tmember', 'tw', 'lc'))


@pytest.mark.parametrize('L,gap,offset', [(3, 0, 0), (5, 0, 2), (4, 1, 1)])
def test_integer_box_layout_is_the_diagonal_mode(L, gap, offset):
    """Thick slices that start on a thin-slice boundary, a whole number of thin slices thick and apart: thick.layout's slabs, and under
    the box profile thick.profile_weights' weights, exactly.  (The gauss profile of this module is cut at +-T and integrated, not
    sampled at the centres: it agrees with thick's only in where the slabs are.)"""
    from mudiff_hip import thick as TK
    Z = 23
    A, centres, _ = R.weights(Z, offset + (L - 1) / 2.0, float(L + gap), float(L), 'box')
    slabs = [(a, b) for a, b, complete in TK.layout(Z, L, gap, offset) if complete]
    assert len(slabs) == A.shape[0] and R.bandwidth(A) == 0
    for j, (a, b) in enumerate(slabs):
        assert list(np.flatnonzero(A[j])) == list(range(a, b + 1)) and centres[j] == (a + b) / 2.0
        assert np.array_equal(A[j, a:b + 1], TK.profile_weights(L, 'box'))


def test_limits_and_the_condition_cap():
    from mudiff_hip import ops
    with pytest.raises(ValueError, match='cond'):                                        # two coincident thick slices
        ops.band_tables(np.array([[0.5, 0.5, 0.0], [0.5, 0.5, 0.0]]))
    with pytest.raises(ValueError, match='cond'):                                        # ... and two that nearly coincide
        ops.band_tables(R.weights(12, 2.0, 0.01, 3.0, 'box', count=2)[0])
    with pytest.raises(ValueError, match='256'):
        ops.band_tables(np.eye(257))
    with pytest.raises(ValueError, match='512'):
        ops.band_tables(np.ones((1, 513)) / 513)
    with pytest.raises(ValueError, match='32 members'):
        ops.band_tables(np.ones((1, 33)) / 33)
    with pytest.raises(ValueError, match='1 to 32 members'):
        ops.band_tables(np.array([[1.0, 0.0], [0.0, 0.0]]))
    with pytest.raises(ValueError, match='bandwidth'):
        ops.band_tables(R.weights(40, 5.0, 1.0, 10.0, 'box', count=12)[0])
    with pytest.raises(ValueError, match='finite'):
        ops.band_tables(np.array([[1.0, np.nan]]))
    with pytest.raises(ValueError, match='CSR'):
        ops.band_tables(([0, 2], [0], [1.0], 3))
    # the realistic cases: 155 thin slices at 1 mm, 5 mm slices from a fractional origin, contiguous and every 2.5 mm
    for step, m, bw in ((5.0, 30, 1), (2.5, 60, 2)):
        A, _, _ = R.weights(155, 2.3, step, 5.0, 'box', count=m)
        tab = ops.band_tables(A)
        print(f'155 thin slices, 5 mm every {step} mm: m {tab.m}, bandwidth {tab.bw}, cond {tab.cond:.4g}')
        assert (tab.m, tab.bw) == (m, bw) and tab.cond <= ops.BAND_MAX_COND
    assert ops.band_tables(R.weights(155, 2.3, 5.0, 5.0, 'box', count=30)[0]).cond < 2.0


def test_geometry_from_the_affines_and_its_refusals():
    from mudiff_hip import thick_volume as TV
    thin = np.array([[0.9, 0.0, 0.0, -80.0], [0.0, 0.9, 0.0, -95.0], [0.0, 0.0, 1.0, -60.0], [0.0, 0.0, 0.0, 1.0]])
    thick = thin.copy()
    thick[:3, 2] = [0.0, 0.0, 2.5]
    thick[:3, 3] = [-80.0, -95.0, -58.75]
    geo = TV.slice_geometry((16, 16, 24), thin, (16, 16, 7), thick)
    c0, step, dz = R.geometry(thin, thick)
    assert (geo['c0'], geo['step'], geo['thin_dz'], geo['thick_dz'], geo['m']) == (c0, step, dz, 2.5, 7) and (c0, step) == (1.25, 2.5)
    rot = np.eye(4)                                                                      # an oblique pair: both turned the same way
    a = 0.3
    rot[:3, :3] = [[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]
    geo = TV.slice_geometry((16, 16, 24), rot @ thin, (16, 16, 7), rot @ thick)
    assert geo['c0'] == pytest.approx(1.25, abs=1e-12) and geo['step'] == pytest.approx(2.5, abs=1e-12)

    def refused(edit, y_shape=(16, 16, 7)):
        b = thick.copy()
        for (r, c), v in edit.items():
            b[r, c] = v
        with pytest.raises(ValueError, match='--known_thick_volume.*out of scope'):
            TV.slice_geometry((16, 16, 24), thin, y_shape, b)

    refused({}, y_shape=(16, 12, 7))
    refused({(0, 0): 0.9 + 2e-3})                                                      # another in-plane voxel size
    refused({(0, 3): -80.0 + 2e-3})                                                    # an in-plane shift of the origin
    refused({(0, 2): 2.5 * np.sin(2e-3), (2, 2): 2.5 * np.cos(2e-3)})                  # a tilted slice axis
    refused({(2, 2): -2.5})                                                            # ... and a reversed one
    TV.slice_geometry((16, 16, 24), thin, (16, 16, 7), thick + 1e-4 * np.eye(4))         # inside the tolerances
    with pytest.raises(ValueError, match='3D'):
        TV.slice_geometry((16, 16, 24), thin, (16, 16), thick)


def _ns(**kw):
    return argparse.Namespace(**{**dict(seed=31, known_resample=1), **kw})


def test_flags_and_their_refusals(capsys):
    from mudiff_hip import thick_volume as TV, volume as V
    assert TV.options_from(_ns()) is None and TV.options_from(argparse.Namespace()) is None
    got = TV.options_from(_ns(known_thick_volume='y.nii.gz'))
    assert got == dict(volume='y.nii.gz', thickness=None, profile='box', drop=[], baseline=False, resample=1)
    got = TV.options_from(_ns(known_thick_volume='y.nii.gz', thick_volume_thickness_mm=5.0, thick_volume_profile='gauss', thick_volume_drop=['1:2', '7:7'],
                              thick_volume_baseline=True, known_resample=3))
    assert got == dict(volume='y.nii.gz', thickness=5.0, profile='gauss', drop=[(1, 2), (7, 7)], baseline=True, resample=3)
    for flag, kw in (('--thick_volume_thickness_mm', dict(thick_volume_thickness_mm=5.0)), ('--thick_volume_profile', dict(thick_volume_profile='box')),
                     ('--thick_volume_drop', dict(thick_volume_drop=['1:2'])), ('--thick_volume_baseline', dict(thick_volume_baseline=True))):
        with pytest.raises(ValueError, match=f'{flag} needs --known_thick_volume'):
            TV.options_from(_ns(**kw))
    for other, value in (('known_volume', 'k.nii.gz'), ('known_kspace', 'equispaced'), ('known_thick', 5), ('known_multislice', 'equispaced'),
                         ('known_mask', 'm.nii.gz'), ('known_drop_slices', ['1:2'])):
        with pytest.raises(ValueError, match=f'--known_thick_volume cannot be combined with --{other}'):
            TV.options_from(_ns(known_thick_volume='y.nii.gz', **{other: value}))
    for flag, kw in (('--thick_volume_thickness_mm', dict(thick_volume_thickness_mm=0.0)), ('--thick_volume_thickness_mm', dict(thick_volume_thickness_mm=float('nan'))),
                     ('--thick_volume_profile', dict(thick_volume_profile='sinc')), ('--thick_volume_drop', dict(thick_volume_drop=['3'])),
                     ('--thick_volume_drop', dict(thick_volume_drop=['4:2'])), ('--known_resample', dict(known_resample=0)),
                     ('--seed', dict(seed=-1)), ('manifest', dict(known_thick_volume='manifest'))):
        with pytest.raises(ValueError, match=flag):
            TV.options_from(_ns(**{**dict(known_thick_volume='y.nii.gz'), **kw}))
    assert TV.options_from(_ns(known_thick_volume='manifest', manifest='cohort.tsv'))['volume'] == 'manifest'
    # through the parser: the flags sit in a parser of their own, --known_resample goes with Y, and its old refusal is what it was
    args = V.build_argparser(VS.cli_argv('--known_thick_volume', 'y.nii.gz', '--known_resample', '2', '--thick_volume_drop', '0:1', '--thick_volume_baseline'))
    assert (args.known_thick_volume, args.known_resample, args.thick_volume_drop, args.thick_volume_baseline) == ('y.nii.gz', 2, ['0:1'], True)
    p = V.make_parser()
    new = ['--known_thick_volume', '--thick_volume_thickness_mm', '--thick_volume_profile', '--thick_volume_drop', '--thick_volume_baseline']
    assert [o for a in p.lates[-3]._actions for o in a.option_strings] == new
    assert V.measurement_modes()[:-1] == V.known_modes() and V.measurement_modes()[-1] is TV
    for argv, text in ((['--known_resample', '2'], '--known_resample needs --known_volume'),
                       (['--known_thick_volume', 'y.nii.gz', '--known_volume', 'k.nii.gz'], 'cannot be combined with --known_volume'),
                       (['--thick_volume_baseline'], '--thick_volume_baseline needs --known_thick_volume')):
        with pytest.raises(SystemExit):
            V.build_argparser(VS.cli_argv(*argv))
        assert text in capsys.readouterr().err


def test_constraint_defaults_and_the_lockstep_mark():
    from mudiff_hip import constraints as Cn, thick_volume as TV
    assert Cn.Constraint.lockstep is False and Cn.FREE.lockstep is False and Cn.KnownVoxels(None, None).lockstep is False
    assert TV.BandMeasurement.lockstep is True and TV.BandMeasurement.tag == 'thick_volume' and TV.BandMeasurement.baseline_through_plane


def _operands(A, seed, P=96):
    g = np.random.default_rng(seed)
    n = A.shape[1]
    x = g.standard_normal((n, P)).astype(np.float32)
    eta = g.standard_normal((n, P)).astype(np.float32)
    y = R.measure(np.tanh(g.standard_normal((n, P))).astype(np.float32), A).astype(np.float32)
    return x, y, eta


@pytest.mark.parametrize('geom', list(GEOMETRIES) + [(3, 1.0, 3.0, 3.0, 'box')])
def test_the_emulated_chain_stays_below_0p6_of_each_bound(geom):
    from mudiff_hip import ops
    A, _, _ = R.weights(*geom)
    tab = ops.band_tables(A)
    worst = dict(out=0.0, residual=0.0)
    for seed in range(4):
        x, y, eta = _operands(A, 1000 * seed + geom[0])
        for clean, (a, s) in ((False, (0.97, 0.2431)), (False, (0.12, 0.9928)), (True, (1.0, 0.0))):
            args = (x, y, A, eta, a, s, clean)
            got, want, bound = R.constrain_fp32(x, y, tab, eta, a, s, clean), R.constrain(*args), R.bound_out(*args)
            used = np.isfinite(bound)
            assert np.array_equal(got[~used].view(np.int32), x[~used].view(np.int32))    # free rows: untouched
            worst['out'] = max(worst['out'], float(np.max(np.abs(got.astype(np.float64) - want)[used] / bound[used])))
            if clean:
                res = np.abs(R.measure(got, A) - y.astype(np.float64))
                worst['residual'] = max(worst['residual'], float(np.max(res / R.bound_residual(x, y, A))))
    print(f'{geom}: worst emulation / bound: out {worst["out"]:.3f}, residual {worst["residual"]:.3f}')
    assert worst['out'] <= 0.6 and worst['residual'] <= 0.6


@pytest.mark.parametrize('geom', list(GEOMETRIES))
def test_a_weight_wrong_by_1e_3_breaks_the_bound(geom):
    """The bound is tight enough to catch a wrong kernel: one weight of the forward table changed by 1e-3 relative."""
    from mudiff_hip import ops
    A, _, _ = R.weights(*geom)
    tab = ops.band_tables(A)
    x, y, eta = _operands(A, 77)
    args = (x, y, A, eta, 0.81, 0.5864, False)
    want, bound = R.constrain(*args), R.bound_out(*args)
    used = np.isfinite(bound)
    for q in (0, tab.nnz // 2, tab.nnz - 1):
        wrong = copy.copy(tab)
        wrong.w = tab.w.copy()
        wrong.w[q] *= np.float32(1.001)
        err = np.abs(R.constrain_fp32(x, y, wrong, eta, 0.81, 0.5864, False).astype(np.float64) - want)
        assert (err[used] > bound[used]).any(), q


def test_interpolated_baseline_against_a_restatement():
    import torch
    from mudiff_hip import thick_volume as TV
    g = np.random.default_rng(5)
    y = g.standard_normal((4, 3, 3)).astype(np.float32)
    c = np.array([1.25, 3.75, 6.25, 8.75])
    got = TV.interpolate(torch.from_numpy(y), c, 12).numpy()
    for z in range(12):
        if z <= c[0]:
            want = y[0]
        elif z >= c[-1]:
            want = y[-1]
        else:
            j = int(np.searchsorted(c, z, side='right')) - 1
            f = (z - c[j]) / (c[j + 1] - c[j])
            want = (1 - f) * y[j] + f * y[j + 1]
        assert np.abs(got[z] - want).max() <= 1e-6
    assert (TV.interpolate(torch.zeros(0, 3, 3), c[:0], 5) == -1).all()
