"""Host: the multi-coil model of --known_sense (mudiff_hip.sense): the fp64 restatement tests/sense_ref.py against
dense linear algebra, the default coil maps, and the flags on both command lines."""
import argparse
import itertools
import os

import numpy as np
import pytest

import kspace_ref as KR
import sense_ref as R
import volume_support as VS
from conftest import REPO

SYMBOLS = ('mud_sense_constrain', 'mud_sense_measure', 'mud_sense_adjoint', 'mud_sense_ws_floats')
FLAGS = ['--known_sense', '--sense_accel', '--sense_center', '--sense_axis', '--sense_mask_file', '--sense_coils', '--sense_maps', '--sense_lambda',
         '--sense_iters', '--sense_noise', '--sense_baseline']
A_TAB = np.array([1.0, 0.97, 0.81, 0.5, 0.12])
S_TAB = np.sqrt(1 - A_TAB ** 2)


def _mask(S, accel=4, center=0.08, seed=3):
    from mudiff_hip import kspace
    return kspace.build_mask(S, 'equispaced', accel, center, 0, seed)[None]


def _operands(S, Nc, rows=2, seed=0):
    g = np.random.default_rng(1000 * S + 10 * Nc + seed)
    x, k, eta = (g.standard_normal((rows, S, S)) for _ in range(3))
    maps, m = R.coil_maps(S, Nc), _mask(S)
    return x, k, eta, maps, m, R.adjoint(R.measure(k, maps, m), maps)


def test_symbols_are_declared_and_bound():
    import re
    import mudiff_hip
    from mudiff_hip import ops
    txt = re.sub(r'/\*.*?\*/', '', open(os.path.join(REPO, 'include', 'mudiff_hip.h')).read(), flags=re.S)
    for name in SYMBOLS:
        assert re.search(r'\b' + name + r'\s*\(', txt), name
        assert name in mudiff_hip.EXPORTED_SYMBOLS, name
    lib = mudiff_hip.load()
    assert lib.mud_version() >= 123
    assert lib.mud_sense_ws_floats(2, 3, 32) == 2 * 2 * 3 * 1024 + 4 * 2 * 1024 + 4 * 2 * 2 and lib.mud_sense_ws_floats(2, 3, 24) == -1
    assert (ops.KIND_SENSE, ops.KIND_SENSE_MEAS, ops.SENSE_MAX_COILS) == (10, 11, 32)
    assert 'sense_constrain' in ops.randn_keyed.__doc__
    readme = open(os.path.join(REPO, 'README.md')).read()
    assert f'C ABI ({len(mudiff_hip.EXPORTED_SYMBOLS)} entry points)' in readme and '--known_sense' in readme


@pytest.mark.parametrize('S,Nc', [(16, 1), (16, 8), (32, 3), (256, 32)])
def test_coil_maps_have_unit_root_sum_of_squares_and_follow_the_formula(S, Nc):
    from mudiff_hip import sense
    C = sense.coil_maps(S, Nc)
    assert C.dtype == np.complex64 and C.shape == (Nc, S, S)
    assert np.array_equal(C, R.coil_maps(S, Nc).astype(np.complex64))
    assert np.abs((np.abs(C.astype(np.complex128)) ** 2).sum(0) - 1).max() <= 4 * Nc * 2.0 ** -24
    c, (iu, iv) = Nc // 2, (3, S - 2)                                            # one element, written out
    u, v, th = (iu - S // 2) / S, (iv - S // 2) / S, 2 * np.pi * (np.arange(Nc) + 0.5) / Nc
    m = np.exp(-((u - 0.75 * np.cos(th)) ** 2 + (v - 0.75 * np.sin(th)) ** 2) / (2 * 0.6 ** 2))
    want = m[c] * np.exp(1j * (th[c] + np.pi * (u * np.cos(th[c]) + v * np.sin(th[c])))) / np.sqrt((m ** 2).sum())
    assert abs(C[c, iu, iv] - want) <= 2.0 ** -23
    assert sense.load_maps(C, S) is not None


def test_load_maps_refuses_what_is_not_a_set_of_sensitivities(tmp_path):
    from mudiff_hip import sense
    C = sense.coil_maps(16, 4)
    np.save(tmp_path / 'ok.npy', C)
    assert np.array_equal(sense.load_maps(str(tmp_path / 'ok.npy'), 16), C)
    holes = C.copy()
    holes[:, :4] = 0                                                              # all zero there: allowed
    assert sense.load_maps(holes, 16).shape == (4, 16, 16)
    for bad in (C * 1.01, C[:, :8], C.real, np.repeat(C, 9, 0) / 3, np.where(np.arange(16) == 3, np.nan, C)):
        with pytest.raises(ValueError, match='--sense_maps'):
            sense.load_maps(bad, 16)
    assert np.abs((np.abs(C * 1.0004) ** 2).sum(0) - 1).max() < 1e-3 and sense.load_maps(C * np.complex64(1.0004), 16) is not None


@pytest.mark.parametrize('Nc', (1, 2, 4, 8))
def test_the_dense_normal_operator_is_symmetric_with_eigenvalues_in_0_1(Nc):
    S = 16
    N = R.dense_normal(R.coil_maps(S, Nc), _mask(S))
    assert np.abs(N - N.T).max() <= 1e-12
    w = np.linalg.eigvalsh(0.5 * (N + N.T))
    assert w.min() >= -1e-12 and w.max() <= 1 + 1e-12
    # <A x, z> = <x, A^H z>
    g = np.random.default_rng(Nc)
    x, z = g.standard_normal((1, S, S)), g.standard_normal((1, Nc, S, S)) + 1j * g.standard_normal((1, Nc, S, S))
    zm = np.where(_mask(S)[:, None] != 0, z, 0)
    assert abs((R.measure(x, R.coil_maps(S, Nc), _mask(S)) * np.conj(zm)).sum().real - (x * R.adjoint(zm, R.coil_maps(S, Nc))).sum()) <= 1e-12


@pytest.mark.parametrize('S,Nc', list(itertools.product((16, 32), (1, 2, 4, 8))))
def test_the_restatement_against_a_dense_solve(S, Nc):
    """lambda = 8, iters = 32, equispaced x4, centre 0.08: within 1e-10 relative of the dense solve of (I + lambda N) (measured: at most
    2.7e-14; at 8 iterations at most 6.6e-4, at 16 at most 3.5e-7).  For Nc in {1, 2} N has few distinct eigenvalues and CG terminates
    after 2 - 3 iterations: the guarded recurrence stays finite to 32."""
    x, k, eta, maps, m, ahy = _operands(S, Nc)
    t, toff = np.array([1, 3]), 0
    a, s = R.levels(2, t, toff, A_TAB, S_TAB, False)
    got, res = R.constrain(x, ahy, maps, m, 8.0, 32, eta, t, toff, A_TAB, S_TAB, False, with_res=True)
    assert np.isfinite(got).all() and np.isfinite(res).all()
    worst = 0.0
    for r in range(2):
        want = R.constrain_dense(x[r], ahy[r], maps, m[0], 8.0, eta[r], a[r], s[r])
        worst = max(worst, np.linalg.norm(got[r] - want) / np.linalg.norm(want))
    print(f'S={S} Nc={Nc}: restatement against the dense solve {worst:.3e}')
    assert worst <= 1e-10
    # the optimality residual of the minimiser is zero, and the data term never grows
    assert R.optimality(got, x, ahy, maps, m, 8.0, eta, a, s).max() <= 1e-10
    d = lambda v: np.sqrt((np.abs(R.measure(v - s[:, None, None] * eta, maps, m) - a[:, None, None, None] * R.measure(k, maps, m)) ** 2).sum((1, 2, 3)))  # noqa: E731
    for iters in (1, 2, 12, 32):
        step = R.constrain(x, ahy, maps, m, 8.0, iters, eta, t, toff, A_TAB, S_TAB, False)
        assert (d(step) <= d(x) * (1 + 1e-12)).all(), iters


def test_an_unguarded_recurrence_would_not_survive_exact_termination():
    """Nc = 1 at 32 iterations: r.r reaches a value whose successor divides 0 by 0 unless the row is frozen; the restatement reports the
    frozen row's cg_res as 0 or as a tiny finite number, never NaN, and b = 0 returns x_new."""
    x, k, eta, maps, m, ahy = _operands(16, 1)
    out, res = R.constrain(x, ahy, maps, m, 8.0, 32, eta, None, 0, None, None, True, with_res=True)
    assert np.isfinite(out).all() and (res < 1e-12).all()
    zero = np.zeros_like(m)
    out, res = R.constrain(x, 0 * ahy, maps, zero, 8.0, 32, eta, None, 0, None, None, True, with_res=True)
    assert np.array_equal(out, x) and (res == 0).all()


@pytest.mark.parametrize('Nc', (1, 3, 8))
def test_a_full_mask_is_solved_in_one_iteration(Nc):
    """M = 1: N = I (unit root-sum-of-squares), so x = (x_new + lambda t) / (1 + lambda) with t = a k + s eta."""
    S, lam = 16, 8.0
    x, k, eta, maps, _, _ = _operands(S, Nc)
    m = np.ones((1, S, S), np.uint8)
    ahy = R.adjoint(R.measure(k, maps, m), maps)
    assert np.abs(ahy - k).max() <= 1e-12
    t = np.array([2, 4])
    a, s = R.levels(2, t, 0, A_TAB, S_TAB, False)
    got = R.constrain(x, ahy, maps, m, lam, 1, eta, t, 0, A_TAB, S_TAB, False)
    want = (x + lam * (a[:, None, None] * k + s[:, None, None] * eta)) / (1 + lam)
    assert np.abs(got - want).max() <= 1e-12


def test_one_uniform_coil_and_a_hermitian_mask_reduce_to_the_single_coil_projection():
    """Nc = 1, C = 1, M Hermitian: N is the projection of mud_kspace_constrain, so the step is x_new - lambda / (1 + lambda) times its
    correction."""
    S, lam = 16, 8.0
    g = np.random.default_rng(5)
    x, k, eta = (g.standard_normal((2, S, S)) for _ in range(3))
    m = KR.symmetrise(_mask(S))
    maps = np.ones((1, S, S), np.complex128)
    y = KR.measure(k, m)
    t = np.array([0, 3])
    got = R.constrain(x, R.adjoint(y[:, None], maps), maps, m, lam, 4, eta, t, 1, A_TAB, S_TAB, False)
    correction = x - KR.constrain(x, y, m, eta, t, 1, A_TAB, S_TAB, False)
    assert np.abs(got - (x - lam / (1 + lam) * correction)).max() <= 1e-12


# ---------------------------------------------------------------------------------------------------
# the flags
# ---------------------------------------------------------------------------------------------------
KV = dict(known_volume='k.nii.gz')
SN = dict(KV, known_sense='equispaced')
PATTERNS = "('equispaced', 'random', 'lowres', 'file')"
REFUSALS = [
    (dict(sense_accel=2), '--sense_accel needs --known_sense'), (dict(sense_center=0.1), '--sense_center needs --known_sense'),
    (dict(sense_axis=1), '--sense_axis needs --known_sense'), (dict(sense_mask_file='m.npy'), '--sense_mask_file needs --known_sense'),
    (dict(sense_coils=4), '--sense_coils needs --known_sense'), (dict(sense_maps='c.npy'), '--sense_maps needs --known_sense'),
    (dict(sense_lambda=1.0), '--sense_lambda needs --known_sense'), (dict(sense_iters=3), '--sense_iters needs --known_sense'),
    (dict(sense_noise=0.1), '--sense_noise needs --known_sense'), (dict(sense_baseline=True), '--sense_baseline needs --known_sense'),
    (dict(KV, known_sense='spiral'), f"--known_sense must be one of {PATTERNS}, got 'spiral'"),
    (dict(known_sense='equispaced'), '--known_sense needs --known_volume'),
    (dict(SN, known_mask='m.nii.gz'), '--known_sense cannot be combined with --known_mask (a voxel mask has no meaning in k-space; use '
                                      '--known_drop_slices for slices that were not measured)'),
    (dict(SN, known_kspace='random'), '--known_sense cannot be combined with --known_kspace: one measurement model per run'),
    (dict(SN, known_thick=3), '--known_sense cannot be combined with --known_thick: one measurement model per run'),
    (dict(SN, known_multislice='random'), '--known_sense cannot be combined with --known_multislice: one measurement model per run'),
    (dict(SN, known_thick_volume='y.nii.gz'), '--known_sense cannot be combined with --known_thick_volume: one measurement model per run'),
    (dict(SN, known_lowres_volume='y.nii.gz'), '--known_sense cannot be combined with --known_lowres_volume: one measurement model per run'),
    (dict(SN, image_size=96), '--known_sense needs an --image_size that is a power of two in [16, 512], got 96'),
    (dict(SN, sense_accel=0), '--sense_accel must be an integer >= 1, got 0'),
    (dict(SN, sense_center=1.5), '--sense_center must lie in [0, 1], got 1.5'),
    (dict(SN, sense_axis=2), '--sense_axis must be 0 or 1, got 2'),
    (dict(SN, sense_mask_file='m.npy'), '--sense_mask_file goes with --known_sense file, and that pattern needs it'),
    (dict(KV, known_sense='file'), '--sense_mask_file goes with --known_sense file, and that pattern needs it'),
    (dict(SN, sense_coils=4, sense_maps='c.npy'), '--sense_coils cannot be combined with --sense_maps: the file says how many coils there are'),
    (dict(SN, sense_coils=0), '--sense_coils must be an integer in [1, 32], got 0'),
    (dict(SN, sense_coils=33), '--sense_coils must be an integer in [1, 32], got 33'),
    (dict(SN, sense_lambda=-1.0), '--sense_lambda must be finite and >= 0, got -1.0'),
    (dict(SN, sense_lambda=float('inf')), '--sense_lambda must be finite and >= 0, got inf'),
    (dict(SN, sense_iters=0), '--sense_iters must be an integer in [1, 64], got 0'),
    (dict(SN, sense_iters=65), '--sense_iters must be an integer in [1, 64], got 65'),
    (dict(SN, sense_noise=-0.5), '--sense_noise must be finite and >= 0, got -0.5'),
    (dict(SN, seed=-1), '--known_sense needs a --seed in [0, 2^64) (its draws are keyed)'),
    (dict(SN, seed=1 << 64), '--known_sense needs a --seed in [0, 2^64) (its draws are keyed)'),
    # two faults: the order of the checks
    (dict(known_sense='equispaced', known_mask='m.nii.gz'), '--known_sense needs --known_volume'),
    (dict(SN, known_mask='m.nii.gz', known_kspace='random'), '--known_sense cannot be combined with --known_mask (a voxel mask has no meaning in '
                                                             'k-space; use --known_drop_slices for slices that were not measured)'),
    (dict(SN, image_size=96, sense_accel=0), '--known_sense needs an --image_size that is a power of two in [16, 512], got 96'),
    (dict(SN, sense_iters=0, seed=-1), '--sense_iters must be an integer in [1, 64], got 0'),
]


@pytest.mark.parametrize('fields,message', REFUSALS, ids=[str(i) for i in range(len(REFUSALS))])
def test_every_refusal_names_its_flag(fields, message):
    from mudiff_hip import sense
    with pytest.raises(ValueError) as e:
        sense.options_from(argparse.Namespace(**fields))
    assert str(e.value) == message


def test_what_is_taken():
    from mudiff_hip import sense
    assert sense.options_from(argparse.Namespace()) is None and sense.options_from(argparse.Namespace(**KV)) is None
    assert sense.options_from(argparse.Namespace(known_sense='lowres', manifest='m.tsv')) == \
        dict(pattern='lowres', accel=4, center=0.08, axis=0, mask_file=None, coils=8, maps=None, lam=8.0, iters=12, noise=0.0, baseline=False)
    got = sense.options_from(argparse.Namespace(**KV, known_sense='file', sense_mask_file='m.npy', sense_accel=1, sense_center=1, sense_axis=1,
                                                sense_maps='c.npy', sense_lambda=0, sense_iters=64, sense_noise=0.5, sense_baseline=True,
                                                image_size=512, seed=(1 << 64) - 1))
    assert got == dict(pattern='file', accel=1, center=1.0, axis=1, mask_file='m.npy', coils=8, maps='c.npy', lam=0.0, iters=64, noise=0.5, baseline=True)


def test_flags_and_their_refusals_on_both_command_lines(capsys):
    from mudiff_hip import cohort as Co, sense, volume as V
    args = V.build_argparser(VS.cli_argv('--known_volume', 'k.nii.gz', '--known_sense', 'random', '--sense_accel', '3', '--sense_coils', '12',
                                         '--sense_lambda', '2.5', '--sense_iters', '7', '--sense_noise', '0.01', '--sense_baseline', '--image_size', '64'))
    assert (args.known_sense, args.sense_accel, args.sense_coils, args.sense_lambda, args.sense_iters, args.sense_noise, args.sense_baseline) == \
        ('random', 3, 12, 2.5, 7, 0.01, True)
    # a late parser of its own, created before --known_thick_volume's: the pinned places stay what they were
    p = V.make_parser()
    flags = lambda late: [o for a in late._actions for o in a.option_strings]            # noqa: E731
    mine = [i for i, late in enumerate(p.lates) if flags(late) == FLAGS]
    assert len(mine) == 1 and not any(o in FLAGS for late in [p] + [q for i, q in enumerate(p.lates) if i != mine[0]] for o in flags(late))
    assert mine[0] == len(p.lates) - 4 and '--known_thick_volume' in flags(p.lates[-3]) and '--known_volume' in flags(p.lates[-2])
    assert '--known_multislice' in flags(p.lates[mine[0] - 1]) and '--unring' in flags(p.lates[1]) and '--ensemble_quantiles' in flags(p.lates[-1])
    assert V.constraint_modes()[:-1] == V.sampling_modes() and V.constraint_modes()[-1] is sense
    assert len(V.known_modes()) == 4 and len(V.measurement_modes()) == 5 and len(V.sampling_modes()) == 6
    known = ['--known_volume', 'k.nii.gz', '--known_sense', 'equispaced']
    refusals = [(['--sense_coils', '4'], '--sense_coils needs --known_sense'), (['--sense_baseline'], '--sense_baseline needs --known_sense'),
                (['--known_sense', 'equispaced'], '--known_sense needs --known_volume'),
                (known + ['--known_mask', 'm.nii.gz'], '--known_sense cannot be combined with --known_mask'),
                (known + ['--known_kspace', 'random'], '--known_sense cannot be combined with --known_kspace'),
                (known + ['--known_thick', '3'], '--known_sense cannot be combined with --known_thick'),
                (known + ['--known_multislice', 'random', '--multislice_thick', '2'], '--known_sense cannot be combined with --known_multislice'),
                (known + ['--known_thick_volume', 'y.nii.gz'], '--known_sense cannot be combined with --known_thick_volume'),
                (known + ['--known_lowres_volume', 'y.nii.gz'], '--known_sense cannot be combined with --known_lowres_volume'),
                (known + ['--image_size', '96'], '--known_sense needs an --image_size'), (known + ['--sense_axis', '2'], '--sense_axis must be 0 or 1'),
                (known + ['--sense_coils', '33'], '--sense_coils must be'), (known + ['--sense_coils', '4', '--sense_maps', 'c.npy'], '--sense_coils cannot'),
                (known + ['--sense_lambda', '-1'], '--sense_lambda must be'), (known + ['--sense_iters', '0'], '--sense_iters must be'),
                (known + ['--sense_noise', 'nan'], '--sense_noise must be'), (known + ['--known_sense', 'spiral'], 'invalid choice'),
                (known + ['--seed', '-1'], 'needs a --seed in [0, 2^64)')]
    for argv, text in refusals:
        with pytest.raises(SystemExit):
            V.build_argparser(VS.cli_argv(*argv))
        assert text in capsys.readouterr().err, argv
    # ... and through the cohort's, where K is the manifest's `known` column
    cohort = lambda *extra: Co.build_argparser(['--manifest', 'cohort.tsv'] + VS.cli_argv(*extra))      # noqa: E731
    assert cohort('--known_sense', 'lowres', '--sense_coils', '2').sense_coils == 2
    for argv, text in refusals:
        argv = [a for a in argv if a not in ('--known_volume', 'k.nii.gz')]
        if text in ('--known_sense needs --known_volume', '--known_sense cannot be combined with --known_mask'):
            continue                                                                      # (a cohort: the manifest names K and its mask)
        with pytest.raises(SystemExit):
            cohort(*argv)
        assert text in capsys.readouterr().err, argv


def test_without_the_flags_the_namespace_is_what_it_was():
    from mudiff_hip import sense, volume as V
    args = V.build_argparser(VS.cli_argv())
    new = {f[2:]: None for f in FLAGS}
    new['sense_baseline'] = False
    assert {k: getattr(args, k) for k in new} == new
    plain = argparse.Namespace(**{k: v for k, v in vars(args).items() if k not in new})      # as the parser left it before these flags
    assert sense.options_from(plain) is None and sense.suffix(None) == ''
    for module in V.constraint_modes():
        assert module.options_from(plain) == module.options_from(args)
