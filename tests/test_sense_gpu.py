"""GPU: the multi-coil measurement, its adjoint and the iterative data-consistency step (csrc/sense.hip: mud_sense_measure,
mud_sense_adjoint, mud_sense_constrain; ops.sense_*) against the fp64 restatement in tests/sense_ref.py.  DESIGN.md section 5.32.

The accuracy rule of the step: its per-slice L2 error against the restatement at the same `iters` stays within 4 x the error of the
same recurrence in torch fp32 / complex64 on the CPU (the margin tests/test_kspace_gpu.py gives two fp32 chains that differ only in
summation order); a slice whose largest error is below one fp32 ulp of the result's largest magnitude is not compared by ratio."""
import ctypes as C
import functools
import itertools

import numpy as np
import pytest
import torch

import kspace_ref as KR
import sense_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SIZES = (16, 32)                   # one line tile per slice; two, and a radix-2 tail
ROWS = (1, 3, 5)
COILS = (1, 2, 3, 8)
ITERS = (1, 2, 12, 32)
LAMBDAS = (1.0, 8.0, 64.0)
NTAB = 5
FACTOR = 4.0
ULP = 2.0 ** -23


def _tables():
    a = np.array([0.99999994, 0.97, 0.81, 0.5, 0.12], np.float32)
    return a, np.sqrt(1 - a.astype(np.float64) ** 2).astype(np.float32)


def _dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).to(DEV)      # (a copy: the shared cases are read-only)


def _cpu(a):
    return torch.from_numpy(np.array(a))


def _l2(a):
    a = np.asarray(a)
    return np.sqrt((np.abs(a.astype(np.complex128 if np.iscomplexobj(a) else np.float64)) ** 2).reshape(a.shape[0], -1).sum(1))


def _bits(v):
    return v.contiguous().view(torch.int32)


@functools.lru_cache(maxsize=None)
def _case(S, rows, Nc):
    """Operands of one shape, shared and never written: x_new, the target k, eta, per-row levels with clamped ends, masks and maps by
    their number of rows (maps of row r: the default ones rolled by r lines, which keeps the unit root-sum-of-squares), the noisy
    measurement y of k and A^H y in fp32 as every side is given them."""
    g = np.random.default_rng(9000 + 100 * S + 10 * rows + Nc)
    x = g.standard_normal((rows, S, S)).astype(np.float32)
    k = np.tanh(g.standard_normal((rows, S, S))).astype(np.float32)
    eta = g.standard_normal((rows, S, S)).astype(np.float32)
    t = g.integers(-2, NTAB + 2, rows).astype(np.int64)
    t[0] = -1
    if rows >= 2:
        t[-1] = NTAB + 1
    base = R.coil_maps(S, Nc).astype(np.complex64)
    maps = {1: base[None].copy(), rows: np.stack([np.roll(base, r, 1) for r in range(rows)])}
    masks = {}
    for mr in {1, rows}:
        m = (g.random((mr, S, S)) < 0.3).astype(np.uint8)
        m[:, 0, 0] = 1
        masks[mr] = m
    ys, ahys = {}, {}
    for mr, pr in itertools.product(sorted(masks), sorted(maps)):
        y = R.measure(k, maps[pr], masks[mr])
        noise = 0.05 * (g.standard_normal(y.shape) + 1j * g.standard_normal(y.shape))
        ys[mr, pr] = np.where(y != 0, y + noise, 0).astype(np.complex64)
        ahys[mr, pr] = R.adjoint(ys[mr, pr], maps[pr]).astype(np.float32)
    for a in (x, k, eta, t, *maps.values(), *masks.values(), *ys.values(), *ahys.values()):
        a.setflags(write=False)
    return x, k, eta, t, masks, maps, ys, ahys


# ---- the same chain in torch on the CPU: fp32 / complex64 ------------------------------------------------------------------------------
def _t_normal(x, maps, mask):
    F = torch.fft.fft2(maps * x[:, None], norm='ortho')
    F = torch.where(mask[:, None], F, torch.zeros((), dtype=torch.complex64))
    return (maps.conj() * torch.fft.ifft2(F, norm='ortho')).sum(1).real


def _torch_chain(x_new, ahy, maps, mask, lam, iters, eta, a, s, with_res=False):
    x_new, ahy, maps, mask = _cpu(x_new), _cpu(ahy), _cpu(maps), _cpu(mask) != 0
    rows = x_new.shape[0]
    maps, mask = maps.expand(rows, *maps.shape[1:]), mask.expand(rows, *mask.shape[1:])
    a, s, lam = torch.from_numpy(a.astype(np.float32)), torch.from_numpy(s.astype(np.float32)), np.float32(lam)
    dot = lambda u, v: (u * v).sum((1, 2))                                               # noqa: E731
    d = x_new if eta is None else x_new - s[:, None, None] * _cpu(eta)
    b = _t_normal(d, maps, mask) - a[:, None, None] * ahy
    e, r, p = torch.zeros_like(b), b.clone(), b.clone()
    rr, bb = dot(r, r), dot(b, b)
    frozen = torch.zeros(rows, dtype=torch.bool)
    one, zero = torch.ones(()), torch.zeros(())
    for _ in range(iters):
        q = p + lam * _t_normal(p, maps, mask)
        pq = dot(p, q)
        frozen |= (rr == 0) | (pq == 0)
        alpha = torch.where(frozen, zero, rr / torch.where(frozen, one, pq))
        e = e + alpha[:, None, None] * p
        r = r - alpha[:, None, None] * q
        rr_new = torch.where(frozen, zero, dot(r, r))
        beta = torch.where(rr_new == 0, zero, rr_new / torch.where(rr == 0, one, rr))
        p = r + beta[:, None, None] * p
        rr = rr_new
    out = (x_new - lam * e).numpy()
    res = torch.where((rr == 0) | (bb == 0), zero, torch.sqrt(rr / torch.where(bb == 0, one, bb))).numpy()
    return (out, res) if with_res else out


def _compare(tag, got, chain, want):
    """The rule of the module docstring, per slice -> the worst ratio among the slices compared by ratio."""
    err, terr = _l2(got - want), _l2(chain - want)
    small = np.abs(got - want).reshape(got.shape[0], -1).max(1) <= ULP * np.abs(want).reshape(got.shape[0], -1).max(1)
    ratio = err / np.maximum(terr, 1e-300)
    print(f'{tag}: error {err.max():.3e}, torch CPU fp32 {terr.max():.3e}, ratio {np.where(small, 0, ratio).max():.3f}')
    assert (small | (err <= FACTOR * terr)).all(), (tag, err, terr)
    return float(np.where(small, 0, ratio).max())


# ---------------------------------------------------------------------------------------------------
# the measurement and its adjoint
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('S,rows,Nc', list(itertools.product(SIZES, ROWS, COILS)) + [(256, 3, 2), (512, 1, 1)])
def test_measure_and_adjoint_against_the_restatement(S, rows, Nc):
    from mudiff_hip import ops
    x, k, eta, t, masks, maps, ys, ahys = _case(S, rows, Nc)
    g = np.random.default_rng(S + rows + Nc)
    for mr, pr in itertools.product(sorted(masks), sorted(maps)):
        want = R.measure(x, maps[pr], masks[mr])
        got = ops.sense_measure(_dev(x), _dev(maps[pr]), _dev(masks[mr]))
        assert got.dtype == torch.complex64 and tuple(got.shape) == (rows, Nc, S, S)
        got = got.cpu().numpy()
        assert (_l2(got - want) <= KR.rule(S) * _l2(want)).all(), (mr, pr, _l2(got - want) / _l2(want))
        assert not got[np.broadcast_to(masks[mr][:, None] == 0, got.shape)].any()             # exact zeros where nothing is measured
        z = (g.standard_normal(want.shape) + 1j * g.standard_normal(want.shape)).astype(np.complex64)
        zd = _dev(z)
        adj = ops.sense_adjoint(zd, _dev(maps[pr] if pr > 1 else maps[pr][0]))                # [Nc,S,S] is taken as one set
        assert torch.equal(zd.cpu(), _cpu(z))                                                 # the input is left alone
        assert adj.dtype == torch.float32 and tuple(adj.shape) == (rows, S, S)
        wadj = R.adjoint(z, maps[pr])
        assert (_l2(adj.cpu().numpy() - wadj) <= KR.rule(S) * _l2(wadj)).all(), (mr, pr, _l2(adj.cpu().numpy() - wadj) / _l2(wadj))
        # <A x, z> = <x, A^H z> with z masked, each side from the device's results, to fp32 rounding: both sides are within the rule
        zm = np.where(masks[mr][:, None] != 0, z, 0).astype(np.complex64)
        adjm = ops.sense_adjoint(_dev(zm), _dev(maps[pr])).cpu().numpy().astype(np.float64)
        lhs = (got.astype(np.complex128) * np.conj(zm.astype(np.complex128))).reshape(rows, -1).sum(1).real
        rhs = (x.astype(np.float64) * adjm).reshape(rows, -1).sum(1)
        assert (np.abs(lhs - rhs) <= 2 * KR.rule(S) * _l2(x) * _l2(zm)).all(), (lhs, rhs)


# ---------------------------------------------------------------------------------------------------
# the constraint
# ---------------------------------------------------------------------------------------------------
def _run(ops, case, mr, pr, lam, iters, toff, clean, **kw):
    x, k, eta, t, masks, maps, ys, ahys = case
    a_tab, s_tab = _tables()
    res = torch.empty(x.shape[0], device=DEV)
    out, res = ops.sense_constrain(_dev(x), _dev(ahys[mr, pr]), _dev(masks[mr]), _dev(maps[pr]), lam, iters, _dev(t), toff, _dev(a_tab), _dev(s_tab),
                                   noise=_dev(eta), clean=clean, cg_res=res, **kw)
    return out, res


def _sides(case, mr, pr, lam, iters, toff, clean):
    """(the restatement's result and cg_res, the torch chain's)."""
    x, k, eta, t, masks, maps, ys, ahys = case
    a_tab, s_tab = _tables()
    a, s = R.levels(x.shape[0], t, toff, a_tab, s_tab, clean)
    want = R.constrain(x, ahys[mr, pr], maps[pr], masks[mr], lam, iters, eta, t, toff, a_tab, s_tab, clean, with_res=True)
    chain = _torch_chain(x, ahys[mr, pr], maps[pr], masks[mr], lam, iters, None if clean else eta, a, s, with_res=True)
    return want, chain


def _check_res(tag, got, want):
    ok = ((got <= FACTOR * want) & (want <= FACTOR * got)) | ((got < 1e-6) & (want < 1e-6))
    assert ok.all(), (tag, got, want)


@pytest.mark.parametrize('Nc', COILS)
@pytest.mark.parametrize('rows', ROWS)
@pytest.mark.parametrize('S', SIZES)
def test_constrain_with_injected_noise_against_the_restatement(S, rows, Nc):
    """Every (iters, lambda) with two of the sixteen (toff, clean, mask rows, map rows), so that each shape sees all sixteen."""
    from mudiff_hip import ops
    case = _case(S, rows, Nc)
    extras = list(itertools.product((0, 1), (False, True), (1, rows), (1, rows)))
    worst = 0.0
    for i, (iters, lam) in enumerate(itertools.product(ITERS, LAMBDAS)):
        for j in (0, 1):
            toff, clean, mr, pr = extras[(2 * i + j) % len(extras)]
            (want, wres), (chain, _) = _sides(case, mr, pr, lam, iters, toff, clean)
            got, res = _run(ops, case, mr, pr, lam, iters, toff, clean)
            tag = f'S={S} rows={rows} Nc={Nc} iters={iters} lambda={lam:g} toff={toff} clean={clean} mask_rows={mr} map_rows={pr}'
            worst = max(worst, _compare(tag, got.cpu().numpy(), chain, want))
            _check_res(tag, res.cpu().numpy().astype(np.float64), wres)
    print(f'constrain S={S} rows={rows} Nc={Nc}: worst error / torch CPU fp32 error {worst:.3f}')


@pytest.mark.parametrize('S,rows,Nc,iters', [(256, 3, 2, 2), (512, 1, 1, 1)])
def test_constrain_at_the_large_sizes(S, rows, Nc, iters):
    """S = 256: production; S = 512: 8 lines per workgroup."""
    from mudiff_hip import ops
    case = _case(S, rows, Nc)
    for toff, clean, mr, pr in ((0, False, rows, 1), (1, True, 1, rows)):
        (want, wres), (chain, _) = _sides(case, mr, pr, 8.0, iters, toff, clean)
        got, res = _run(ops, case, mr, pr, 8.0, iters, toff, clean)
        _compare(f'S={S} clean={clean}', got.cpu().numpy(), chain, want)
        _check_res(S, res.cpu().numpy().astype(np.float64), wres)


@pytest.mark.parametrize('Nc', COILS)
@pytest.mark.parametrize('rows', ROWS)
@pytest.mark.parametrize('S', SIZES)
def test_constrain_keyed_draw_in_place_alone_twice_and_the_bits_of_x_new(S, rows, Nc):
    from mudiff_hip import ops
    x, k, eta, t, masks, maps, ys, ahys = case = _case(S, rows, Nc)
    a_tab, s_tab = _tables()
    at, st, xd, td, ed = _dev(a_tab), _dev(s_tab), _dev(x), _dev(t), _dev(eta)
    m, mp, ahy = _dev(masks[rows]), _dev(maps[rows]), _dev(ahys[rows, rows])
    lam, iters = 8.0, 12
    # the keyed draw is the injected ops.randn_keyed row, bit for bit
    g = np.random.default_rng(rows)
    keys = np.stack([g.integers(0, 200, rows), g.integers(0, 16, rows)], 1).astype(np.int64)
    seed, step = 2024, 3
    draw = ops.randn_keyed(torch.from_numpy(keys), S * S, seed, step, ops.KIND_SENSE).to(DEV).view(rows, S, S)
    want = ops.sense_constrain(xd, ahy, m, mp, lam, iters, td, 0, at, st, noise=draw)
    got = ops.sense_constrain(xd, ahy, m, mp, lam, iters, td, 0, at, st, keys=keys, seed=seed, step=step)
    assert torch.equal(_bits(got), _bits(want))
    assert not torch.equal(_bits(got), _bits(ops.sense_constrain(xd, ahy, m, mp, lam, iters, td, 0, at, st, keys=keys, seed=seed, step=step + 1)))
    # out is x_new, and two runs: the same bits, with and without a draw; [rows, 1, S, S] as the sampler holds it
    for clean in (False, True):
        want, wres = _run(ops, case, rows, rows, lam, iters, 0, clean)
        again, ares = _run(ops, case, rows, rows, lam, iters, 0, clean)
        assert torch.equal(_bits(again), _bits(want)) and torch.equal(_bits(ares), _bits(wres))
        inplace = xd.clone()
        assert ops.sense_constrain(inplace, ahy, m, mp, lam, iters, td, 0, at, st, noise=ed, clean=clean, out=inplace) is inplace
        assert torch.equal(_bits(inplace), _bits(want))
        assert torch.equal(_bits(ops.sense_constrain(xd[:, None], ahy, m, mp, lam, iters, td, 0, at, st, noise=ed[:, None], clean=clean)[:, 0]), _bits(want))
        # a row alone is the row in its batch
        for r in {0, rows - 1}:
            s = slice(r, r + 1)
            res = torch.empty(1, device=DEV)
            alone = ops.sense_constrain(xd[s], ahy[s], m[s], mp[s], lam, iters, td[s], 0, at, st, noise=ed[s], clean=clean, cg_res=res)[0]
            assert torch.equal(_bits(alone), _bits(want[s])) and torch.equal(_bits(res), _bits(wres[s]))
    # a zero mask, lambda = 0 and an all-zero map set: the bits of x_new, a negative zero included
    xz = xd.clone()
    xz[0, 0, :4] = torch.tensor([-0.0, 0.0, -1.5, 2.5], device=DEV)
    for clean in (False, True):
        for mr in {1, rows}:
            zero = torch.zeros(mr, S, S, device=DEV, dtype=torch.uint8)
            res = torch.full((rows,), 7.0, device=DEV)
            got = ops.sense_constrain(xz, torch.zeros_like(ahy), zero, mp, lam, iters, td, 0, at, st, noise=ed, clean=clean, cg_res=res)[0]
            assert torch.equal(_bits(got), _bits(xz)) and bool((res == 0).all())
        assert torch.equal(_bits(ops.sense_constrain(xz, ahy, m, mp, 0.0, iters, td, 0, at, st, noise=ed, clean=clean)), _bits(xz))
        assert torch.equal(_bits(ops.sense_constrain(xz, torch.zeros_like(ahy), m, torch.zeros_like(mp), lam, iters, td, 0, at, st, noise=ed, clean=clean)),
                           _bits(xz))


@pytest.mark.parametrize('rows', ROWS)
@pytest.mark.parametrize('S', SIZES)
def test_one_coil_stays_finite_past_its_exact_termination(S, rows):
    """Nc = 1: N has few distinct eigenvalues and CG ends long before 32 iterations; the result then stays what it was at 12."""
    from mudiff_hip import ops
    case = _case(S, rows, 1)
    for clean in (False, True):
        (want, _), (chain, _) = _sides(case, 1, 1, 8.0, 12, 0, clean)
        for iters in (12, 32):
            got, res = _run(ops, case, 1, 1, 8.0, iters, 0, clean)
            assert bool(torch.isfinite(got).all()) and bool(torch.isfinite(res).all())
            _compare(f'S={S} rows={rows} Nc=1 iters={iters}', got.cpu().numpy(), chain, want)


def test_bad_arguments_are_refused_before_a_launch():
    import mudiff_hip
    from mudiff_hip import MudiffHipError, ops
    lib = mudiff_hip.load()
    rows, S, Nc = 3, 16, 2
    f = dict(device=DEV, dtype=torch.float32)
    x, out, ahy, res = torch.randn(rows, S, S, **f), torch.full((rows, S, S), 7.0, **f), torch.zeros(rows, S, S, **f), torch.full((rows,), 7.0, **f)
    work = torch.zeros(ops.sense_ws_floats(rows, Nc, S), **f)
    assert work.numel() == 2 * rows * Nc * S * S + 4 * rows * S * S + 4 * rows and lib.mud_sense_ws_floats(rows, 33, S) == -1
    maps = torch.ones(rows, Nc, S, S, device=DEV, dtype=torch.complex64)
    y = torch.zeros(rows, Nc, S, S, device=DEV, dtype=torch.complex64)
    m = torch.ones(rows, S, S, device=DEV, dtype=torch.uint8)
    p = lambda v: None if v is None else C.c_void_p(v.data_ptr())                        # noqa: E731

    def call(S_=S, mask_rows=rows, map_rows=rows, coils=Nc, lam=8.0, iters=2, work_=work, kind=10, step=0, x_=x, ahy_=ahy, maps_=maps, res_=res,
             rows_=rows):
        return lib.mud_sense_constrain(p(x_), p(ahy_), p(m), mask_rows, p(maps_), map_rows, coils, lam, iters, None, None, 0, step, kind, None, 0, None,
                                       None, 1, 1, p(out), p(res_), p(work_), rows_, S_, None)

    assert call() == 0
    torch.cuda.synchronize()
    out.fill_(7.0)
    res.fill_(7.0)
    for kw in (dict(S_=24), dict(S_=1024), dict(S_=8), dict(mask_rows=2), dict(map_rows=2), dict(coils=0), dict(coils=33), dict(iters=0),
               dict(iters=65), dict(lam=-1.0), dict(lam=float('inf')), dict(lam=float('nan')), dict(work_=None), dict(kind=16), dict(kind=-1),
               dict(step=-1), dict(step=1 << 24), dict(x_=None), dict(ahy_=None), dict(maps_=None), dict(res_=None), dict(work_=out), dict(work_=x),
               dict(rows_=0), dict(S_=512, rows_=1024, mask_rows=1, map_rows=1, coils=8)):
        assert call(**kw) == 1 and b'mud_sense_constrain' in lib.mud_last_error(), kw
    inside = work[8:8 + rows * S * S].view(rows, S, S)                                    # an operand inside the workspace
    assert call(ahy_=inside) == 1 and b'work' in lib.mud_last_error()
    assert lib.mud_sense_measure(None, p(maps), rows, Nc, p(m), rows, p(y), rows, S, None) == 1
    assert lib.mud_sense_measure(p(x), p(maps), rows, 33, p(m), rows, p(y), rows, S, None) == 1 and b'mud_sense_measure' in lib.mud_last_error()
    assert lib.mud_sense_measure(p(x), p(maps), 2, Nc, p(m), rows, p(y), rows, S, None) == 1
    assert lib.mud_sense_adjoint(p(y), p(maps), rows, Nc, None, rows, S, None) == 1 and b'mud_sense_adjoint' in lib.mud_last_error()
    assert lib.mud_sense_adjoint(p(y), p(maps), rows, Nc, p(out), rows, 24, None) == 1
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((res == 7.0).all())                          # nothing was launched
    for kind in (ops.KIND_SENSE, ops.KIND_SENSE_MEAS):
        assert tuple(ops.randn_keyed(torch.tensor([[1, 0]]), 8, 1, 0, kind).shape) == (1, 8)
    assert (ops.KIND_SENSE, ops.KIND_SENSE_MEAS) == (10, 11)
    # the wrappers' own checks
    mk = lambda **kw: ops.sense_constrain(kw.get('x', x), kw.get('ahy', ahy), kw.get('m', m), kw.get('maps', maps), kw.get('lam', 8.0),   # noqa: E731
                                          kw.get('iters', 2), None, 0, None, None, clean=kw.get('clean', True), work=kw.get('work'))
    for kw in (dict(ahy=ahy[:2]), dict(m=m[:2]), dict(maps=maps[:2]), dict(maps=maps.real.contiguous()), dict(lam=-1.0), dict(iters=0), dict(iters=65),
               dict(work=work[:-1]), dict(clean=False), dict(x=x.cpu()), dict(x=torch.zeros(rows, 24, 24, **f))):
        with pytest.raises(MudiffHipError):
            mk(**kw)
    with pytest.raises(MudiffHipError):
        ops.sense_measure(x, maps[:2], m)
    with pytest.raises(MudiffHipError):
        ops.sense_adjoint(y, maps[:, :1])


def test_sample_keyed_takes_the_constraint_and_stays_what_it_was_without():
    """GraphSampler.sample_keyed(constraint=SenseRows): in a child process with MUD_DETERMINISTIC=1 (read at import), as
    tests/test_kspace_gpu.py runs its sampler checks."""
    import os
    import subprocess
    import sys
    from conftest import PKG, REPO
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([REPO, PKG, os.path.join(REPO, 'tests'), os.environ.get('PYTHONPATH', '')]), MUD_DETERMINISTIC='1')
    c = subprocess.run([sys.executable, '-c', 'import test_sense_gpu as T; T.sampler_checks(); print("SAMPLER-OK")'], cwd=REPO, env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert c.returncode == 0 and 'SAMPLER-OK' in c.stdout, c.stdout[-3000:] + c.stderr[-3000:]


def sampler_checks():
    """The body of test_sample_keyed_takes_the_constraint_and_stays_what_it_was_without (run in its child process)."""
    import volume_support as VS
    from oracle import mudiff_oracle as O
    from backbones.ncsnpp_generator_adagn_feat import NCSNpp, NCSNpp_adaptive
    from mudiff_hip import constraints as Cn, ops, sampling as Sm
    assert ops.DETERMINISTIC
    cfg = O.default_config(**VS.TINY_MODEL)
    g1, g2 = NCSNpp(cfg), NCSNpp_adaptive(cfg)
    g1.load_state_dict(O.make_state_dict(cfg, 'g1', 9)); g2.load_state_dict(O.make_state_dict(cfg, 'g2', 9))
    g1, g2 = g1.to(DEV).eval(), g2.to(DEV).eval()
    B, S, Nc, T = 3, 16, 4, int(cfg.num_timesteps)
    lam, iters = 8.0, 32
    sampler = Sm.GraphSampler(Sm.Posterior_Coefficients(cfg, DEV), g1, g2, cfg, B, S, S, DEV)
    g = np.random.default_rng(11)
    conds = [_dev(np.tanh(g.standard_normal((B, 1, S, S))).astype(np.float32)) for _ in range(3)]
    k = np.tanh(g.standard_normal((B, S, S))).astype(np.float32)
    m = (g.random((1, S, S)) < 0.4).astype(np.uint8)
    maps = R.coil_maps(S, Nc).astype(np.complex64)
    ahy = R.adjoint(R.measure(k, maps, m).astype(np.complex64), maps).astype(np.float32)
    rows_of = lambda a, idx=None: Cn.SenseRows(_dev(a if idx is None else a[idx]), _dev(m), _dev(maps), lam, iters)      # noqa: E731
    keys = torch.tensor([[4, 0], [5, 0], [6, 1]])
    before = sampler.sample_keyed(*conds, keys, 31, T)
    out = sampler.sample_keyed(*conds, keys, 31, T, constraint=rows_of(ahy))
    work = sampler._sense_work
    x_new = sampler.sense_x_new.clone()
    again = sampler.sample_keyed(*conds, keys, 31, T, constraint=rows_of(ahy), coupling='shared', resample=2)
    assert sampler._sense_work is work and torch.isfinite(again).all()                  # one workspace
    assert torch.equal(sampler.sample_keyed(*conds, keys, 31, T), before)               # without the constraint: what it was
    assert not torch.equal(out, before)
    # the last step is the clean one: its optimality residual against the torch chain's
    xn = x_new[:, 0].cpu().numpy()
    one, zero = np.ones(B), np.zeros(B)
    chain = _torch_chain(xn, ahy, maps[None], m, lam, iters, None, one, zero)
    opt = R.optimality(out[:, 0].cpu().numpy(), xn, ahy, maps, m, lam, None, one, zero)
    topt = R.optimality(chain, xn, ahy, maps, m, lam, None, one, zero)
    print(f'optimality residual of the last step: {opt} (torch CPU fp32: {topt})')
    assert (opt <= FACTOR * topt).all(), (opt, topt)
    # a row's result does not depend on the rows around it
    alone = sampler.sample_keyed(*[c[[1, 1, 1]] for c in conds], keys[[1, 1, 1]], 31, T, constraint=rows_of(ahy, [1, 1, 1]))
    assert torch.equal(alone[0], out[1])
    with pytest.raises(ValueError, match='mutually exclusive'):
        sampler.sample_keyed(*conds, keys, 31, T, constraint=rows_of(ahy), kspace=(torch.zeros(B, S, S, device=DEV, dtype=torch.complex64), _dev(m)))
    with pytest.raises(ValueError, match='sense'):
        sampler.sample_keyed(*conds, keys, 31, T, constraint=rows_of(ahy[:2]))
    odd = Sm.GraphSampler.__new__(Sm.GraphSampler)                                       # the size check needs no captured graph
    odd.B, odd.H, odd.W = B, 24, 24
    with pytest.raises(ValueError, match='power of two'):
        Sm.GraphSampler.sample_keyed(odd, *conds, keys, 31, T, constraint=rows_of(ahy))
