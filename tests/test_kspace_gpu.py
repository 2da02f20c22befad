"""GPU: the batched 2D FFT and the k-space data-consistency step (csrc/kspace.hip: mud_fft2_c2c, mud_fft2_r2c, mud_kspace_constrain;
ops.fft2, ops.kspace_constrain) against the fp64 restatement in tests/kspace_ref.py.  DESIGN.md section 5.26.

The accuracy rule of a transform: relative L2 error <= 8 * log2(S^2) * 2^-24 (kspace_ref.rule: the worst case of a radix FFT with
correctly rounded twiddles) and <= 4 x the error torch's own fp32 FFT makes on the CPU on the same input, computed here."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import kspace_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SIZES = (16, 32, 256, 512)         # the smallest, an odd log2, production, the largest (an odd log2 again)
ROWS = (1, 3, 5)
NTAB = 5
FACTOR = 4.0


def _tables():
    a = np.array([0.99999994, 0.97, 0.81, 0.5, 0.12], np.float32)
    return a, np.sqrt(1 - a.astype(np.float64) ** 2).astype(np.float32)


def _dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).to(DEV)      # (a copy: the shared cases are read-only)


def _cpu(a):
    return torch.from_numpy(np.array(a))                                                 # (a copy: the shared cases are read-only)


def _err(got, want):
    """Per-slice L2 error and norm of the reference: two fp64 [rows] arrays."""
    d = np.asarray(got).astype(np.complex128) - want
    return np.sqrt((np.abs(d) ** 2).sum((1, 2))), np.sqrt((np.abs(want) ** 2).sum((1, 2)))


@functools.lru_cache(maxsize=None)
def _fft_case(S, rows):
    """A complex input, its fp64 transforms and the error of torch's fp32 CPU FFT on it: computed once, shared, never written."""
    g = np.random.default_rng(100 * S + rows)
    x = (g.standard_normal((rows, S, S)) + 1j * g.standard_normal((rows, S, S))).astype(np.complex64)
    fwd, inv = R.fft2(x), R.fft2(x, inverse=True)
    tx = torch.from_numpy(x)
    t_fwd, t_inv = torch.fft.fft2(tx, norm='ortho'), torch.fft.ifft2(tx, norm='ortho')
    t_trip = torch.fft.ifft2(t_fwd, norm='ortho')
    torch_err = dict(fwd=_err(t_fwd.numpy(), fwd)[0], inv=_err(t_inv.numpy(), inv)[0], trip=_err(t_trip.numpy(), x.astype(np.complex128))[0])
    for a in (x, fwd, inv):
        a.setflags(write=False)
    return x, fwd, inv, torch_err


def _check_rule(name, S, got, want, torch_err):
    err, norm = _err(got, want)
    print(f'{name} S={S}: rel L2 error {np.max(err / norm):.3e} (rule {R.rule(S):.3e}; torch CPU fp32 {np.max(torch_err / norm):.3e})')
    assert (err <= R.rule(S) * norm).all(), (name, S, err / norm)
    assert (err <= FACTOR * torch_err).all(), (name, S, err / torch_err)


@pytest.mark.parametrize('rows', ROWS)
@pytest.mark.parametrize('S', SIZES)
def test_fft2_against_numpy_fp64(S, rows):
    from mudiff_hip import ops
    x, fwd, inv, terr = _fft_case(S, rows)
    xd = _dev(x)
    F = ops.fft2(xd)
    assert F.dtype == torch.complex64 and tuple(F.shape) == (rows, S, S)
    _check_rule('forward', S, F.cpu().numpy(), fwd, terr['fwd'])
    _check_rule('inverse', S, ops.fft2(xd, inverse=True).cpu().numpy(), inv, terr['inv'])
    _check_rule('round trip', S, ops.fft2(F, inverse=True).cpu().numpy(), x.astype(np.complex128), terr['trip'])
    assert torch.equal(xd.cpu(), _cpu(x))                                   # the input is left alone


@pytest.mark.parametrize('rows', ROWS)
@pytest.mark.parametrize('S', SIZES)
def test_fft2_forms_agree_bit_for_bit(S, rows):
    from mudiff_hip import ops
    x = _fft_case(S, rows)[0]
    xd = _dev(x)
    bits = lambda t: torch.view_as_real(t).contiguous().view(torch.int32)               # noqa: E731
    for inverse in (False, True):
        want = ops.fft2(xd, inverse=inverse)
        inplace = xd.clone()
        assert ops.fft2(inplace, inverse=inverse, out=inplace) is inplace
        assert torch.equal(bits(inplace), bits(want))
        out = torch.empty_like(xd)
        assert ops.fft2(xd, inverse=inverse, out=out) is out and torch.equal(bits(out), bits(want))
        re = xd.real.contiguous()
        assert torch.equal(bits(ops.fft2(re, inverse=inverse)), bits(ops.fft2(torch.complex(re, torch.zeros_like(re)), inverse=inverse)))
        if rows == 5:                                                                     # a slice alone and inside a batch of 5
            for r in (0, 4):
                assert torch.equal(bits(ops.fft2(xd[r:r + 1].contiguous(), inverse=inverse)), bits(want[r:r + 1]))


# ---------------------------------------------------------------------------------------------------
# the constraint
# ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _con_case(S, rows):
    g = np.random.default_rng(7000 + 10 * S + rows)
    x = g.standard_normal((rows, S, S)).astype(np.float32)
    k = np.tanh(g.standard_normal((rows, S, S))).astype(np.float32)
    eta = g.standard_normal((rows, S, S)).astype(np.float32)
    masks = {mr: R.symmetrise((g.random((mr, S, S)) < 0.3).astype(np.uint8)) for mr in {1, rows}}
    t = g.integers(-2, NTAB + 2, rows).astype(np.int64)                                  # per-row levels, the clamped ends included
    t[0] = -1
    if rows >= 2:
        t[-1] = NTAB + 1
    ys = {mr: R.measure(k, m).astype(np.complex64) for mr, m in masks.items()}           # the fp32 measurements every side is given
    for a in (x, k, eta, t) + tuple(masks.values()) + tuple(ys.values()):
        a.setflags(write=False)
    return x, k, eta, t, masks, ys


def _torch_chain(x, y, m, eta, t, toff, a_tab, s_tab, clean):
    """The same chain in torch on the CPU: fp32 / complex64."""
    x, y, m = _cpu(x), _cpu(y), _cpu(m) != 0
    if clean:
        d, a = x, torch.ones(x.shape[0])
    else:
        c = np.clip(t + toff, 0, len(a_tab) - 1)
        a, s = torch.from_numpy(a_tab[c]), torch.from_numpy(s_tab[c])
        d = x - s[:, None, None] * _cpu(eta)
    r = torch.where(m, torch.fft.fft2(d, norm='ortho') - a[:, None, None] * y, torch.zeros((), dtype=torch.complex64))
    return (x - torch.fft.ifft2(r, norm='ortho').real).numpy()


@pytest.mark.parametrize('rows', ROWS)
@pytest.mark.parametrize('S', SIZES)
def test_constrain_with_injected_noise_against_the_restatement(S, rows):
    from mudiff_hip import ops
    a_tab, s_tab = _tables()
    x, k, eta, t, masks, ys = _con_case(S, rows)
    at, st = _dev(a_tab), _dev(s_tab)
    l2 = lambda a: np.sqrt((np.abs(np.asarray(a, np.complex128)) ** 2).sum((1, 2)))      # noqa: E731
    worst = 0.0
    for mr in sorted(masks):
        m, y = masks[mr], ys[mr]
        for toff in (0, 1):
            for clean in (False, True):
                want = R.constrain(x, y, m, eta, t, toff, a_tab, s_tab, clean)
                got = ops.kspace_constrain(_dev(x), _dev(y), _dev(m), _dev(t), toff, at, st, noise=_dev(eta), clean=clean).cpu().numpy()
                ref = _torch_chain(x, y, m, eta, t, toff, a_tab, s_tab, clean)
                err, terr = l2(got - want), l2(ref - want)
                c = np.clip(t + toff, 0, NTAB - 1)
                a, s = (np.ones(rows), np.zeros(rows)) if clean else (a_tab[c].astype(np.float64), s_tab[c].astype(np.float64))
                bound = 3 * R.rule(S) * (l2(x) + s * l2(eta) + a * l2(y))
                worst = max(worst, float(np.max(err / np.maximum(terr, 1e-300))))
                assert (err <= bound).all(), (mr, toff, clean, err / bound)
                assert (err <= FACTOR * terr).all(), (mr, toff, clean, err / terr)
    print(f'constrain S={S} rows={rows}: worst error / torch CPU complex64 error {worst:.3f}')


@pytest.mark.parametrize('rows', ROWS)
@pytest.mark.parametrize('S', SIZES)
def test_constrain_keyed_draw_zero_mask_full_mask_and_in_place(S, rows):
    from mudiff_hip import ops
    a_tab, s_tab = _tables()
    x, k, eta, t, masks, ys = _con_case(S, rows)
    at, st, xd, td = _dev(a_tab), _dev(s_tab), _dev(x), _dev(t)
    m, y = _dev(masks[rows]), _dev(ys[rows])
    bits = lambda v: v.contiguous().view(torch.int32)                                    # noqa: E731
    # the keyed draw is the injected ops.randn_keyed row, bit for bit
    g = np.random.default_rng(rows)
    keys = np.stack([g.integers(0, 200, rows), g.integers(0, 16, rows)], 1).astype(np.int64)
    seed, step = 2024, 3
    draw = ops.randn_keyed(torch.from_numpy(keys), S * S, seed, step, ops.KIND_KSPACE).to(DEV).view(rows, S, S)
    want = ops.kspace_constrain(xd, y, m, td, 0, at, st, noise=draw)
    got = ops.kspace_constrain(xd, y, m, td, 0, at, st, keys=keys, seed=seed, step=step)
    assert torch.equal(bits(got), bits(want))
    assert not torch.equal(bits(got), bits(ops.kspace_constrain(xd, y, m, td, 0, at, st, keys=keys, seed=seed, step=step + 1)))
    # out is x_new: the same bits as out of place, with and without a draw
    for clean in (False, True):
        want = ops.kspace_constrain(xd, y, m, td, 0, at, st, noise=_dev(eta), clean=clean)
        inplace = xd.clone()
        assert ops.kspace_constrain(inplace, y, m, td, 0, at, st, noise=_dev(eta), clean=clean, out=inplace) is inplace
        assert torch.equal(bits(inplace), bits(want))
    # [rows, 1, S, S] as the sampler holds it
    assert torch.equal(bits(ops.kspace_constrain(xd[:, None], y, m, td, 0, at, st, noise=_dev(eta)[:, None])[:, 0]),
                       bits(ops.kspace_constrain(xd, y, m, td, 0, at, st, noise=_dev(eta))))
    # a mask of zeros: the bits of x_new, a negative zero included
    xz = xd.clone()
    xz[0, 0, :4] = torch.tensor([-0.0, 0.0, -1.5, 2.5], device=DEV)
    for mr in (1, rows):
        zero = torch.zeros(mr, S, S, device=DEV, dtype=torch.uint8)
        for clean in (False, True):
            assert torch.equal(bits(ops.kspace_constrain(xz, y, zero, td, 0, at, st, noise=_dev(eta), clean=clean)), bits(xz))
    # a mask of ones and clean: k, within the rule
    ones = np.ones((1, S, S), np.uint8)
    yk = R.measure(k, ones)
    got = ops.kspace_constrain(xd, _dev(yk.astype(np.complex64)), _dev(ones), None, 0, None, None, clean=True).cpu().numpy()
    err = np.sqrt(((got - k.astype(np.float64)) ** 2).sum((1, 2)))
    scale = np.sqrt((x.astype(np.float64) ** 2).sum((1, 2))) + np.sqrt((k.astype(np.float64) ** 2).sum((1, 2)))
    assert (err <= 3 * R.rule(S) * scale).all(), err / scale


@pytest.mark.parametrize('S', SIZES)
def test_clean_step_with_a_hermitian_mask_meets_the_measurements(S):
    """The measured coefficients of the clean result are y, the others those of x_new, both within the rule."""
    from mudiff_hip import ops
    rows = 3
    x, k, eta, t, masks, ys = _con_case(S, rows)
    m, y = masks[1], ys[1]
    assert np.array_equal(R.symmetrise(m), m)
    got = ops.kspace_constrain(_dev(x), _dev(y), _dev(m), None, 0, None, None, clean=True).cpu().numpy()
    F, Fx = R.fft2(got), R.fft2(x)
    scale = np.sqrt((x.astype(np.float64) ** 2).sum((1, 2))) + np.sqrt((np.abs(y.astype(np.complex128)) ** 2).sum((1, 2)))
    on = np.sqrt((np.abs(np.where(m != 0, F - y, 0)) ** 2).sum((1, 2)))
    off = np.sqrt((np.abs(np.where(m == 0, F - Fx, 0)) ** 2).sum((1, 2)))
    print(f'S={S}: measured |F(out) - y| / scale {np.max(on / scale):.3e}, unmeasured |F(out) - F(x)| / scale {np.max(off / scale):.3e} '
          f'(rule x 3: {3 * R.rule(S):.3e})')
    assert (on <= 3 * R.rule(S) * scale).all() and (off <= 3 * R.rule(S) * scale).all()
    assert 0 < int(m.sum()) < m.size


def parent_bit_cases():
    """(name, output) of ops.kspace_constrain and ops.fft2 at S = 16 and 512 (the two ends; 512 runs 8 lines per workgroup), rows 1 and
    3: a mask shared by the rows and one per row, of zeros and of ones; noise injected at toff -1 / 0 / +1 against levels at both ends
    of the table, the keyed draw out of place and in place, `clean`; fft2 of a real and a complex input, forward and inverse."""
    import parent_bits as P
    from mudiff_hip import ops
    at, st = (_dev(v) for v in _tables())
    for S in (16, 512):
        for rows in (1, 3):
            x, _, eta, t, masks, ys = _con_case(S, rows)
            x, eta, t = _dev(x), _dev(eta), _dev(t)
            keys = torch.stack([torch.arange(rows) + 11, torch.arange(rows) % 2], 1)
            for mr in sorted(masks):
                m, y = _dev(masks[mr]), _dev(ys[mr])
                tag = f'S{S} rows {rows} mask {mr}'
                for toff in (-1, 0, 1):
                    yield f'{tag} noise toff {toff}', ops.kspace_constrain(x, y, m, P.level_t(rows, toff).to(DEV), toff, at, st, noise=eta)
                yield f'{tag} keyed', ops.kspace_constrain(x, y, m, t, 0, at, st, keys=keys, seed=2024, step=3)
                xd = x.clone()
                yield f'{tag} keyed in place', ops.kspace_constrain(xd, y, m, t, 0, at, st, keys=keys, seed=2024, step=3, out=xd)
                yield f'{tag} clean', ops.kspace_constrain(x, y, m, None, 0, None, None, clean=True)
            y = _dev(ys[rows])
            for name, fill in (('zeros', 0), ('ones', 1)):
                m = torch.full((1, S, S), fill, device=DEV, dtype=torch.uint8)
                yield f'S{S} rows {rows} mask of {name} noise', ops.kspace_constrain(x, y, m, t, 0, at, st, noise=eta)
                yield f'S{S} rows {rows} mask of {name} clean', ops.kspace_constrain(x, y, m, None, 0, None, None, clean=True)
            z = _dev(_fft_case(S, rows)[0])
            for inverse in (False, True):
                yield f'S{S} rows {rows} fft2 complex inverse {inverse}', ops.fft2(z, inverse=inverse)
                yield f'S{S} rows {rows} fft2 real inverse {inverse}', ops.fft2(x, inverse=inverse)


def test_the_bits_are_those_of_the_parent_commit():
    import parent_bits as P
    P.check('test_kspace_gpu', parent_bit_cases())


def test_bad_arguments_are_refused_before_a_launch():
    import mudiff_hip
    from mudiff_hip import MudiffHipError, ops
    lib = mudiff_hip.load()
    rows, S = 3, 16
    f = dict(device=DEV, dtype=torch.float32)
    x, out, work = torch.randn(rows, S, S, **f), torch.full((rows, S, S), 7.0, **f), torch.zeros(rows, S, S, device=DEV, dtype=torch.complex64)
    y, m = torch.zeros(rows, S, S, device=DEV, dtype=torch.complex64), torch.ones(rows, S, S, device=DEV, dtype=torch.uint8)
    p = lambda v: None if v is None else C.c_void_p(v.data_ptr())                        # noqa: E731

    def call(S_=S, mask_rows=rows, work_=work, kind=5, step=0, x_=x):
        return lib.mud_kspace_constrain(p(x_), p(y), p(m), mask_rows, None, None, 0, step, kind, None, 0, None, None, 1, 1, p(out), p(work_), rows, S_, None)

    assert call() == 0
    torch.cuda.synchronize()
    out.fill_(7.0)
    for kw in (dict(S_=24), dict(S_=1024), dict(S_=8), dict(mask_rows=2), dict(work_=None), dict(kind=16), dict(kind=-1), dict(step=-1),
               dict(step=1 << 24), dict(x_=None), dict(work_=out)):
        assert call(**kw) == 1 and b'mud_kspace_constrain' in lib.mud_last_error(), kw
    for S_ in (24, 1024):
        assert lib.mud_fft2_c2c(p(y), p(y), rows, S_, 0, None) == 1 and b'mud_fft2_c2c' in lib.mud_last_error()
    assert lib.mud_fft2_c2c(None, p(y), rows, S, 0, None) == 1 and lib.mud_fft2_r2c(p(x), None, rows, S, 0, None) == 1
    assert lib.mud_fft2_c2c(p(y), p(y), 0, S, 0, None) == 1
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())                                                       # nothing was launched
    # the wrappers' own checks
    with pytest.raises(MudiffHipError):
        ops.fft2(torch.zeros(2, 24, 24, device=DEV))
    with pytest.raises(MudiffHipError):
        ops.fft2(torch.zeros(2, 16, 32, device=DEV))
    with pytest.raises(MudiffHipError):
        ops.fft2(torch.zeros(2, 16, 16, device=DEV, dtype=torch.float64))
    with pytest.raises(MudiffHipError):
        ops.kspace_constrain(x, y, m[:2], None, 0, None, None, clean=True)
    with pytest.raises(MudiffHipError):
        ops.kspace_constrain(x, y.real.contiguous(), m, None, 0, None, None, clean=True)
    with pytest.raises(MudiffHipError):
        ops.kspace_constrain(x, y, m, None, 0, None, None)                                # no t, no tables
    with pytest.raises(MudiffHipError):
        ops.kspace_constrain(x.cpu(), y, m, None, 0, None, None, clean=True)


def test_sample_keyed_takes_kspace_and_stays_what_it_was_without():
    """GraphSampler.sample_keyed(kspace=): exclusive with known, refused on a grid the transform does not take, one workspace per sampler;
    the measured coefficients of the result are y; without kspace the result is bit for bit the one of a sampler that never saw it.
    In a child process with MUD_DETERMINISTIC=1 (read at import): every GroupNorm then reduces in a fixed order, so bits can be compared."""
    import os
    import subprocess
    import sys
    from conftest import PKG, REPO
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([REPO, PKG, os.path.join(REPO, 'tests'), os.environ.get('PYTHONPATH', '')]), MUD_DETERMINISTIC='1')
    c = subprocess.run([sys.executable, '-c', 'import test_kspace_gpu as T; T.sampler_checks(); print("SAMPLER-OK")'], cwd=REPO, env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert c.returncode == 0 and 'SAMPLER-OK' in c.stdout, c.stdout[-3000:] + c.stderr[-3000:]


def sampler_checks():
    """The body of test_sample_keyed_takes_kspace_and_stays_what_it_was_without (run in its child process)."""
    import volume_support as VS
    from oracle import mudiff_oracle as O
    from backbones.ncsnpp_generator_adagn_feat import NCSNpp, NCSNpp_adaptive
    from mudiff_hip import ops, sampling as Sm
    assert ops.DETERMINISTIC
    cfg = O.default_config(**VS.TINY_MODEL)
    g1, g2 = NCSNpp(cfg), NCSNpp_adaptive(cfg)
    g1.load_state_dict(O.make_state_dict(cfg, 'g1', 9)); g2.load_state_dict(O.make_state_dict(cfg, 'g2', 9))
    g1, g2 = g1.to(DEV).eval(), g2.to(DEV).eval()
    B, S, T = 3, 16, int(cfg.num_timesteps)
    sampler = Sm.GraphSampler(Sm.Posterior_Coefficients(cfg, DEV), g1, g2, cfg, B, S, S, DEV)
    g = np.random.default_rng(11)
    conds = [_dev(np.tanh(g.standard_normal((B, 1, S, S))).astype(np.float32)) for _ in range(3)]
    k = np.tanh(g.standard_normal((B, S, S))).astype(np.float32)
    m = R.symmetrise((g.random((1, S, S)) < 0.4).astype(np.uint8))
    y = R.measure(k, m).astype(np.complex64)
    keys = torch.tensor([[4, 0], [5, 0], [6, 1]])
    before = sampler.sample_keyed(*conds, keys, 31, T)
    out = sampler.sample_keyed(*conds, keys, 31, T, kspace=(_dev(y), _dev(m)))
    work = sampler._ks_work
    again = sampler.sample_keyed(*conds, keys, 31, T, kspace=(_dev(y), _dev(m)), coupling='shared', resample=2)
    assert sampler._ks_work is work and torch.isfinite(again).all()
    assert torch.equal(sampler.sample_keyed(*conds, keys, 31, T), before)               # without kspace: what it was
    assert not torch.equal(out, before)
    F = R.fft2(out[:, 0].cpu().numpy())
    scale = np.sqrt((out[:, 0].cpu().numpy().astype(np.float64) ** 2).sum((1, 2))) + np.sqrt((np.abs(y) ** 2).sum((1, 2)))
    for res in (out, again):
        F = R.fft2(res[:, 0].cpu().numpy())
        on = np.sqrt((np.abs(np.where(m != 0, F - y, 0)) ** 2).sum((1, 2)))
        assert (on <= 3 * R.rule(S) * scale).all(), on / scale
    # a row's result does not depend on the rows around it
    alone = sampler.sample_keyed(*[c[[1, 1, 1]] for c in conds], keys[[1, 1, 1]], 31, T, kspace=(_dev(y[[1, 1, 1]]), _dev(m)))
    assert torch.equal(alone[0], out[1])
    with pytest.raises(ValueError, match='mutually exclusive'):
        sampler.sample_keyed(*conds, keys, 31, T, kspace=(_dev(y), _dev(m)), known=torch.zeros(B, 1, S, S, device=DEV),
                             known_mask=torch.zeros(B, 1, S, S, device=DEV, dtype=torch.uint8))
    with pytest.raises(ValueError, match='kspace'):
        sampler.sample_keyed(*conds, keys, 31, T, kspace=(_dev(y)[:2], _dev(m)))
    odd = Sm.GraphSampler.__new__(Sm.GraphSampler)                                       # the size check needs no captured graph
    odd.B, odd.H, odd.W = B, 24, 24
    with pytest.raises(ValueError, match='power of two'):
        Sm.GraphSampler.sample_keyed(odd, *conds, keys, 31, T, kspace=(_dev(y), _dev(m)))
