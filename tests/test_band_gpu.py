"""GPU: the banded data-consistency step of a thick volume with a geometry of its own (csrc/band.hip: mud_band_constrain,
mud_band_measure; ops.band_tables, ops.band_constrain, ops.band_measure) against the restatements in tests/band_ref.py.  DESIGN.md
section 5.29.

The accuracy rules count the roundings of the kernel's chain (band_ref.bound_out, bound_residual, bound_measure); the fp32 emulation of
the chain stays below 0.6 of each (tests/test_thick_volume_host.py).  Shapes: row_len 4 (one quad), 33 (element by element, a cut quad),
256, 1028 (more than one workgroup of 256 quads, not a multiple of it); the four geometries of the host test (bandwidth 1, 2, 3, 2;
box and gauss; fractional origins; thin slices under no thick slice in the first two) and one thick slice over a stack of 3
(bandwidth 0); 1 and 3 sets."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import band_ref as R
import thick_ref

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ROW_LENS = (4, 33, 256, 1028)
GEOMETRIES = ((12, 1.25, 2.5, 3.0, 'box'), (24, 3.25, 2.5, 3.0, 'gauss'), (24, 1.7, 1.0, 3.0, 'box'), (24, 1.0, 1.5, 3.0, 'box'),
              (3, 1.0, 3.0, 3.0, 'box'))
SETS = (1, 3)
NTAB = 5
SEED = 0x1234567890ABCDEF


def _levels():
    a = np.array([0.99999994, 0.97, 0.81, 0.5, 0.12], np.float32)
    return a, np.sqrt(1 - a.astype(np.float64) ** 2).astype(np.float32)


def _dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).to(DEV)      # (a copy: the shared cases are read-only)


def _bits(t):
    return t.view(torch.int32)


@functools.lru_cache(maxsize=None)
def _matrix(geom):
    A, _, _ = R.weights(*geom)
    A.setflags(write=False)
    return A


@functools.lru_cache(maxsize=None)
def _case(row_len, gi, sets):
    """x, eta [sets, n, row_len], y [m, row_len] = A k, t [sets * n] (the set's level sits in its row 0; the other rows name another
    one, which must not count), keys [sets * n, 2].  A -0 is planted in a covered row and, where the geometry has one, in a free row.
    Computed once, shared, never written."""
    geom = GEOMETRIES[gi]
    A = _matrix(geom)
    m, n = A.shape
    g = np.random.default_rng(100000 * gi + 10 * row_len + sets)
    x = g.standard_normal((sets, n, row_len)).astype(np.float32)
    eta = g.standard_normal((sets, n, row_len)).astype(np.float32)
    k = np.tanh(g.standard_normal((n, row_len))).astype(np.float32)
    y = R.measure(k, A).astype(np.float32)
    free = np.flatnonzero((R.as_kernel(A) != 0).sum(0) == 0).tolist()
    x[:, 0, -1] = -0.0
    for i in free:
        x[:, i, 0] = -0.0
    t = np.zeros((sets, n), np.int64)
    for s in range(sets):
        t[s, 0] = (s + 1) % NTAB
        t[s, 1:] = (s + 3) % NTAB
    keys = np.stack([np.tile(np.arange(n), sets) + 40, np.repeat(np.arange(sets), n)], 1).astype(np.int64)
    for a in (x, eta, y, t, keys):
        a.setflags(write=False)
    return dict(A=A, m=m, n=n, x=x, eta=eta, y=y, t=t.reshape(-1), keys=keys, free=free)


@functools.lru_cache(maxsize=None)
def _tables(gi):
    from mudiff_hip import ops
    return ops.band_tables(_matrix(GEOMETRIES[gi]))


def _level(c, s):
    a_tab, s_tab = _levels()
    lv = int(np.clip(c['t'][s * c['n']], 0, NTAB - 1))
    return float(a_tab[lv]), float(s_tab[lv])


ALL = [(r, g, s) for r in ROW_LENS for g in range(len(GEOMETRIES)) for s in SETS]


@pytest.mark.parametrize('row_len,gi,sets', ALL)
def test_constrain_with_injected_noise_against_the_restatement(row_len, gi, sets):
    from mudiff_hip import ops
    c, tab = _case(row_len, gi, sets), _tables(gi)
    a_tab, s_tab = _levels()
    x = _dev(c['x'])
    for clean in (False, True):
        got = ops.band_constrain(x, _dev(c['y']), tab, _dev(c['t']), 0, _dev(a_tab), _dev(s_tab), noise=_dev(c['eta']), clean=clean)
        worst, worst_res, exact = 0.0, 0.0, True
        for s in range(sets):
            a, sg = _level(c, s)
            args = (c['x'][s], c['y'], c['A'], c['eta'][s], a, sg, clean)
            want, bound = R.constrain(*args), R.bound_out(*args)
            g = got[s].cpu().numpy()
            err = np.abs(g.astype(np.float64) - want)
            used = np.isfinite(bound)
            worst = max(worst, float(np.max(err[used] / bound[used])))
            assert (err[used] <= bound[used]).all()
            exact = exact and np.array_equal(g.view(np.int32), R.constrain_fp32(c['x'][s], c['y'], tab, c['eta'][s], a, sg, clean).view(np.int32))
            if clean:
                res = np.abs(R.measure(g, c['A']) - c['y'].astype(np.float64))
                rb = R.bound_residual(c['x'][s], c['y'], c['A'])
                worst_res = max(worst_res, float(np.max(res / rb)))
                assert (res <= rb).all()
        print(f'row_len {row_len} geometry {gi} sets {sets} clean {clean}: worst |out - ref| / bound {worst:.3f}' +
              (f', worst clean residual / bound {worst_res:.3f}' if clean else ''))
        assert exact, 'the kernel and the fp32 emulation of its chain differ in some bit'
        if c['free']:
            assert torch.equal(_bits(got[:, c['free']]), _bits(x[:, c['free']]))         # free rows: x's bits, the -0 included
            assert np.signbit(got[0, c['free'][0], 0].item()) and got[0, c['free'][0], 0].item() == 0.0
    assert torch.equal(_bits(x), _bits(_dev(c['x'])))                                    # the operand is not written


@pytest.mark.parametrize('row_len,gi,sets', ALL)
def test_keyed_draw_in_place_and_independence_of_the_sets(row_len, gi, sets):
    from mudiff_hip import ops
    c, tab = _case(row_len, gi, sets), _tables(gi)
    a_tab, s_tab = (_dev(v) for v in _levels())
    x, y, t, keys = _dev(c['x']), _dev(c['y']), _dev(c['t']), _dev(c['keys'])
    step, n = 7, c['n']
    kw = dict(keys=keys, seed=SEED, step=step)
    keyed = ops.band_constrain(x, y, tab, t, 0, a_tab, s_tab, **kw)
    eta = ops.randn_keyed(keys, row_len, SEED, step, ops.KIND_BAND).view(sets, n, row_len)
    injected = ops.band_constrain(x, y, tab, t, 0, a_tab, s_tab, noise=eta)
    assert torch.equal(_bits(keyed), _bits(injected))                                    # the kernel draws what randn_keyed gives kind 8
    assert not torch.equal(keyed, ops.band_constrain(x, y, tab, t, 0, a_tab, s_tab, **dict(kw, step=8)))
    inplace = x.clone()
    assert ops.band_constrain(inplace, y, tab, t, 0, a_tab, s_tab, out=inplace, **kw) is inplace
    assert torch.equal(_bits(inplace), _bits(keyed))
    for clean in (False, True):
        whole = ops.band_constrain(x, y, tab, t, 0, a_tab, s_tab, clean=clean, **kw)
        for s in range(sets if sets > 1 else 0):                                         # a set alone: the bits it gets among three
            alone = ops.band_constrain(x[s:s + 1], y, tab, t[s * n:(s + 1) * n], 0, a_tab, s_tab, keys=keys[s * n:(s + 1) * n], seed=SEED,
                                       step=step, clean=clean)
            assert torch.equal(_bits(alone[0]), _bits(whole[s]))


@pytest.mark.parametrize('row_len,gi,sets', ALL)
def test_measure_against_the_restatement(row_len, gi, sets):
    from mudiff_hip import ops
    c, tab = _case(row_len, gi, sets), _tables(gi)
    got = ops.band_measure(_dev(c['x']), tab)
    assert tuple(got.shape) == (sets, c['m'], row_len)
    worst = 0.0
    for s in range(sets):
        err = np.abs(got[s].cpu().numpy().astype(np.float64) - R.measure(c['x'][s], c['A']))
        bound = R.bound_measure(c['x'][s], c['A'])
        worst = max(worst, float(np.max(err / np.maximum(bound, 1e-300))))
        assert (err <= bound).all()
    print(f'row_len {row_len} geometry {gi} sets {sets}: worst |A x - ref| / bound {worst:.3f}')


@pytest.mark.parametrize('row_len', ROW_LENS)
@pytest.mark.parametrize('profile', ('box', 'gauss'))
def test_integer_contiguous_layout_against_the_diagonal_kernel(row_len, profile):
    """Slabs of L = 4 thin slices from slice 1 of 13: A A^T is diagonal, and mud_slab_constrain projects the same way."""
    from mudiff_hip import ops
    n, L, off = 13, 4, 1
    A = np.zeros((3, n))
    for j in range(3):
        A[j, off + j * L:off + (j + 1) * L] = thick_ref.profile(L, profile)
    assert R.bandwidth(A) == 0
    g = np.random.default_rng(row_len)
    x = g.standard_normal((n, row_len)).astype(np.float32)
    eta = g.standard_normal((n, row_len)).astype(np.float32)
    y = R.measure(np.tanh(g.standard_normal((n, row_len))).astype(np.float32), A).astype(np.float32)
    a_tab, s_tab = _levels()
    t = np.full(n, 2, np.int64)
    members = np.array([[off + j * L + l for l in range(L)] for j in range(3)], np.int32)
    w = np.stack([A[j, members[j]] for j in range(3)]).astype(np.float32)
    gains = np.stack([thick_ref.gains(r) for r in w])
    for clean in (False, True):
        band = ops.band_constrain(_dev(x)[None], _dev(y), ops.band_tables(A), _dev(t), 0, _dev(a_tab), _dev(s_tab), noise=_dev(eta)[None], clean=clean)[0]
        slab = ops.slab_constrain(_dev(x), _dev(y), members, w, _dev(t), 0, _dev(a_tab), _dev(s_tab), gains=gains, noise=_dev(eta), clean=clean)
        b1 = R.bound_out(x, y, A, eta, float(a_tab[2]), float(s_tab[2]), clean)
        b2 = thick_ref.bound_out(x, y, members, w, gains, eta, t, 0, a_tab, s_tab, clean)
        err = np.abs(band.cpu().numpy().astype(np.float64) - slab.cpu().numpy().astype(np.float64))
        used = np.isfinite(b1)
        print(f'row_len {row_len} {profile} clean {clean}: worst |band - slab| / bound {np.max(err[used] / (b1 + b2)[used]):.3f}')
        assert (err[used] <= (b1 + b2)[used]).all()
        assert torch.equal(_bits(band[0]), _bits(slab[0]))                               # the free first slice


def test_entries_refuse_bad_arguments_before_any_launch():
    import mudiff_hip
    from mudiff_hip import ops
    lib = mudiff_hip.load()
    tab = _tables(0)
    st = tab.on(torch.device(DEV))
    n, m, row_len = tab.n, tab.m, 8
    x = torch.zeros(1, n, row_len, device=DEV)
    y = torch.zeros(m, row_len, device=DEV)
    work = torch.zeros(m, row_len, device=DEV)
    p = lambda v: None if v is None else C.c_void_p(v.data_ptr())      # noqa: E731

    def constrain(tab_=st, x_=x, y_=y, out_=x, work_=work, sets=1, n_=row_len, kind=8, step=0, clean=1):
        return lib.mud_band_constrain(p(x_), p(y_), C.byref(tab_), None, None, C.c_uint64(0), step, kind, None, 0, None, None, 1, clean, p(out_),
                                      p(work_), sets, n_, None)

    assert constrain() == 0
    bad = lambda **kw: type(st)(**{**{f: getattr(st, f) for f, _ in st._fields_}, **kw})      # noqa: E731
    for kw in (dict(tab_=bad(m=0)), dict(tab_=bad(m=257)), dict(tab_=bad(n=513)), dict(tab_=bad(bw=9)), dict(tab_=bad(bw=m)),
               dict(tab_=bad(nnz=m - 1)), dict(tab_=bad(nnz=m * 32 + 1)), dict(tab_=bad(lc=None)), dict(sets=0), dict(sets=65536), dict(n_=0),
               dict(n_=1 << 28), dict(kind=16), dict(step=1 << 24), dict(x_=None), dict(work_=None), dict(work_=x), dict(work_=y),
               dict(clean=0)):
        assert constrain(**kw) == 1 and b'mud_band_constrain' in lib.mud_last_error(), kw
    ax = torch.zeros(1, m, row_len, device=DEV)
    assert lib.mud_band_measure(p(x), C.byref(st), p(ax), 1, row_len, None) == 0
    for args in ((None, st, ax, 1, row_len), (x, bad(n=0), ax, 1, row_len), (x, st, x, 1, row_len), (x, st, ax, 0, row_len)):
        assert lib.mud_band_measure(p(args[0]), C.byref(args[1]), p(args[2]), args[3], args[4], None) == 1
        assert b'mud_band_measure' in lib.mud_last_error(), args
    with pytest.raises(mudiff_hip.MudiffHipError, match='band_constrain'):
        ops.band_constrain(x[0], y, tab, None, 0, None, None, clean=True)                # not [sets, n, ...]
    torch.cuda.synchronize()
