"""GPU: the data-consistency step of a target measured on a grid coarser in all three axes (csrc/lowres.hip: mud_lowres_constrain,
mud_lowres_measure, mud_lowres_ws_floats; ops.lowres_tables, ops.lowres_constrain, ops.lowres_measure) against the restatements in
tests/lowres_ref.py.  DESIGN.md section 5.31.

The accuracy rule: |kernel - (a)| <= 4 * max(err_c, eps32 * max|x|) per case, with (a) the fp64 dense projection and err_c the max-abs
error of (c), the fp32 emulation of the four passes, against (a) on the same inputs; the 4 covers a different but fixed summation order
inside a pass.  Shapes are non-square so that a swapped axis cannot pass: n x H x W = 7 x 12 x 8 (whole quads) and 5 x 10 x 6 (ragged
quads, eta blocks that straddle image rows), the first again with x one float off 16-byte alignment; 1 and 2 sets.  Coarse lattices:
ratio 2 aligned (all three G diagonal), ratio 2.5 at offset 0.3 (bandwidth >= 1), extent 1.5 x spacing (overlap), gauss, A_y = A_x = I,
A_z = I.
Measured on an MI355X over all 144 (case, mode, set) runs: largest err_c 4.66e-7, largest |kernel - (a)| 4.66e-7; the kernel and (c)
agree to the bit in every one of them, the keyed ones included (asserted for clean and injected noise; a keyed run would differ where the
device's and numpy's cos / sin differ in the last place of eta)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import band_ref
import ensemble_ref
import lowres_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SHAPES = ((7, 12, 8), (5, 10, 6))
# per axis (c0, step, width, profile) in fine-voxel units, or None = the identity
ALIGNED, FRACTIONAL, OVERLAP, GAUSS = (0.5, 2.0, 2.0, 'box'), (1.05, 2.5, 2.5, 'box'), (1.0, 2.0, 3.0, 'box'), (1.5, 2.0, 2.0, 'gauss')
LATTICES = {'aligned2': (ALIGNED,) * 3, 'ratio2.5+0.3': (FRACTIONAL,) * 3, 'overlap1.5': (OVERLAP,) * 3, 'gauss': (GAUSS,) * 3,
            'inplane_identity': (FRACTIONAL, None, None), 'z_identity': (None, FRACTIONAL, FRACTIONAL)}
SETS = (1, 2)
NTAB = 5
SEED = 0x1234567890ABCDEF
STEP = 7
MODES = ('clean', 'noise', 'keyed')
CASES = [(si, lat, sets) for si in range(len(SHAPES)) for lat in LATTICES for sets in SETS]


def _levels():
    a = np.array([0.99999994, 0.97, 0.81, 0.5, 0.12], np.float32)
    return a, np.sqrt(1 - a.astype(np.float64) ** 2).astype(np.float32)


def _dev(a, offset=False):
    """A device copy; offset: one float off 16-byte alignment."""
    if a is None:
        return None
    a = np.ascontiguousarray(a)
    if not offset:
        return torch.from_numpy(a.copy()).to(DEV)
    buf = torch.empty(a.size + 4, dtype=torch.float32, device=DEV)
    view = buf[1:1 + a.size].view(a.shape)
    view.copy_(torch.from_numpy(a.copy()))
    assert view.data_ptr() % 16 == 4
    return view


def _bits(t):
    return t.contiguous().view(torch.int32)


@functools.lru_cache(maxsize=None)
def _matrices(si, lat):
    out = []
    for size, spec in zip(SHAPES[si], LATTICES[lat]):
        A = np.eye(size) if spec is None else band_ref.weights(size, *spec)[0]
        assert A.shape[0] >= 1
        A.setflags(write=False)
        out.append(A)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def _tables(si, lat):
    from mudiff_hip import ops
    return ops.lowres_tables(*_matrices(si, lat))


@functools.lru_cache(maxsize=None)
def _case(si, lat, sets):
    """x, eta [sets, n, H, W], y = A k, t (the set's level sits in its row 0; the other rows name another one, which must not count),
    keys, the keyed eta of the restatement, and per mode and set the references (a) and (c).  Computed once, shared, never written."""
    n, H, W = SHAPES[si]
    Az, Ay, Ax = _matrices(si, lat)
    tabs = _tables(si, lat)
    g = np.random.default_rng(1000 * si + 10 * sorted(LATTICES).index(lat) + sets)
    x = g.standard_normal((sets, n, H, W)).astype(np.float32)
    eta = g.standard_normal((sets, n, H, W)).astype(np.float32)
    k = np.tanh(g.standard_normal((n, H, W))).astype(np.float32)
    y = R.measure_dense(k, Az, Ay, Ax).astype(np.float32)
    cover = [(band_ref.as_kernel(A) != 0).any(0) for A in (Az, Ay, Ax)]
    covered = cover[0][:, None, None] & cover[1][None, :, None] & cover[2][None, None, :]
    x[:, 0, 0, 0] = -0.0
    free = np.argwhere(~covered)
    if len(free):
        x[(slice(None),) + tuple(free[0])] = -0.0
    t = np.zeros((sets, n), np.int64)
    for s in range(sets):
        t[s, 0] = (s + 1) % NTAB
        t[s, 1:] = (s + 3) % NTAB
    keys = np.stack([np.tile(np.arange(n), sets) + 40, np.repeat(np.arange(sets), n)], 1).astype(np.int64)
    keyed = ensemble_ref.randn_keyed(keys, H * W, SEED, STEP, 9).reshape(sets, n, H, W)
    a_tab, s_tab = _levels()
    ref = {}
    for mode in MODES:
        e = {'clean': None, 'noise': eta, 'keyed': keyed}[mode]
        for s in range(sets):
            a, sg = float(a_tab[t[s, 0]]), float(s_tab[t[s, 0]])
            args = (None if e is None else e[s], a, sg, mode == 'clean')
            dense = R.constrain_dense(x[s], y, Az, Ay, Ax, *args)
            emul = R.constrain_fp32(x[s], y, tabs, *args)
            err_c = float(np.abs(emul.astype(np.float64) - dense).max())
            ref[mode, s] = dict(dense=dense, emul=emul, err_c=err_c, bound=4 * max(err_c, R.EPS32 * float(np.abs(x[s]).max())), eta=args[0],
                                a=a, sg=sg)
    for v in (x, eta, y, t, keys, keyed, covered):
        v.setflags(write=False)
    return dict(x=x, eta=eta, y=y, t=t.reshape(-1), keys=keys, keyed=keyed, covered=covered, ref=ref, mats=(Az, Ay, Ax), tabs=tabs)


def _run(c, mode, x=None, out=None, sl=slice(None), offset=False):
    """ops.lowres_constrain on the sets `sl` of case c."""
    from mudiff_hip import ops
    a_tab, s_tab = (_dev(v) for v in _levels())
    n = c['x'].shape[1]
    rows = slice(None) if sl == slice(None) else slice(sl.start * n, sl.stop * n)
    x = _dev(c['x'][sl], offset) if x is None else x
    kw = dict(clean=True) if mode == 'clean' else dict(noise=_dev(c['eta'][sl], offset)) if mode == 'noise' else \
        dict(keys=_dev(c['keys'][rows]), seed=SEED, step=STEP)
    return ops.lowres_constrain(x, _dev(c['y']), c['tabs'], _dev(c['t'][rows]), 0, a_tab, s_tab, out=out, **kw)


def _check_against_dense(c, mode, got, sets, label):
    Az, Ay, Ax = c['mats']
    N = R.null_basis(Az, Ay, Ax)
    for s in range(sets):
        ref = c['ref'][mode, s]
        g = got[s].cpu().numpy().astype(np.float64)
        x64 = c['x'][s].astype(np.float64)
        err = float(np.abs(g - ref['dense']).max())
        d = g if mode == 'clean' else g - ref['sg'] * ref['eta'].astype(np.float64)
        res = float(np.abs(R.measure_dense(d, Az, Ay, Ax) - (1.0 if mode == 'clean' else ref['a']) * c['y'].astype(np.float64)).max())
        null = float(np.abs(N @ (N.T @ (g - x64).reshape(-1))).max()) if N.shape[1] else 0.0
        exact = np.array_equal(got[s].cpu().numpy().view(np.int32), ref['emul'].view(np.int32))
        print(f'{label} {mode} set {s}: err_c {ref["err_c"]:.3e} |kernel - (a)| {err:.3e} |A (out - s eta) - a y| {res:.3e} '
              f'null-space part of out - x {null:.3e} bound {ref["bound"]:.3e} kernel == (c) bit for bit: {exact}')
        assert exact or mode == 'keyed', 'the kernel and the fp32 emulation of its chain differ in some bit'
        assert err <= ref['bound']
        assert res <= ref['bound']
        assert null <= ref['bound']


@pytest.mark.parametrize('si,lat,sets', CASES)
def test_constrain_against_the_dense_projection(si, lat, sets):
    c = _case(si, lat, sets)
    for mode in MODES:
        x = _dev(c['x'])
        got = _run(c, mode, x=x)
        _check_against_dense(c, mode, got, sets, f'{SHAPES[si]} {lat} sets {sets}')
        assert torch.equal(_bits(x), _bits(_dev(c['x'])))                                # the operand is not written
        again = _run(c, mode, x=got)                                                     # a second application changes nothing
        for s in range(sets):
            assert float((again[s] - got[s]).abs().max()) <= c['ref'][mode, s]['bound']


@pytest.mark.parametrize('lat', LATTICES)
def test_an_operand_one_float_off_alignment(lat):
    """12 x 8 has whole quads, so only the alignment sends this run to the element-by-element instance: same sums, same bits."""
    c = _case(0, lat, 2)
    for mode in MODES:
        got = _run(c, mode, offset=True)
        _check_against_dense(c, mode, got, 2, f'{SHAPES[0]} {lat} offset')
        assert torch.equal(_bits(got), _bits(_run(c, mode)))


@pytest.mark.parametrize('si,lat,sets', CASES)
def test_runs_repeat_sets_are_independent_and_free_pixels_keep_their_bits(si, lat, sets):
    c = _case(si, lat, sets)
    free = torch.from_numpy(~c['covered']).to(DEV)
    for mode in MODES:
        first = _run(c, mode)
        assert torch.equal(_bits(first), _bits(_run(c, mode)))                           # two runs, the same bits
        for s in range(sets if sets > 1 else 0):                                         # a set alone: the bits it gets among two
            assert torch.equal(_bits(_run(c, mode, sl=slice(s, s + 1))[0]), _bits(first[s]))
        x = _dev(c['x'])
        x0 = x.clone()
        assert _run(c, mode, x=x, out=x) is x                                            # in place
        assert torch.equal(_bits(x), _bits(first))
        assert torch.equal(_bits(x[:, free]), _bits(x0[:, free]))                        # pixels under no coarse voxel: x's bits, the -0 too
        assert torch.equal(_bits(first[:, free]), _bits(x0[:, free]))
        if bool(free.any()):
            i = tuple(np.argwhere(~c['covered'])[0])
            assert np.signbit(first[(0,) + i].item()) and first[(0,) + i].item() == 0.0
    from mudiff_hip import ops
    first = _run(c, 'keyed')
    n, H, W = SHAPES[si]
    eta = ops.randn_keyed(_dev(c['keys']), H * W, SEED, STEP, ops.KIND_LOWRES).view(sets, n, H, W)
    a_tab, s_tab = (_dev(v) for v in _levels())
    injected = ops.lowres_constrain(_dev(c['x']), _dev(c['y']), c['tabs'], _dev(c['t']), 0, a_tab, s_tab, noise=eta)
    assert torch.equal(_bits(injected), _bits(first))                                    # the kernel draws what randn_keyed gives kind 9
    other = ops.lowres_constrain(_dev(c['x']), _dev(c['y']), c['tabs'], _dev(c['t']), 0, a_tab, s_tab, keys=_dev(c['keys']), seed=SEED, step=STEP + 1)
    assert not torch.equal(other, first)


@pytest.mark.parametrize('si', range(len(SHAPES)))
@pytest.mark.parametrize('sets', SETS)
def test_identity_in_plane_agrees_with_the_band_kernel(si, sets):
    from mudiff_hip import ops
    c = _case(si, 'inplane_identity', sets)
    a_tab, s_tab = (_dev(v) for v in _levels())
    for mode in ('clean', 'noise'):
        kw = dict(clean=True) if mode == 'clean' else dict(noise=_dev(c['eta']))
        band = ops.band_constrain(_dev(c['x']), _dev(c['y']), c['tabs'].z, _dev(c['t']), 0, a_tab, s_tab, **kw)
        low = _run(c, mode)
        for s in range(sets):
            diff = float((band[s] - low[s]).abs().max())
            print(f'{SHAPES[si]} sets {sets} {mode} set {s}: |lowres - band| {diff:.3e} bound {c["ref"][mode, s]["bound"]:.3e}')
            assert diff <= c['ref'][mode, s]['bound']


@pytest.mark.parametrize('si,lat,sets', CASES)
def test_measure_against_the_dense_product(si, lat, sets):
    from mudiff_hip import ops
    c = _case(si, lat, sets)
    got = ops.lowres_measure(_dev(c['x']), c['tabs'])
    assert tuple(got.shape) == (sets,) + c['tabs'].shape
    for s in range(sets):
        dense = R.measure_dense(c['x'][s], *c['mats'])
        emul = R.measure_fp32(c['x'][s], c['tabs'])
        err_c = float(np.abs(emul.astype(np.float64) - dense).max())
        err = float(np.abs(got[s].cpu().numpy().astype(np.float64) - dense).max())
        print(f'{SHAPES[si]} {lat} sets {sets} set {s}: measure err_c {err_c:.3e} |kernel - (a)| {err:.3e}')
        assert err <= 4 * max(err_c, R.EPS32 * float(np.abs(c['x'][s]).max()))


def test_entries_refuse_bad_arguments_before_any_launch():
    import mudiff_hip
    from mudiff_hip import ops
    lib = mudiff_hip.load()
    tabs = _tables(0, 'ratio2.5+0.3')
    dev = torch.device(DEV)
    sz, sy, sx = (t.on(dev) for t in (tabs.z, tabs.y, tabs.x))
    n, H, W = SHAPES[0]
    x = torch.zeros(1, n, H, W, device=DEV)
    y = torch.zeros(tabs.shape, device=DEV)
    assert lib.mud_lowres_ws_floats(1, n, *tabs.shape) == (n + tabs.z.m) * tabs.y.m * tabs.x.m
    assert lib.mud_lowres_ws_floats(0, n, *tabs.shape) == -1 and lib.mud_lowres_ws_floats(1, n, 2, 0, 2) == -1
    work = torch.full((ops.lowres_ws_floats(1, tabs),), 7.0, device=DEV)
    p = lambda v: None if v is None else C.c_void_p(v.data_ptr())      # noqa: E731
    ref = lambda v: None if v is None else C.byref(v)                  # noqa: E731

    def constrain(z=sz, y_tab=sy, x_tab=sx, x_=x, y_=y, out_=x, work_=work, H_=H, W_=W, rows=n, kind=9, step=0, clean=1):
        return lib.mud_lowres_constrain(p(x_), p(y_), ref(z), ref(y_tab), ref(x_tab), H_, W_, rows, p(work_), None, None, C.c_uint64(0), step, kind,
                                        None, 0, None, None, 1, clean, p(out_), None)

    bad = lambda st, **kw: type(st)(**{**{f: getattr(st, f) for f, _ in st._fields_}, **kw})      # noqa: E731
    refused = (dict(z=None), dict(y_tab=None), dict(x_tab=None), dict(z=bad(sz, m=0)), dict(y_tab=bad(sy, m=0)), dict(x_tab=bad(sx, m=0)),
               dict(z=bad(sz, m=257)), dict(y_tab=bad(sy, bw=9)), dict(x_tab=bad(sx, nnz=0)), dict(x_tab=bad(sx, lc=None)),
               dict(y_tab=bad(sy, n=H + 1)), dict(x_tab=bad(sx, n=W - 1)), dict(H_=H + 1), dict(W_=W + 4), dict(rows=n + 1), dict(rows=0),
               dict(rows=65536 // n * n + n), dict(kind=16), dict(step=1 << 24), dict(x_=None), dict(y_=None), dict(out_=None), dict(work_=None),
               dict(work_=x), dict(work_=y), dict(out_=y), dict(clean=0))
    for kw in refused:
        assert constrain(**kw) == 1 and b'mud_lowres_constrain' in lib.mud_last_error(), kw
    torch.cuda.synchronize()
    assert bool((work == 7.0).all()) and bool((x == 0).all())                            # nothing was launched
    assert constrain() == 0
    ax = torch.zeros((1,) + tabs.shape, device=DEV)

    def measure(z=sz, y_tab=sy, x_tab=sx, x_=x, ax_=ax, work_=work, rows=n):
        return lib.mud_lowres_measure(p(x_), ref(z), ref(y_tab), ref(x_tab), H, W, rows, p(work_), p(ax_), None)

    assert measure() == 0
    for kw in (dict(x_=None), dict(ax_=None), dict(work_=None), dict(z=bad(sz, m=0)), dict(y_tab=bad(sy, n=H - 1)), dict(x_tab=bad(sx, n=W + 1)),
               dict(rows=n - 1), dict(ax_=x), dict(work_=ax)):
        assert measure(**kw) == 1 and b'mud_lowres_measure' in lib.mud_last_error(), kw
    with pytest.raises(mudiff_hip.MudiffHipError, match='lowres_constrain'):
        ops.lowres_constrain(x[0], y, tabs, None, 0, None, None, clean=True)             # not [sets, n, H, W]
    with pytest.raises(mudiff_hip.MudiffHipError, match='lowres_constrain'):
        ops.lowres_constrain(x, y[:1], tabs, None, 0, None, None, clean=True)
    with pytest.raises(mudiff_hip.MudiffHipError, match='lowres_measure'):
        ops.lowres_measure(x.transpose(2, 3), tabs)
    torch.cuda.synchronize()
