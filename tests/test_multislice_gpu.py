"""GPU: the data-consistency step of accelerated thick slices (csrc/slab_kspace.hip: mud_slab_kspace_constrain; ops.slab_kspace_constrain,
constraints.SlabKSpaceRows) against the fp64 restatement in tests/multislice_ref.py.  DESIGN.md section 5.28.

The accuracy rule, per member row in L2 over the image: multislice_ref.bound (kspace's 3 rule(S) and thick's rounding count together) and
<= 4 x the error the same chain makes in torch on the CPU in fp32 / complex64, computed here (test_kspace_gpu.py's FACTOR rule)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import kspace_ref as KR
import multislice_ref as R
import thick_ref as TR

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GRID = [(S, L, G) for S in (16, 32) for L in (1, 2, 5, 16) for G in (1, 3)] + [(512, 2, 1)]      # the smallest; an odd log2; 8 lines a workgroup
GRID += [(128, 2, 1), (256, 5, 1)]      # the row passes' own tiles: 16 lines up to S = 64, then 8 and 4 (and 2 at S = 512)
NTAB = 5
FACTOR = 4.0
SEED = 0x1234567890ABCDEF


def _tables():
    a = np.array([0.99999994, 0.97, 0.81, 0.5, 0.12], np.float32)
    return a, np.sqrt(1 - a.astype(np.float64) ** 2).astype(np.float32)


def _dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).to(DEV)      # (a copy: the shared cases are read-only)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _l2(a):
    return np.sqrt((np.abs(np.asarray(a)).astype(np.float64) ** 2).sum((-2, -1)))


@functools.lru_cache(maxsize=None)
def _case(S, L, G):
    """Member l of group j is row l (G + 1) + j: the groups interleave and row l (G + 1) + G of every stripe is free (S = 512: one
    group of 2 in 3 rows).  The table is one slot wider than L (L < 16), an unused tail of -1; with G = 3 and L > 1 the last group is
    one member short as well.  Levels per row, both clamped ends among the first members.  Computed once, shared, never written."""
    g = np.random.default_rng(100000 + 1000 * S + 10 * L + G)
    rows = L * (G + 1) if S < 512 else 3                            # (S = 128, 256: one group, a free row after every member)
    W = min(L + 1, 16)
    members = np.full((G, W), -1, np.int32)
    members[:, :L] = [[l * (G + 1) + j for l in range(L)] for j in range(G)] if S < 512 else [[0, 2]]
    kind = 'gauss' if L % 2 else 'box'
    w = np.ones((G, W), np.float32)                                # (an unused slot's weight is never read)
    w[:, :L] = TR.profile(L, kind).astype(np.float32)
    if G == 3 and L > 1:
        members[-1, L - 1] = -1
        w[-1, :L - 1] = TR.profile(L - 1, kind).astype(np.float32)
    gn = np.ones((G, W), np.float32)
    for j in range(G):
        n = int((members[j] >= 0).sum())
        gn[j, :n] = TR.gains(w[j, :n])
    x = g.standard_normal((rows, S, S)).astype(np.float32)
    free = np.setdiff1d(np.arange(rows), members[members >= 0])
    x[free[0], 0, 0] = -0.0                                        # a free row's -0 ...
    x[0, 0, 1] = -0.0                                              # ... and a member's
    eta = g.standard_normal((rows, S, S)).astype(np.float32)
    k = np.tanh(g.standard_normal((rows, S, S))).astype(np.float32)
    masks = {mr: np.stack([KR.symmetrise((g.random((S, S)) < 0.3).astype(np.uint8)) for _ in range(mr)]) for mr in {1, G}}
    assert all(0 < m.sum() < m.size for m in masks.values())
    ys = {mr: R.measure(k, members, w, m).astype(np.complex64) for mr, m in masks.items()}      # the fp32 measurements every side is given
    t = g.integers(-2, NTAB + 2, rows).astype(np.int64)            # per-row levels; only a group's first member's counts
    t[members[0, 0]] = -1
    t[members[-1, 0]] = NTAB + 1 if G > 1 else -1
    keys = np.stack([np.arange(rows) + 40, np.arange(rows) % 3], 1).astype(np.int64)
    for a in (members, w, gn, x, eta, k, t, keys) + tuple(masks.values()) + tuple(ys.values()):
        a.setflags(write=False)
    return dict(rows=rows, members=members, w=w, g=gn, x=x, eta=eta, k=k, masks=masks, ys=ys, t=t, keys=keys, free=free.tolist())


def _torch_chain(c, y, m, toff, a_tab, s_tab, clean):
    """The same chain in torch on the CPU, fp32 / complex64, in the kernel's order."""
    x, eta, out = torch.from_numpy(np.array(c['x'])), torch.from_numpy(np.array(c['eta'])), torch.from_numpy(np.array(c['x']))
    y, m = torch.from_numpy(np.array(y)), torch.from_numpy(np.array(m)) != 0
    for j, row in enumerate(c['members']):
        slots = [(l, int(r)) for l, r in enumerate(row) if r >= 0]
        lv = int(np.clip(c['t'][slots[0][1]] + toff, 0, NTAB - 1))
        a, s = (1.0, 0.0) if clean else (float(a_tab[lv]), float(s_tab[lv]))
        acc = torch.zeros_like(x[0])
        for l, r in slots:
            d = x[r] if clean else x[r] - torch.tensor(s, dtype=torch.float32) * eta[r]
            acc = acc + float(c['w'][j, l]) * d
        res = torch.where(m[0 if m.shape[0] == 1 else j], torch.fft.fft2(acc, norm='ortho') - (y[j] if clean else torch.tensor(a, dtype=torch.float32) * y[j]),
                          torch.zeros((), dtype=torch.complex64))
        cor = torch.fft.ifft2(res, norm='ortho').real
        for l, r in slots:
            out[r] = x[r] - float(c['g'][j, l]) * cor
    return out.numpy()


def _op(c, mr, toff=0, clean=False, **kw):
    from mudiff_hip import ops
    a_tab, s_tab = _tables()
    kw.setdefault('gains', c['g'])
    x = kw.pop('x', None)
    return ops.slab_kspace_constrain(_dev(c['x']) if x is None else x, _dev(c['ys'][mr]), _dev(c['masks'][mr]), c['members'], c['w'], _dev(c['t']), toff,
                                     _dev(a_tab), _dev(s_tab), clean=clean, **kw)


@pytest.mark.parametrize('S,L,G', GRID)
def test_constrain_with_injected_noise_against_the_restatement(S, L, G):
    c = _case(S, L, G)
    a_tab, s_tab = _tables()
    x = _dev(c['x'])
    used = sorted(int(r) for r in c['members'][c['members'] >= 0])
    worst, worst_t = 0.0, 0.0
    for mr in sorted(c['masks']):
        m, y = c['masks'][mr], c['ys'][mr]
        for toff in (0, 1):
            for clean in (False, True):
                got = _op(c, mr, toff, clean, x=x, noise=_dev(c['eta']))
                args = (c['x'], y, c['members'], c['w'], c['g'], c['eta'], c['t'], toff, a_tab, s_tab, clean)
                want = R.constrain(c['x'], y, m, *args[2:])
                bound = R.bound(*args)
                err = _l2(got.cpu().numpy().astype(np.float64) - want)
                terr = _l2(_torch_chain(c, y, m, toff, a_tab, s_tab, clean).astype(np.float64) - want)
                worst = max(worst, float(np.max(err[used] / bound[used])))
                worst_t = max(worst_t, float(np.max(err[used] / np.maximum(terr[used], 1e-300))))
                assert (err[used] <= bound[used]).all(), (mr, toff, clean, err[used] / bound[used])
                assert (err[used] <= FACTOR * terr[used]).all(), (mr, toff, clean, err[used] / terr[used])
                assert torch.equal(_bits(got[c['free']]), _bits(x[c['free']]))           # free rows: x_new's bits, the -0 included
                assert np.signbit(got[c['free'][0], 0, 0].item())
    print(f'S={S} L={L} G={G}: worst error / bound {worst:.4f}, worst error / torch CPU complex64 error {worst_t:.3f}')
    assert torch.equal(_bits(x), _bits(_dev(c['x'])))                                    # the operand is not written


@pytest.mark.parametrize('S,L,G', GRID)
def test_keyed_draw_in_place_shapes_zero_mask_and_independence_of_the_batch(S, L, G):
    from mudiff_hip import ops
    c = _case(S, L, G)
    a_tab, s_tab = (_dev(v) for v in _tables())
    rows = c['rows']
    x, t, keys, eta = _dev(c['x']), _dev(c['t']), _dev(c['keys']), _dev(c['eta'])
    y, m = _dev(c['ys'][G]), _dev(c['masks'][G])
    step = 7
    kw = dict(gains=c['g'], keys=keys, seed=SEED, step=step)
    call = lambda x_, **k: ops.slab_kspace_constrain(x_, y, m, c['members'], c['w'], t, 0, a_tab, s_tab, **k)      # noqa: E731
    # the keyed draw is the injected ops.randn_keyed row of kind 7, bit for bit; another step changes the bits
    keyed = call(x, **kw)
    draw = ops.randn_keyed(keys, S * S, SEED, step, ops.KIND_MULTISLICE).view(rows, S, S)
    assert torch.equal(_bits(keyed), _bits(call(x, gains=c['g'], noise=draw)))
    assert not torch.equal(_bits(keyed), _bits(call(x, **dict(kw, step=8))))
    # out is x_new: the same bits as out of place, with and without a draw
    for clean in (False, True):
        want = call(x, gains=c['g'], noise=eta, clean=clean)
        inplace = x.clone()
        assert call(inplace, gains=c['g'], noise=eta, clean=clean, out=inplace) is inplace
        assert torch.equal(_bits(inplace), _bits(want))
    # [rows, 1, S, S] as the sampler holds it
    assert torch.equal(_bits(call(x[:, None], gains=c['g'], noise=eta[:, None])[:, 0]), _bits(call(x, gains=c['g'], noise=eta)))
    # a mask of zeros: the bits of x_new on every row, a negative zero included
    for mr in (1, G):
        zero = torch.zeros(mr, S, S, device=DEV, dtype=torch.uint8)
        for clean in (False, True):
            got = ops.slab_kspace_constrain(x, y, zero, c['members'], c['w'], t, 0, a_tab, s_tab, gains=c['g'], noise=eta, clean=clean)
            assert torch.equal(_bits(got), _bits(x))
    # a group alone equals the group inside its batch, also with its rows in other places
    for clean in (False, True):
        whole = call(x, clean=clean, **kw)
        for j in range(G):
            mem = c['members'][j]
            n = int((mem >= 0).sum())
            r = torch.from_numpy(mem[:n].astype(np.int64)).to(DEV)
            tab = np.full((1, mem.shape[0]), -1, np.int32)
            tab[0, :n] = np.arange(n)
            one = dict(gains=c['g'][j:j + 1], keys=keys[r], seed=SEED, step=step, clean=clean)
            alone = ops.slab_kspace_constrain(x[r], y[j:j + 1], m[j:j + 1], tab, c['w'][j:j + 1], t[r], 0, a_tab, s_tab, **one)
            assert torch.equal(_bits(alone), _bits(whole[r]))
            perm = torch.arange(n - 1, -1, -1, device=DEV)                               # reversed positions, the same table order
            tab[0, :n] = np.arange(n)[::-1]
            one['keys'] = keys[r][perm]
            moved = ops.slab_kspace_constrain(x[r][perm], y[j:j + 1], m[j:j + 1], tab, c['w'][j:j + 1], t[r][perm], 0, a_tab, s_tab, **one)
            assert torch.equal(_bits(moved[perm]), _bits(whole[r]))


@pytest.mark.parametrize('S', (16, 32, 256, 512))
def test_one_member_with_unit_weight_has_the_bits_of_kspace_constrain(S):
    """L = 1, w = g = 1: acc = 0 + 1 * d and c = 1 * re are exact, so the chain is mud_kspace_constrain's on those rows."""
    from mudiff_hip import ops
    rows = 5 if S < 512 else 3
    g = np.random.default_rng(S)
    a_tab, s_tab = (_dev(v) for v in _tables())
    x, eta = (_dev(g.standard_normal((rows, S, S)).astype(np.float32)) for _ in range(2))
    x[1, 0, :2] = torch.tensor([-0.0, 0.0], device=DEV)
    pick = [3, 1, 4] if S < 512 else [2, 0]                                              # groups in another order than the rows
    members = np.array([[r] for r in pick], np.int32)
    idx = torch.tensor(pick, device=DEV)
    mask = _dev(np.stack([KR.symmetrise((g.random((S, S)) < 0.3).astype(np.uint8)) for _ in pick]))
    y = torch.where(mask != 0, ops.fft2(_dev(np.tanh(g.standard_normal((len(pick), S, S))).astype(np.float32))), torch.zeros((), device=DEV, dtype=torch.complex64))
    t = _dev(g.integers(-1, NTAB + 1, rows).astype(np.int64))
    keys = _dev(np.stack([np.arange(rows) + 9, np.arange(rows) % 2], 1).astype(np.int64))
    ones = np.ones((len(pick), 1), np.float32)
    for kw in (dict(noise=eta), dict(keys=keys, seed=SEED, step=3), dict(clean=True)):
        got = ops.slab_kspace_constrain(x, y, mask, members, ones, t, 1, a_tab, s_tab, gains=ones, kind=ops.KIND_KSPACE, **kw)
        kk = dict(kw)
        if 'noise' in kk:
            kk['noise'] = eta[idx]
        if 'keys' in kk:
            kk['keys'] = keys[idx]
        want = ops.kspace_constrain(x[idx], y, mask, t[idx], 1, a_tab, s_tab, **kk)
        assert torch.equal(_bits(got[idx]), _bits(want)), kw
        rest = [r for r in range(rows) if r not in pick]
        assert torch.equal(_bits(got[rest]), _bits(x[rest]))


@pytest.mark.parametrize('S,L,G', [(16, 5, 3), (32, 16, 1), (512, 2, 1)])
def test_the_numeric_identities_of_the_clean_step(S, L, G):
    """A mask of ones: ops.slab_constrain given Re F^H y, within the bound.  A Hermitian mask: the measured coefficients of the slab
    average are y, the unmeasured ones those of x_new's average, within 3 rule(S)-scaled norms."""
    from mudiff_hip import ops
    c = _case(S, L, G)
    x = _dev(c['x'])
    ones = np.ones((1, S, S), np.uint8)
    y1 = R.measure(c['k'], c['members'], c['w'], ones).astype(np.complex64)
    got = ops.slab_kspace_constrain(x, _dev(y1), _dev(ones), c['members'], c['w'], None, 0, None, None, gains=c['g'], clean=True)
    yi = ops.fft2(_dev(y1), inverse=True).real.contiguous()
    want = ops.slab_constrain(x.view(c['rows'], -1), yi.view(G, -1), c['members'], c['w'], None, 0, None, None, gains=c['g'], clean=True).view_as(x)
    bound = R.bound(c['x'], y1, c['members'], c['w'], c['g'], None, None, 0, None, None, True)
    used = sorted(int(r) for r in c['members'][c['members'] >= 0])
    err = _l2((got - want).cpu().numpy())
    print(f'S={S} L={L} G={G}: full mask against slab_constrain, worst error / bound {np.max(err[used] / bound[used]):.4f}')
    assert (err[used] <= bound[used]).all()
    m, y = c['masks'][1], c['ys'][1]
    assert np.array_equal(KR.symmetrise(m[0])[None], m) and 0 < int(m.sum()) < m.size
    got = ops.slab_kspace_constrain(x, _dev(y), _dev(m), c['members'], c['w'], None, 0, None, None, gains=c['g'], clean=True).cpu().numpy()
    F, Fx = KR.fft2(TR.average(got, c['members'], c['w'])), KR.fft2(TR.average(c['x'], c['members'], c['w']))
    scale = _l2(TR.average(np.abs(c['x']), c['members'], c['w'])) + _l2(y)
    on, off = _l2(np.where(m != 0, F - y, 0)), _l2(np.where(m == 0, F - Fx, 0))
    print(f'S={S} L={L} G={G}: measured |F(A out) - y| / scale {np.max(on / scale):.3e}, unmeasured {np.max(off / scale):.3e} '
          f'(rule x 3: {3 * KR.rule(S):.3e})')
    assert (on <= 3 * KR.rule(S) * scale).all() and (off <= 3 * KR.rule(S) * scale).all()


def test_many_groups_take_more_than_one_launch():
    """40 groups of one row at S = 16: the tables travel as kernel arguments, 32 groups a launch; work, y and mask move on with them."""
    from mudiff_hip import ops
    g = np.random.default_rng(3)
    G, S = 40, 16
    members = g.permutation(G + 2)[:G].reshape(G, 1).astype(np.int32)
    w = np.full((G, 1), 1.0, np.float32)
    x, k = g.standard_normal((G + 2, S, S)).astype(np.float32), np.tanh(g.standard_normal((G + 2, S, S))).astype(np.float32)
    mask = np.stack([KR.symmetrise((g.random((S, S)) < 0.3).astype(np.uint8)) for _ in range(G)])
    y = R.measure(k, members, w, mask).astype(np.complex64)
    got = ops.slab_kspace_constrain(_dev(x), _dev(y), _dev(mask), members, w, None, 0, None, None, clean=True)
    want = R.constrain(x, y, mask, members, w, w, None, None, 0, None, None, True)
    err, bound = _l2(got.cpu().numpy() - want), R.bound(x, y, members, w, w, None, None, 0, None, None, True)
    used = members[:, 0].astype(np.int64)
    assert (err[used] <= bound[used]).all()
    free = np.setdiff1d(np.arange(G + 2), used)
    assert torch.equal(_bits(got[free]), _bits(_dev(x)[free]))
    used = torch.from_numpy(used).to(DEV)
    same = ops.kspace_constrain(_dev(x)[used], _dev(y), _dev(mask), None, 0, None, None, clean=True)      # every group: its own y and mask
    assert torch.equal(_bits(got[used]), _bits(same))


def test_bad_arguments_are_refused_before_a_launch():
    import mudiff_hip
    from mudiff_hip import MudiffHipError, ops
    lib = mudiff_hip.load()
    rows, S, L = 6, 16, 3
    f = dict(device=DEV, dtype=torch.float32)
    cz = dict(device=DEV, dtype=torch.complex64)
    x, out = torch.randn(rows, S, S, **f), torch.full((rows, S, S), 7.0, **f)
    y, work, m = torch.zeros(2, S, S, **cz), torch.zeros(2, S, S, **cz), torch.ones(2, S, S, device=DEV, dtype=torch.uint8)
    t, keys = torch.zeros(rows, device=DEV, dtype=torch.int64), torch.zeros(rows, 2, device=DEV, dtype=torch.int64)
    tab = torch.ones(NTAB, **f)
    p = lambda v: None if v is None else C.c_void_p(v.data_ptr())                        # noqa: E731
    h = lambda a: C.c_void_p(a.ctypes.data)                                              # noqa: E731
    good_m = np.array([[0, 2, 4], [1, 3, -1]], np.int32)
    good_w = np.full((2, 3), 0.25, np.float32)

    def call(mem=good_m, w=good_w, g=good_w, L_=L, groups=2, kind=7, step=0, clean=0, x_=x, y_=y, m_=m, mask_rows=2, keys_=keys, t_=t, rows_=rows, S_=S,
             out_=out, work_=work, off=0):
        mem, w, g = (np.ascontiguousarray(v) for v in (mem, w, g))
        xp = None if x_ is None else C.c_void_p(x_.data_ptr() + off)
        return lib.mud_slab_kspace_constrain(xp, p(y_), p(m_), mask_rows, h(mem), h(w), h(g), groups, L_, None, p(keys_), 0, step, kind, p(t_), 0,
                                             p(tab), p(tab), NTAB, clean, p(out_), p(work_), rows_, S_, None)

    def edit(a, i, v):
        a = a.copy()
        a[i] = v
        return a

    assert call() == 0
    torch.cuda.synchronize()
    assert bool((out[5] == x[5]).all()) and not bool((out[0] == 7.0).any())              # (row 5 is free: copied)
    out.fill_(7.0)
    work.zero_()
    bad = [(dict(S_=24), b'power of two'), (dict(S_=1024), b'power of two'), (dict(S_=8), b'power of two'),
           (dict(rows_=1 << 23), b'2^31'), (dict(rows_=0), b'rows must'), (dict(mask_rows=3), b'mask_rows'), (dict(mask_rows=0), b'mask_rows'),
           (dict(mem=edit(good_m, (0, 1), 6)), b'members'), (dict(mem=edit(good_m, (0, 1), -2)), b'members'),   # outside [0, rows)
           (dict(mem=edit(good_m, (1, 0), 2)), b'members'), (dict(mem=edit(good_m, (0, 1), 0)), b'members'),    # in two groups; twice in one
           (dict(mem=edit(good_m, (1, slice(None)), -1)), b'members'),                                         # a group with no member
           (dict(w=edit(good_w, (0, 0), 0.0)), b'weights'), (dict(w=edit(good_w, (1, 1), np.nan)), b'weights'),
           (dict(g=edit(good_w, (0, 2), 0.0)), b'gains'), (dict(g=edit(good_w, (0, 2), np.inf)), b'gains'),
           (dict(L_=0), b'L must'), (dict(L_=17), b'L must'), (dict(groups=-1), b'groups'), (dict(groups=7), b'groups'),
           (dict(kind=16), b'kind'), (dict(kind=-1), b'kind'), (dict(step=-1), b'step'), (dict(step=1 << 24), b'step'),
           (dict(x_=None), b'null'), (dict(out_=None), b'null'), (dict(y_=None), b'null'), (dict(m_=None), b'null'), (dict(work_=None), b'null'),
           (dict(t_=None), b'null'), (dict(keys_=None), b'keys'), (dict(off=4), b'aligned'), (dict(work_=out), b'work must'),
           (dict(work_=y), b'work must')]
    for kw, word in bad:
        assert call(**kw) == 1 and b'mud_slab_kspace_constrain' in lib.mud_last_error() and word in lib.mud_last_error(), (kw, lib.mud_last_error())
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((work == 0).all())                           # nothing was launched, nothing was copied
    assert lib.mud_randn_keyed(p(out), rows, S * S, p(keys), 0, 0, 3, None) == 1          # kinds 3 and 4 stay refused, 7 is taken
    assert lib.mud_randn_keyed(p(out), rows, S * S, p(keys), 0, 0, 4, None) == 1
    assert bool((out == 7.0).all())
    assert lib.mud_randn_keyed(p(out), rows, S * S, p(keys), 0, 0, 7, None) == 0
    # the wrappers' own checks
    with pytest.raises(MudiffHipError):
        ops.slab_kspace_constrain(x, y[:1], m, good_m, good_w, None, 0, None, None, clean=True)          # one y for two groups
    with pytest.raises(MudiffHipError):
        ops.slab_kspace_constrain(x, y.real.contiguous(), m, good_m, good_w, None, 0, None, None, clean=True)
    with pytest.raises(MudiffHipError):
        ops.slab_kspace_constrain(x, y, torch.ones(3, S, S, device=DEV, dtype=torch.uint8), good_m, good_w, None, 0, None, None, clean=True)
    with pytest.raises(MudiffHipError):
        ops.slab_kspace_constrain(x, y, m, good_m, good_w, None, 0, None, None)                          # no t, no tables
    with pytest.raises(MudiffHipError):
        ops.slab_kspace_constrain(x, y, m, good_m, good_w, t, 0, tab, tab)                               # neither noise nor keys
    with pytest.raises(MudiffHipError, match='named twice'):
        ops.slab_kspace_constrain(x, y, m, edit(good_m, (1, 0), 2), good_w, None, 0, None, None, clean=True)
    with pytest.raises(MudiffHipError):
        ops.slab_kspace_constrain(torch.zeros(rows, 24, 24, **f), y, m, good_m, good_w, None, 0, None, None, clean=True)
    with pytest.raises(MudiffHipError):
        ops.slab_kspace_constrain(x, y, m, good_m, good_w, None, 0, None, None, clean=True, work=torch.zeros(1, S, S, **cz))
    with pytest.raises(MudiffHipError):
        ops.slab_kspace_constrain(x.cpu(), y, m, good_m, good_w, None, 0, None, None, clean=True)


def test_sample_keyed_takes_the_constraint_and_stays_what_it_was_without():
    """GraphSampler.sample_keyed(constraint=SlabKSpaceRows(...)): the measured coefficients of the slab averages of the result are y under
    the rule, a slab alone equals the slab in its batch, the constraint is refused with known, kspace and thick, and without it the
    result is bit for bit the one of a sampler that never saw it.  In a child process with MUD_DETERMINISTIC=1 (read at import): every
    GroupNorm then reduces in a fixed order."""
    import os
    import subprocess
    import sys
    from conftest import PKG, REPO
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([REPO, PKG, os.path.join(REPO, 'tests'), os.environ.get('PYTHONPATH', '')]), MUD_DETERMINISTIC='1')
    c = subprocess.run([sys.executable, '-c', 'import test_multislice_gpu as T; T.sampler_checks(); print("SAMPLER-OK")'], cwd=REPO, env=env,
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
    B, S, L, T = 7, 16, 3, int(cfg.num_timesteps)
    sampler = Sm.GraphSampler(Sm.Posterior_Coefficients(cfg, DEV), g1, g2, cfg, B, S, S, DEV)
    g = np.random.default_rng(11)
    conds = [_dev(np.tanh(g.standard_normal((B, 1, S, S))).astype(np.float32)) for _ in range(3)]
    k = np.tanh(g.standard_normal((B, S, S))).astype(np.float32)
    members = np.array([[0, 1, 2], [4, 5, 6]], np.int32)                                 # row 3 is a gap slice
    w = TR.profile(L, 'gauss').astype(np.float32)
    m = KR.symmetrise((g.random((S, S)) < 0.4).astype(np.uint8))[None]
    y = R.measure(k, members, w, m).astype(np.complex64)
    keys = torch.tensor([[4 + r, r % 2] for r in range(B)])
    before = sampler.sample_keyed(*conds, keys, 31, T)
    con = lambda y_=y, mem=members: Cn.SlabKSpaceRows((_dev(y_), _dev(m), mem, w, None))      # noqa: E731
    out = sampler.sample_keyed(*conds, keys, 31, T, constraint=con())
    work = sampler._ks_work
    x_new = sampler.thick_x_new.clone()                                                  # what the last reverse step gave the constraint
    assert not torch.equal(out, before)
    assert torch.equal(out[3], x_new[3])                                                 # the free row: copied

    def residual_ok(res, given):
        F = KR.fft2(TR.average(res[:, 0].cpu().numpy(), members, w))
        scale = _l2(TR.average(np.abs(given[:, 0].cpu().numpy()), members, w)) + _l2(y)
        on = _l2(np.where(m != 0, F - y, 0))
        print(f'sampler: worst measured residual / (3 rule x scale) {np.max(on / (3 * KR.rule(S) * scale)):.3f}')
        return (on <= 3 * KR.rule(S) * scale).all()

    assert residual_ok(out, x_new)
    again = sampler.sample_keyed(*conds, keys, 31, T, constraint=con(), coupling='shared', resample=2)
    assert sampler._ks_work is work and torch.isfinite(again).all() and residual_ok(again, sampler.thick_x_new)
    assert torch.equal(sampler.sample_keyed(*conds, keys, 31, T), before)                # without the constraint: what it was
    assert torch.equal(sampler.sample_keyed(*conds, keys, 31, T, constraint=con(y[:0], members[:0])), before)      # no group: free
    # a slab alone (the rest of the batch: padding in no group) equals the slab in its batch
    rows = [4, 5, 6, 6, 6, 6, 6]
    alone = sampler.sample_keyed(*[c[rows] for c in conds], keys[rows], 31, T, constraint=con(y[1:], np.array([[0, 1, 2]], np.int32)))
    assert torch.equal(alone[:3], out[4:7])
    zeros = torch.zeros(B, 1, S, S, device=DEV)
    with pytest.raises(ValueError, match='exclusive'):
        sampler.sample_keyed(*conds, keys, 31, T, constraint=con(), known=zeros, known_mask=zeros.to(torch.uint8))
    with pytest.raises(ValueError, match='exclusive'):
        sampler.sample_keyed(*conds, keys, 31, T, constraint=con(), kspace=(torch.zeros(B, S, S, device=DEV, dtype=torch.complex64),
                                                                            torch.zeros(1, S, S, device=DEV, dtype=torch.uint8)))
    with pytest.raises(ValueError, match='exclusive'):
        sampler.sample_keyed(*conds, keys, 31, T, constraint=con(), thick=(zeros[:2, 0], members, w, None))
    with pytest.raises(ValueError, match='multislice'):
        sampler.sample_keyed(*conds, keys, 31, T, constraint=con(y[:1]))
    with pytest.raises(ValueError, match='multislice'):
        sampler.sample_keyed(*conds, keys, 31, T, constraint=con(mem=members + 3))        # a row outside the batch
    odd = Sm.GraphSampler.__new__(Sm.GraphSampler)                                       # the size check needs no captured graph
    odd.B, odd.H, odd.W = B, 24, 24
    with pytest.raises(ValueError, match='power of two'):
        Sm.GraphSampler.sample_keyed(odd, *conds, keys, 31, T, constraint=con())
    # an ensemble: a chunk ends before a slab it would cut, and the samples do not depend on the chunks
    from mudiff_hip import ensemble as E, multislice as M
    n, starts = 8, [1, 5]
    c8 = [_dev(np.tanh(g.standard_normal((n, 1, S, S))).astype(np.float32)) for _ in range(3)]
    avg = ops.slab_average(_dev(np.tanh(g.standard_normal((n, S, S))).astype(np.float32)), [[1, 2, 3], [5, 6, 7]], w)
    y8 = torch.where(_dev(m) != 0, ops.fft2(avg), torch.zeros((), device=DEV, dtype=torch.complex64))
    report = lambda: dict(slabs=[dict(measured=True), dict(measured=True)])              # noqa: E731
    meas = lambda: M.MultisliceMeasurement(y8, _dev(m), starts, n, w, report(), 1, dict(baseline=False))      # noqa: E731
    m1, m2 = meas(), meas()
    whole = E.sample_ensemble(cfg, g1, g2, c8, 2, 31, sampler=sampler, constraint=m1, return_samples=True)
    cut = E.sample_ensemble(cfg, g1, g2, c8, 2, 31, sampler=sampler, constraint=m2, return_samples=True, chunk=3)      # chunks 0, 1..3, 4, 5..7
    assert all(torch.equal(a_, b_) for a_, b_ in zip(whole, cut)) and torch.equal(m1.residual, m2.residual) and bool((m1.y_norm > 0).all())
    assert bool((m1.residual * m1.y_norm <= 3 * KR.rule(S) * (m1.x_norm + m1.y_norm)).all())
    assert m1.finish()['max_residual'] == float(m1.residual.max())
    assert not torch.equal(whole[2], E.sample_ensemble(cfg, g1, g2, c8, 2, 31, sampler=sampler, return_samples=True)[2])
    with pytest.raises(ValueError, match='chunk'):
        E.sample_ensemble(cfg, g1, g2, c8, 2, 31, sampler=sampler, constraint=meas(), chunk=2)
