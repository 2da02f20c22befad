"""GPU: the thick-slice data-consistency step (csrc/slab.hip: mud_slab_constrain, mud_slab_average; ops.slab_constrain, ops.slab_average,
GraphSampler.sample_keyed(thick=)) against the fp64 restatement in tests/thick_ref.py.  DESIGN.md section 5.27.

The accuracy rules count the roundings of the kernel's chain (thick_ref.bound_out, thick_ref.bound_residual); an fp32 emulation of the
chain stays below 0.6 of each (tests/test_thick_host.py).  Shapes: row_len 4 (one quad), 33 (element by element, a cut quad), 256,
1028 (more than one workgroup of 256 quads, not a multiple of it); L 1, 2, 5, 16; one group, and three interleaved groups with free
rows between their stripes, an unused tail in the last group's table and a duplicated padding row outside every group."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import thick_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ROW_LENS = (4, 33, 256, 1028)
LS = (1, 2, 5, 16)
GROUPS = (1, 3)
NTAB = 5
SEED = 0x1234567890ABCDEF


def _tables():
    a = np.array([0.99999994, 0.97, 0.81, 0.5, 0.12], np.float32)
    return a, np.sqrt(1 - a.astype(np.float64) ** 2).astype(np.float32)


def _dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).to(DEV)      # (a copy: the shared cases are read-only)


@functools.lru_cache(maxsize=None)
def _case(row_len, L, G):
    """Member l of group j is row l (G + 1) + j: the groups interleave, row l (G + 1) + G of every stripe is free, and the last row
    repeats the one before it (a padded batch).  With G = 3 and L > 1 the last group's table ends in an unused slot, whose row is free.
    Computed once, shared, never written."""
    g = np.random.default_rng(1000 * row_len + 10 * L + G)
    rows = L * (G + 1) + 1
    members = np.array([[l * (G + 1) + j for l in range(L)] for j in range(G)], np.int32)
    if G == 3 and L > 1:
        members[-1, -1] = -1
    kind = 'gauss' if L % 2 else 'box'
    w = np.where(members >= 0, R.profile(L, kind).astype(np.float32)[None], np.float32(0))
    if G == 3 and L > 1:                                           # the shortened group's own profile, so that its weights sum to 1
        w[-1, :L - 1] = R.profile(L - 1, kind).astype(np.float32)
    gn = np.stack([R.gains(r) for r in w])
    x = g.standard_normal((rows, row_len)).astype(np.float32)
    x[-2, 0] = -0.0                                                # a free row's -0 ...
    x[-1] = x[-2]
    x[0, -1] = -0.0                                                # ... and a member's
    eta = g.standard_normal((rows, row_len)).astype(np.float32)
    k = np.tanh(g.standard_normal((rows, row_len))).astype(np.float32)
    y = R.average(k, members, w).astype(np.float32)
    t = np.zeros(rows, np.int64)
    for j in range(G):
        t[members[j][members[j] >= 0]] = (j + 1) % NTAB
    keys = np.stack([np.arange(rows) + 40, np.arange(rows) % 3], 1).astype(np.int64)
    keys[-1] = keys[-2]
    free = np.setdiff1d(np.arange(rows), members[members >= 0])
    for a in (members, w, gn, x, eta, y, t, keys):
        a.setflags(write=False)
    return dict(rows=rows, members=members, w=w, g=gn, x=x, eta=eta, y=y, t=t, keys=keys, free=free.tolist())


def _bits(t):
    return t.view(torch.int32)


@pytest.mark.parametrize('G', GROUPS)
@pytest.mark.parametrize('L', LS)
@pytest.mark.parametrize('row_len', ROW_LENS)
def test_constrain_with_injected_noise_against_the_restatement(row_len, L, G):
    from mudiff_hip import ops
    c = _case(row_len, L, G)
    a_tab, s_tab = _tables()
    x = _dev(c['x'])
    for clean in (False, True):
        got = ops.slab_constrain(x, _dev(c['y']), c['members'], c['w'], _dev(c['t']), 0, _dev(a_tab), _dev(s_tab), gains=c['g'], noise=_dev(c['eta']),
                                 clean=clean)
        args = (c['x'], c['y'], c['members'], c['w'], c['g'], c['eta'], c['t'], 0, a_tab, s_tab, clean)
        want, bound = R.constrain(*args), R.bound_out(*args)
        err = np.abs(got.cpu().numpy().astype(np.float64) - want)
        used = np.isfinite(bound)
        print(f'row_len {row_len} L {L} G {G} clean {clean}: worst |out - ref| / bound {np.max(err[used] / bound[used]):.3f}')
        assert (err[used] <= bound[used]).all()
        assert torch.equal(_bits(got[c['free']]), _bits(x[c['free']]))                   # free rows: x_new's bits, the -0 included
        assert np.signbit(got[-2, 0].item()) and got[-2, 0].item() == 0.0
        if clean:
            res = np.abs(R.average(got.cpu().numpy(), c['members'], c['w']) - c['y'].astype(np.float64))
            rb = R.bound_residual(c['x'], c['y'], c['members'], c['w'])
            print(f'row_len {row_len} L {L} G {G}: worst clean residual / bound {np.max(res / rb):.3f}')
            assert (res <= rb).all()
    assert torch.equal(_bits(x), _bits(_dev(c['x'])))                                    # the operand is not written


@pytest.mark.parametrize('G', GROUPS)
@pytest.mark.parametrize('L', LS)
@pytest.mark.parametrize('row_len', ROW_LENS)
def test_keyed_draw_in_place_and_independence_of_the_batch(row_len, L, G):
    from mudiff_hip import ops
    c = _case(row_len, L, G)
    a_tab, s_tab = (_dev(v) for v in _tables())
    x, y, t, keys = _dev(c['x']), _dev(c['y']), _dev(c['t']), _dev(c['keys'])
    step = 7
    kw = dict(gains=c['g'], keys=keys, seed=SEED, step=step)
    keyed = ops.slab_constrain(x, y, c['members'], c['w'], t, 0, a_tab, s_tab, **kw)
    eta = ops.randn_keyed(keys, row_len, SEED, step, ops.KIND_THICK)
    injected = ops.slab_constrain(x, y, c['members'], c['w'], t, 0, a_tab, s_tab, gains=c['g'], noise=eta)
    assert torch.equal(_bits(keyed), _bits(injected))                                    # the kernel draws what randn_keyed gives kind 6
    assert not torch.equal(keyed, ops.slab_constrain(x, y, c['members'], c['w'], t, 0, a_tab, s_tab, **dict(kw, step=8)))
    inplace = x.clone()
    assert ops.slab_constrain(inplace, y, c['members'], c['w'], t, 0, a_tab, s_tab, out=inplace, **kw) is inplace
    assert torch.equal(_bits(inplace), _bits(keyed))
    for clean in (False, True):
        whole = ops.slab_constrain(x, y, c['members'], c['w'], t, 0, a_tab, s_tab, clean=clean, **kw)
        for j in range(G):                                                               # a group alone, and with its rows in other places
            m = c['members'][j]
            n = int((m >= 0).sum())
            rows = torch.from_numpy(m[:n].astype(np.int64)).to(DEV)
            tab = np.full((1, L), -1, np.int32)
            tab[0, :n] = np.arange(n)
            one = dict(gains=c['g'][j:j + 1], keys=keys[rows], seed=SEED, step=step, clean=clean)
            alone = ops.slab_constrain(x[rows], y[j:j + 1], tab, c['w'][j:j + 1], t[rows], 0, a_tab, s_tab, **one)
            assert torch.equal(_bits(alone), _bits(whole[rows]))
            perm = torch.arange(n - 1, -1, -1, device=DEV)                               # reversed positions, the same table order
            tab[0, :n] = np.arange(n)[::-1]
            one['keys'] = keys[rows][perm]
            moved = ops.slab_constrain(x[rows][perm], y[j:j + 1], tab, c['w'][j:j + 1], t[rows][perm], 0, a_tab, s_tab, **one)
            assert torch.equal(_bits(moved[perm]), _bits(whole[rows]))


@pytest.mark.parametrize('row_len', ROW_LENS)
def test_one_member_against_known_constrain(row_len):
    """L = 1 with w = g = 1 replaces the row by q_sample(k): ops.known_constrain's result up to the projection's extra roundings,
    4 * 2^-24 (|x_new| + |a k| + |s eta|)."""
    from mudiff_hip import ops
    c = _case(row_len, 1, 3)
    a_tab, s_tab = _tables()
    x, eta, t = _dev(c['x']), _dev(c['eta']), _dev(c['t'])
    members = c['members']
    rows = torch.from_numpy(members[:, 0].astype(np.int64)).to(DEV)
    k = _dev(c['y'])                                                                     # w = 1: y is k
    for clean in (False, True):
        got = ops.slab_constrain(x, k, members, np.ones((3, 1), np.float32), t, 0, _dev(a_tab), _dev(s_tab), noise=eta, clean=clean)[rows]
        want = ops.known_constrain(x[rows], k, None, t[rows], 0, _dev(a_tab), _dev(s_tab), noise=eta[rows], clean=clean)
        a = a_tab[c['t'][members[:, 0]]][:, None].astype(np.float64)
        s = s_tab[c['t'][members[:, 0]]][:, None].astype(np.float64)
        xr, er = np.abs(c['x'][members[:, 0]]).astype(np.float64), np.abs(c['eta'][members[:, 0]]).astype(np.float64)
        bound = 4 * R.EPS * (xr + np.abs(c['y']) * (1.0 if clean else a) + (0.0 if clean else s * er))
        err = np.abs(got.cpu().numpy().astype(np.float64) - want.cpu().numpy())
        print(f'row_len {row_len} clean {clean}: worst |slab - known| / bound {np.max(err / bound):.3f}')
        assert (err <= bound).all()


@pytest.mark.parametrize('toff', (0, 1, -1))
def test_the_level_is_the_first_members_and_clamps(toff):
    from mudiff_hip import ops
    c = _case(33, 5, 3)
    a_tab, s_tab = _tables()
    t = np.array(c['t'])
    t[c['members'][0]] = NTAB - 1                                                        # + 1: clamped to the last entry
    t[c['members'][1]] = 0                                                               # - 1: clamped to the first
    t[c['members'][1][1:]] = 3                                                           # only the first member's level counts
    got = ops.slab_constrain(_dev(c['x']), _dev(c['y']), c['members'], c['w'], _dev(t), toff, _dev(a_tab), _dev(s_tab), gains=c['g'],
                             noise=_dev(c['eta']))
    args = (c['x'], c['y'], c['members'], c['w'], c['g'], c['eta'], t, toff, a_tab, s_tab, False)
    err, bound = np.abs(got.cpu().numpy().astype(np.float64) - R.constrain(*args)), R.bound_out(*args)
    used = np.isfinite(bound)
    assert (err[used] <= bound[used]).all()


@pytest.mark.parametrize('G', GROUPS)
@pytest.mark.parametrize('L', LS)
@pytest.mark.parametrize('row_len', ROW_LENS)
def test_slab_average_against_the_restatement(row_len, L, G):
    from mudiff_hip import ops
    c = _case(row_len, L, G)
    got = ops.slab_average(_dev(c['x']), c['members'], c['w'])
    assert got.shape == (G, row_len) and got.dtype == torch.float32
    want = R.average(c['x'], c['members'], c['w'])
    bound = (L + 4) * R.EPS * R.average(np.abs(c['x']), c['members'], c['w'])
    assert (np.abs(got.cpu().numpy().astype(np.float64) - want) <= bound).all()
    shaped = ops.slab_average(_dev(c['x']).view(c['rows'], 1, row_len), c['members'], c['w'])
    assert shaped.shape == (G, 1, row_len) and torch.equal(shaped.view(G, row_len), got)


def test_many_groups_take_more_than_one_launch():
    """40 groups of 4 rows: the tables travel as kernel arguments, 32 groups or 128 members a launch."""
    from mudiff_hip import ops
    g = np.random.default_rng(3)
    G, L, n = 40, 4, 36
    members = g.permutation(G * L).reshape(G, L).astype(np.int32)
    w = R.profile(L, 'gauss').astype(np.float32)
    x = g.standard_normal((G * L, n)).astype(np.float32)
    y = g.standard_normal((G, n)).astype(np.float32)
    got = ops.slab_constrain(_dev(x), _dev(y), members, w, None, 0, None, None, clean=True)
    args = (x, y, members, w, R.gains(w), None, None, 0, None, None, True)
    assert (np.abs(got.cpu().numpy().astype(np.float64) - R.constrain(*args)) <= R.bound_out(*args)).all()
    assert (np.abs(R.average(got.cpu().numpy(), members, w) - y) <= R.bound_residual(x, y, members, w)).all()
    avg = ops.slab_average(_dev(x), members, w)
    assert (np.abs(avg.cpu().numpy().astype(np.float64) - R.average(x, members, w)) <= (L + 4) * R.EPS * R.average(np.abs(x), members, w)).all()


def parent_bit_cases():
    """(name, output) of ops.slab_constrain and ops.slab_average over the row lengths of tests/parent_bits.py and L = 1, 5, 16 with three
    interleaved groups (free rows with a -0, an unused tail for L > 1): injected noise at toff -1 / 0 / +1 against first-member levels
    at both ends of the table, the keyed draw out of place and in place, `clean`, an operand 4 bytes off a 16-byte boundary; then one row
    alone, 33 groups of one member in 37 rows (two launches) and 9 groups of 16 (144 slots: the launch splits on slots)."""
    import parent_bits as P
    from mudiff_hip import ops
    at, st = (_dev(v) for v in _tables())
    for row_len in P.ROW_LENS:
        for L in (1, 5, 16):
            c = _case(row_len, L, 3)
            x, y, eta, keys = (_dev(c[n]) for n in ('x', 'y', 'eta', 'keys'))
            tab = dict(gains=c['g'])
            for toff in (-1, 0, 1):
                t = torch.full((c['rows'],), 2)
                t[c['members'][0][0]], t[c['members'][1][0]] = 0, NTAB - 1
                yield f'{row_len} L{L} noise toff {toff}', ops.slab_constrain(x, y, c['members'], c['w'], t.to(DEV), toff, at, st, noise=eta, **tab)
            t = _dev(c['t'])
            yield f'{row_len} L{L} keyed', ops.slab_constrain(x, y, c['members'], c['w'], t, 0, at, st, keys=keys, seed=SEED, step=7, **tab)
            xd = x.clone()
            yield f'{row_len} L{L} keyed in place', ops.slab_constrain(xd, y, c['members'], c['w'], t, 0, at, st, keys=keys, seed=SEED, step=7, out=xd, **tab)
            yield f'{row_len} L{L} clean', ops.slab_constrain(x, y, c['members'], c['w'], None, 0, None, None, clean=True, **tab)
            yield f'{row_len} L{L} average', ops.slab_average(x, c['members'], c['w'])
    c = _case(8, 5, 3)
    x, y, eta, t = P.off_by_one_float(_dev(c['x'])), _dev(c['y']), _dev(c['eta']), _dev(c['t'])
    assert x.is_contiguous() and x.data_ptr() % 16 == 4
    yield 'unaligned noise', ops.slab_constrain(x, y, c['members'], c['w'], t, 0, at, st, noise=eta, gains=c['g'])
    yield 'unaligned keyed', ops.slab_constrain(x, y, c['members'], c['w'], t, 0, at, st, keys=_dev(c['keys']), seed=SEED, step=7, gains=c['g'])
    yield 'unaligned average', ops.slab_average(x, c['members'], c['w'])
    g = np.random.default_rng(5)
    for name, rows, members in (('one row', 1, [[0]]), ('33 groups', 37, [[r] for r in range(36, 3, -1)]),
                                ('144 slots', 144, g.permutation(144).reshape(9, 16))):
        members = np.array(members, np.int32)
        w = R.profile(members.shape[1], 'gauss').astype(np.float32)
        x, eta = (_dev(g.standard_normal((rows, 33)).astype(np.float32)) for _ in range(2))
        y = _dev(g.standard_normal((len(members), 33)).astype(np.float32))
        t, keys = P.level_t(rows, 0).to(DEV), torch.stack([torch.arange(rows) + 2, torch.arange(rows) % 3], 1)
        yield f'{name} noise', ops.slab_constrain(x, y, members, w, t, 0, at, st, noise=eta)
        yield f'{name} keyed', ops.slab_constrain(x, y, members, w, t, 0, at, st, keys=keys, seed=SEED, step=1)
        yield f'{name} clean', ops.slab_constrain(x, y, members, w, None, 0, None, None, clean=True)
        yield f'{name} average', ops.slab_average(x, members, w)


def test_the_bits_are_those_of_the_parent_commit():
    import parent_bits as P
    P.check('test_thick_gpu', parent_bit_cases())


def test_bad_arguments_are_refused_before_a_launch():
    import mudiff_hip
    from mudiff_hip import MudiffHipError, ops
    lib = mudiff_hip.load()
    rows, n, L = 6, 8, 3
    f = dict(device=DEV, dtype=torch.float32)
    x, out, y, avg = torch.randn(rows, n, **f), torch.full((rows, n), 7.0, **f), torch.zeros(2, n, **f), torch.full((2, n), 7.0, **f)
    t, keys = torch.zeros(rows, device=DEV, dtype=torch.int64), torch.zeros(rows, 2, device=DEV, dtype=torch.int64)
    tab = torch.ones(NTAB, **f)
    p = lambda v: None if v is None else C.c_void_p(v.data_ptr())                        # noqa: E731
    h = lambda a: C.c_void_p(a.ctypes.data)                                              # noqa: E731
    good_m = np.array([[0, 2, 4], [1, 3, -1]], np.int32)
    good_w = np.full((2, 3), 0.25, np.float32)

    def call(m=good_m, w=good_w, g=good_w, L_=L, groups=2, kind=6, step=0, clean=0, x_=x, y_=y, keys_=keys, t_=t, rows_=rows, n_=n, out_=out):
        m, w, g = (np.ascontiguousarray(v) for v in (m, w, g))
        return lib.mud_slab_constrain(p(x_), p(y_), h(m), h(w), h(g), groups, L_, None, p(keys_), 0, step, kind, p(t_), 0, p(tab), p(tab), NTAB, clean,
                                      p(out_), rows_, n_, None)

    def edit(a, i, v):
        a = a.copy()
        a[i] = v
        return a

    assert call() == 0
    torch.cuda.synchronize()
    assert bool((out[5] == x[5]).all()) and not bool((out[0] == 7.0).any())              # (row 5 is free: copied)
    out.fill_(7.0)
    bad = [(dict(m=edit(good_m, (0, 1), 6)), b'members'), (dict(m=edit(good_m, (0, 1), -2)), b'members'),       # outside [0, rows)
           (dict(m=edit(good_m, (1, 0), 2)), b'members'), (dict(m=edit(good_m, (0, 1), 0)), b'members'),        # in two groups; twice in one
           (dict(m=edit(good_m, (1, slice(None)), -1)), b'members'),                                           # a group with no member
           (dict(w=edit(good_w, (0, 0), 0.0)), b'weights'), (dict(w=edit(good_w, (0, 0), -1.0)), b'weights'),
           (dict(w=edit(good_w, (1, 1), np.nan)), b'weights'), (dict(w=edit(good_w, (1, 1), np.inf)), b'weights'),
           (dict(g=edit(good_w, (0, 2), 0.0)), b'gains'), (dict(g=edit(good_w, (0, 2), np.nan)), b'gains'), (dict(g=edit(good_w, (0, 2), np.inf)), b'gains'),
           (dict(L_=0), b'L must'), (dict(L_=17), b'L must'), (dict(groups=-1), b'groups'), (dict(groups=7), b'groups'),
           (dict(rows_=1 << 20, n_=1 << 11), b'2^31'), (dict(kind=16), b'kind'), (dict(kind=-1), b'kind'), (dict(step=-1), b'step'),
           (dict(step=1 << 24), b'step'), (dict(x_=None), b'null'), (dict(out_=None), b'null'), (dict(y_=None), b'null'), (dict(t_=None), b'null'),
           (dict(keys_=None), b'keys'), (dict(rows_=0), b'bad sizes'), (dict(n_=0), b'bad sizes')]
    for kw, word in bad:
        assert call(**kw) == 1 and b'mud_slab_constrain' in lib.mud_last_error() and word in lib.mud_last_error(), (kw, lib.mud_last_error())
    assert lib.mud_slab_constrain(p(x), p(y), None, h(good_w), h(good_w), 2, L, None, p(keys), 0, 0, 6, p(t), 0, p(tab), p(tab), NTAB, 0, p(out), rows,
                                  n, None) == 1

    def average(m=good_m, w=good_w, L_=L, groups=2, x_=x, avg_=avg, rows_=rows):
        m, w = np.ascontiguousarray(m), np.ascontiguousarray(w)
        return lib.mud_slab_average(p(x_), h(m), h(w), groups, L_, p(avg_), rows_, n, None)

    for kw in (dict(m=edit(good_m, (0, 1), 6)), dict(m=edit(good_m, (1, 0), 2)), dict(w=edit(good_w, (0, 0), 0.0)), dict(L_=17), dict(groups=0),
               dict(x_=None), dict(avg_=None), dict(rows_=1 << 29)):
        assert average(**kw) == 1 and b'mud_slab_average' in lib.mud_last_error(), kw
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((avg == 7.0).all())                          # nothing was launched, nothing was copied
    assert lib.mud_randn_keyed(p(out), rows, n, p(keys), 0, 0, 3, None) == 1              # kinds 3 and 4 stay refused, 6 is taken
    assert lib.mud_randn_keyed(p(out), rows, n, p(keys), 0, 0, 6, None) == 0
    # the wrappers' own checks
    with pytest.raises(MudiffHipError):
        ops.slab_constrain(x, y[:1], good_m, good_w, None, 0, None, None, clean=True)     # one y for two groups
    with pytest.raises(MudiffHipError):
        ops.slab_constrain(x, y, good_m, good_w[:, :2], None, 0, None, None, clean=True)
    with pytest.raises(MudiffHipError):
        ops.slab_constrain(x, y, good_m, good_w, None, 0, None, None)                     # no t, no tables
    with pytest.raises(MudiffHipError):
        ops.slab_constrain(x, y, good_m, good_w, t, 0, tab, tab)                          # neither noise nor keys
    with pytest.raises(MudiffHipError, match='named twice'):
        ops.slab_constrain(x, y, edit(good_m, (1, 0), 2), good_w, None, 0, None, None, clean=True)
    with pytest.raises(MudiffHipError):
        ops.slab_average(x.cpu(), good_m, good_w)


def test_sample_keyed_takes_thick_and_stays_what_it_was_without():
    """GraphSampler.sample_keyed(thick=): the measured slab averages of the result are y under the residual rule, a slab alone equals
    the slab in its batch, thick is refused with known and with kspace, and without it the result is bit for bit the one of a sampler
    that never saw it.  In a child process with MUD_DETERMINISTIC=1 (read at import): every GroupNorm then reduces in a fixed order."""
    import os
    import subprocess
    import sys
    from conftest import PKG, REPO
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([REPO, PKG, os.path.join(REPO, 'tests'), os.environ.get('PYTHONPATH', '')]), MUD_DETERMINISTIC='1')
    c = subprocess.run([sys.executable, '-c', 'import test_thick_gpu as T; T.sampler_checks(); print("SAMPLER-OK")'], cwd=REPO, env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert c.returncode == 0 and 'SAMPLER-OK' in c.stdout, c.stdout[-3000:] + c.stderr[-3000:]


def sampler_checks():
    """The body of test_sample_keyed_takes_thick_and_stays_what_it_was_without (run in its child process)."""
    import volume_support as VS
    from oracle import mudiff_oracle as O
    from backbones.ncsnpp_generator_adagn_feat import NCSNpp, NCSNpp_adaptive
    from mudiff_hip import ops, sampling as Sm
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
    w = R.profile(L, 'gauss').astype(np.float32)
    y = R.average(k, members, w).astype(np.float32)
    keys = torch.tensor([[4 + r, r % 2] for r in range(B)])
    before = sampler.sample_keyed(*conds, keys, 31, T)
    thick = (_dev(y), members, w, None)
    out = sampler.sample_keyed(*conds, keys, 31, T, thick=thick)
    x_new = sampler.thick_x_new.clone()                                                  # what the last reverse step gave the constraint
    assert not torch.equal(out, before)
    assert torch.equal(out[3], x_new[3])                                                 # the free row: copied
    flat = lambda v: v[:, 0].reshape(B, -1).cpu().numpy()                                # noqa: E731
    res = np.abs(R.average(flat(out), members, w) - y.reshape(2, -1))
    rb = R.bound_residual(flat(x_new), y.reshape(2, -1), members, w)
    print(f'sampler: worst clean residual / bound {np.max(res / rb):.3f}')
    assert (res <= rb).all()
    again = sampler.sample_keyed(*conds, keys, 31, T, thick=thick, coupling='shared', resample=2)
    assert torch.isfinite(again).all()
    res = np.abs(R.average(flat(again), members, w) - y.reshape(2, -1))
    assert (res <= R.bound_residual(flat(sampler.thick_x_new), y.reshape(2, -1), members, w)).all()
    assert torch.equal(sampler.sample_keyed(*conds, keys, 31, T), before)                # without thick: what it was
    assert torch.equal(sampler.sample_keyed(*conds, keys, 31, T, thick=(_dev(y[:0]), members[:0], w, None)), before)      # no group: free
    # a slab alone (the rest of the batch: padding in no group) equals the slab in its batch
    rows = [4, 5, 6, 6, 6, 6, 6]
    alone = sampler.sample_keyed(*[c[rows] for c in conds], keys[rows], 31, T, thick=(_dev(y[1:]), np.array([[0, 1, 2]], np.int32), w, None))
    assert torch.equal(alone[:3], out[4:7])

    class Object:                                                                        # an object with the attributes serves as the tuple does
        pass
    o = Object()
    o.y, o.members, o.weights, o.gains = _dev(y), members, w, ops.slab_gains(w)[0]
    assert torch.equal(sampler.sample_keyed(*conds, keys, 31, T, thick=o), out)
    zeros = torch.zeros(B, 1, S, S, device=DEV)
    with pytest.raises(ValueError, match='exclusive'):
        sampler.sample_keyed(*conds, keys, 31, T, thick=thick, known=zeros, known_mask=zeros.to(torch.uint8))
    with pytest.raises(ValueError, match='exclusive'):
        sampler.sample_keyed(*conds, keys, 31, T, thick=thick, kspace=(torch.zeros(B, S, S, device=DEV, dtype=torch.complex64),
                                                                       torch.zeros(1, S, S, device=DEV, dtype=torch.uint8)))
    with pytest.raises(ValueError, match='thick'):
        sampler.sample_keyed(*conds, keys, 31, T, thick=(_dev(y)[:1], members, w, None))
    with pytest.raises(ValueError, match='thick'):
        sampler.sample_keyed(*conds, keys, 31, T, thick=(_dev(y), members + 3, w, None))      # a row outside the batch
    # an ensemble: a chunk ends before a slab it would cut, and the samples do not depend on the chunks
    from mudiff_hip import ensemble as E, thick as TK
    n, starts = 8, [1, 5]
    c8 = [_dev(np.tanh(g.standard_normal((n, 1, S, S))).astype(np.float32)) for _ in range(3)]
    y8 = ops.slab_average(_dev(np.tanh(g.standard_normal((n, S, S))).astype(np.float32)), [[1, 2, 3], [5, 6, 7]], w)
    meas = lambda: TK.ThickMeasurement(y8, starts, n, w, dict(slabs=[]), 1, dict(interp=False))      # noqa: E731
    m1, m2 = meas(), meas()
    whole = E.sample_ensemble(cfg, g1, g2, c8, 2, 31, sampler=sampler, thick=m1, return_samples=True)
    cut = E.sample_ensemble(cfg, g1, g2, c8, 2, 31, sampler=sampler, thick=m2, return_samples=True, chunk=3)      # chunks 0, 1..3, 4, 5..7
    assert all(torch.equal(a_, b_) for a_, b_ in zip(whole, cut)) and torch.equal(m1.residual, m2.residual) and bool((m1.y_norm > 0).all())
    assert bool((m1.residual * m1.y_norm <= 3 * (L + 4) * R.EPS * (m1.x_norm + m1.y_norm)).all())
    assert not torch.equal(whole[2], E.sample_ensemble(cfg, g1, g2, c8, 2, 31, sampler=sampler, return_samples=True)[2])
    with pytest.raises(ValueError, match='chunk'):
        E.sample_ensemble(cfg, g1, g2, c8, 2, 31, sampler=sampler, thick=meas(), chunk=2)
