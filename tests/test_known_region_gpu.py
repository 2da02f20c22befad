"""GPU: sampling with a partly acquired target (csrc/known_region.hip: mud_known_constrain, mud_known_coverage; ops.known_constrain,
ops.known_coverage; GraphSampler.sample_keyed's known / known_mask / resample) against the numpy restatement in
tests/known_region_ref.py.  DESIGN.md section 5.25."""
import json
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest
import torch

from conftest import PKG, REPO
import known_region_ref as R
import volume_support as VS

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ROWS = (1, 5, 37)
ROW_LENS = (4, 10, 100, 4099)      # one whole block; a ragged tail; whole blocks; a ragged tail over more than one workgroup per row
NTAB = 5


def _tables():
    a = np.array([0.99999994, 0.97, 0.81, 0.5, 0.12], np.float32)
    return a, np.sqrt(1 - a.astype(np.float64) ** 2).astype(np.float32)


def _case(rows, row_len, seed=0):
    g = np.random.default_rng(1000 * rows + row_len + seed)
    x = g.standard_normal((rows, row_len)).astype(np.float32)
    k = np.tanh(g.standard_normal((rows, row_len))).astype(np.float32)
    m = (g.random((rows, row_len)) < 0.5).astype(np.uint8)
    eta = g.standard_normal((rows, row_len)).astype(np.float32)
    t = g.integers(-2, NTAB + 2, rows).astype(np.int64)       # per-row levels, the clamped ends included
    if rows >= 2:
        t[0], t[-1] = -1, NTAB + 1
    return x, k, m, eta, t


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize('row_len', ROW_LENS)
@pytest.mark.parametrize('rows', ROWS)
def test_constrain_with_injected_noise_is_the_restatement_bit_for_bit(rows, row_len):
    from mudiff_hip import ops
    a_tab, s_tab = _tables()
    x, k, m, eta, t = _case(rows, row_len)
    at, st = _dev(a_tab), _dev(s_tab)
    for toff in (0, 1):
        for clean in (False, True):
            want = R.constrain(x, k, m, eta, t, toff, a_tab, s_tab, clean)
            got = ops.known_constrain(_dev(x), _dev(k), _dev(m), _dev(t), toff, at, st, noise=_dev(eta), clean=clean).cpu().numpy()
            assert np.array_equal(_bits(got), _bits(want)), (rows, row_len, toff, clean)
            # an out view offset by one float: the element-by-element path, and nothing written outside it
            big = torch.full((rows * row_len + 2,), 7.0, device=DEV)
            out = big[1:-1].view(rows, row_len)
            ops.known_constrain(_dev(x), _dev(k), _dev(m), _dev(t), toff, at, st, noise=_dev(eta), clean=clean, out=out)
            assert np.array_equal(_bits(out.cpu().numpy()), _bits(want))
            assert float(big[0]) == 7.0 and float(big[-1]) == 7.0
            # in place on x_new
            xd = _dev(x)
            assert ops.known_constrain(xd, _dev(k), _dev(m), _dev(t), toff, at, st, noise=_dev(eta), clean=clean, out=xd) is xd
            assert np.array_equal(_bits(xd.cpu().numpy()), _bits(want))
    # the known part is ops.q_sample's arithmetic
    q = ops.q_sample(_dev(k), _dev(eta), _dev(t), 1, at, st).cpu().numpy()
    got = ops.known_constrain(_dev(x), _dev(k), _dev(m), _dev(t), 1, at, st, noise=_dev(eta)).cpu().numpy()
    assert np.array_equal(_bits(got)[m != 0], _bits(q)[m != 0])
    # mask all 0: x_new's bits; mask all 1 and clean: known's bits
    zero, one = np.zeros_like(m), np.ones_like(m)
    got = ops.known_constrain(_dev(x), _dev(k), _dev(zero), _dev(t), 0, at, st, noise=_dev(eta)).cpu().numpy()
    assert np.array_equal(_bits(got), _bits(x))
    got = ops.known_constrain(_dev(x), _dev(k), _dev(one), _dev(t), 0, at, st, noise=_dev(eta), clean=True).cpu().numpy()
    assert np.array_equal(_bits(got), _bits(k))
    # a select, not a blend: NaN / inf of `known` outside the mask never reach out
    for poison in (np.nan, np.inf, -np.inf):
        kp = np.where(m != 0, k, np.float32(poison)).astype(np.float32)
        for clean in (False, True):
            got = ops.known_constrain(_dev(x), _dev(kp), _dev(m), _dev(t), 0, at, st, noise=_dev(eta), clean=clean).cpu().numpy()
            assert np.isfinite(got).all() and np.array_equal(_bits(got)[m == 0], _bits(x)[m == 0])
            assert np.array_equal(_bits(got), _bits(R.constrain(x, k, m, eta, t, 0, a_tab, s_tab, clean)))


@pytest.mark.parametrize('rows,row_len', [(5, 4), (37, 10), (5, 100), (1, 4099)])
def test_constrain_with_keyed_noise(rows, row_len):
    from mudiff_hip import ops
    a_tab, s_tab = _tables()
    x, k, m, _, t = _case(rows, row_len, seed=1)
    at, st = _dev(a_tab), _dev(s_tab)
    g = np.random.default_rng(rows)
    keys = np.stack([g.integers(0, 200, rows), g.integers(0, 16, rows)], 1).astype(np.int64)
    seed, step = 2024, 3
    # kind 2: the draw of ops.randn_keyed, bit for bit
    eta2 = ops.randn_keyed(torch.from_numpy(keys), row_len, seed, step, ops.KIND_NOISE).to(DEV)
    want = ops.known_constrain(_dev(x), _dev(k), _dev(m), _dev(t), 0, at, st, noise=eta2)
    got = ops.known_constrain(_dev(x), _dev(k), _dev(m), _dev(t), 0, at, st, keys=keys, seed=seed, step=step, kind=ops.KIND_NOISE)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    # kind 3 against the restatement: a one-ulp difference of eta carried through (the <= 1 ulp tests/test_ensemble_gpu.py allows)
    assert ops.KIND_KNOWN == R.KIND_KNOWN == 3 and ops.KIND_RENOISE == R.KIND_RENOISE == 4
    eta = R.keyed_eta(keys, row_len, seed, step, R.KIND_KNOWN)
    want = R.constrain(x, k, m, eta, t, 0, a_tab, s_tab)
    got = ops.known_constrain(_dev(x), _dev(k), _dev(m), _dev(t), 0, at, st, keys=keys, seed=seed, step=step, kind=ops.KIND_KNOWN).cpu().numpy()
    c = np.clip(t, 0, NTAB - 1)
    bound = np.abs(s_tab[c]).reshape(rows, 1).astype(np.float64) * np.spacing(np.abs(eta)).astype(np.float64) + np.spacing(np.abs(want)).astype(np.float64)
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    print(f'rows {rows} row_len {row_len}: max err / bound {float((err / bound).max()):.3f}, differing {int((got != want).sum())} of {got.size}')
    assert (err <= bound).all()
    assert np.array_equal(_bits(got)[m == 0], _bits(x)[m == 0])
    other = ops.known_constrain(_dev(x), _dev(k), _dev(m), _dev(t), 0, at, st, keys=keys, seed=seed, step=step, kind=ops.KIND_RENOISE).cpu().numpy()
    assert (other != got)[m != 0].any()                        # another kind is another draw
    # the mask == NULL form equals the all-ones mask (and needs no x_new)
    one = np.ones_like(m)
    full = ops.known_constrain(_dev(x), _dev(k), _dev(one), _dev(t), 1, at, st, keys=keys, seed=seed, step=step, kind=ops.KIND_RENOISE)
    none = ops.known_constrain(None, _dev(k), None, _dev(t), 1, at, st, keys=keys, seed=seed, step=step, kind=ops.KIND_RENOISE)
    assert torch.equal(full.view(torch.int32), none.view(torch.int32))
    kd = _dev(k)                                               # ... in place on `known`: the sampler's re-noising
    ops.known_constrain(None, kd, None, _dev(t), 1, at, st, keys=keys, seed=seed, step=step, kind=ops.KIND_RENOISE, out=kd)
    assert torch.equal(kd.view(torch.int32), none.view(torch.int32))


def test_constrain_does_not_depend_on_row_order_or_batching():
    from mudiff_hip import ops
    rows, row_len = 37, 100
    a_tab, s_tab = _tables()
    x, k, m, _, t = _case(rows, row_len, seed=2)
    at, st = _dev(a_tab), _dev(s_tab)
    g = torch.Generator().manual_seed(3)
    keys = torch.stack([torch.randint(0, 200, (rows,), generator=g), torch.randint(0, 16, (rows,), generator=g)], 1)
    run = lambda idx: ops.known_constrain(_dev(x[idx]), _dev(k[idx]), _dev(m[idx]), _dev(t[idx]), 0, at, st, keys=keys[idx], seed=11, step=2)      # noqa: E731
    full = run(np.arange(rows))
    perm = torch.randperm(rows, generator=g).numpy()
    assert torch.equal(run(perm), full[torch.from_numpy(perm).to(DEV)])
    parts = [run(np.arange(a, b)) for a, b in ((0, 5), (5, 6), (6, 30), (30, 37))]
    assert torch.equal(torch.cat(parts, 0), full)


def test_constrain_refuses_bad_arguments():
    from mudiff_hip import MudiffHipError, ops
    a_tab, s_tab = _tables()
    x, k, m, eta, t = (_dev(v) for v in _case(2, 8))
    at, st = _dev(a_tab), _dev(s_tab)
    with pytest.raises(MudiffHipError, match='noise or keys'):
        ops.known_constrain(x, k, m, t, 0, at, st)
    with pytest.raises(MudiffHipError, match='x_new'):
        ops.known_constrain(None, k, m, t, 0, at, st, noise=eta)
    with pytest.raises(MudiffHipError, match='mask'):
        ops.known_constrain(x, k, m.float(), t, 0, at, st, noise=eta)
    for bad in (dict(kind=16), dict(kind=-1), dict(step=-1), dict(step=1 << 24)):
        with pytest.raises(MudiffHipError):
            ops.known_constrain(x, k, m, t, 0, at, st, keys=[[0, 0], [1, 0]], seed=1, **bad)
    with pytest.raises(MudiffHipError):                                               # mud_randn_keyed itself keeps to kinds 0..2
        ops.randn_keyed(torch.tensor([[0, 0]]), 8, 1, 0, ops.KIND_KNOWN)


def parent_bit_cases():
    """(name, output) of ops.known_constrain over the shapes and paths of tests/parent_bits.py: every row length and row count with
    injected noise, the keyed draw and `clean`, out of place and in place, toff -1 / 0 / +1 against levels at both ends of the table;
    then the unaligned form, no mask, a quad with nothing known beside a mixed one, and `out is known`."""
    import parent_bits as P
    from mudiff_hip import ops
    at, st = (_dev(v) for v in _tables())
    for rows in P.ROWS:
        keys = torch.stack([torch.arange(rows) * 3 + 1, torch.arange(rows) % 4], 1)
        for row_len in P.ROW_LENS:
            x, k, m, eta, _ = (_dev(v) for v in _case(rows, row_len))
            draws = dict(noise=dict(noise=eta), keyed=dict(keys=keys, seed=2024, step=3), clean=dict(clean=True))
            for mode, kw in draws.items():
                for toff in ((0,) if mode == 'clean' else (-1, 0, 1)):
                    t = P.level_t(rows, toff).to(DEV)
                    yield f'{rows}x{row_len} {mode} toff {toff}', ops.known_constrain(x, k, m, t, toff, at, st, **kw)
                xd = x.clone()
                yield f'{rows}x{row_len} {mode} in place', ops.known_constrain(xd, k, m, P.level_t(rows, 0).to(DEV), 0, at, st, out=xd, **kw)
    rows, row_len = 5, 8
    x, k, m, eta, _ = (_dev(v) for v in _case(rows, row_len))
    t, keys = P.level_t(rows, 0).to(DEV), torch.stack([torch.arange(rows) + 7, torch.arange(rows) % 2], 1)
    for mode, kw in dict(noise=dict(noise=eta), keyed=dict(keys=keys, seed=9, step=1), clean=dict(clean=True)).items():
        ku = P.off_by_one_float(k)
        assert ku.is_contiguous() and ku.data_ptr() % 16 == 4
        yield f'unaligned known {mode}', ops.known_constrain(x, ku, m, t, 0, at, st, **kw)
        yield f'unaligned out {mode}', ops.known_constrain(x, k, m, t, 0, at, st, out=P.off_by_one_float(x), **kw)
        yield f'no mask {mode}', ops.known_constrain(None, k, None, t, 1, at, st, **kw)
        quads = m.clone()
        quads[:, :4] = 0
        quads[:, 4:] = torch.tensor([1, 0, 0, 1], dtype=torch.uint8)
        yield f'empty quad {mode}', ops.known_constrain(x, k, quads, t, 0, at, st, **kw)
        kd = k.clone()
        yield f'out is known {mode}', ops.known_constrain(x, kd, m, t, 0, at, st, out=kd, **kw)


def test_the_bits_are_those_of_the_parent_commit():
    import parent_bits as P
    P.check('test_known_region_gpu', parent_bit_cases())


# ---------------------------------------------------------------------------------------------------
SRC, DST = (7, 9, 11), (8, 8, 8)
DYADIC = {
    'identity': np.eye(4)[:3],
    'half_x': np.array([[1, 0, 0, 0.5], [0, 1, 0, 0], [0, 0, 1, 0]], np.float64),
    'half_all_negative': np.array([[1, 0, 0, -0.5], [0, 1, 0, 0.5], [0, 0, 1, -0.5]], np.float64),
    'scale_2': np.array([[2, 0, 0, 0], [0, 2, 0, 0], [0, 0, 2, 0]], np.float64),
    'scale_half': np.array([[0.5, 0, 0, 0.25], [0, 0.5, 0, 3], [0, 0, 0.5, 7.5]], np.float64),
    'permute_flip': np.array([[0, 0, -1, 6], [1, 0, 0, 0], [0, 1, 0, 2]], np.float64),
}
OBLIQUE = np.array([[0.9130, -0.2710, 0.1170, 0.3137], [0.2390, 1.0310, -0.0930, 0.6173], [-0.1510, 0.0870, 1.2070, 0.4391]], np.float64)


@pytest.mark.parametrize('name', sorted(DYADIC))
def test_coverage_of_dyadic_matrices_is_the_restatement(name):
    from mudiff_hip import ops
    want = R.coverage(DYADIC[name], SRC, DST)
    got = VS.to_host_xyz(ops.known_coverage(DYADIC[name], SRC, DST, DEV))
    assert got.dtype == np.uint8 and np.array_equal(got, want), name
    assert 0 < int(want.sum()) <= want.size
    if name == 'identity':
        assert int(want.sum()) == 7 * 8 * 8                  # the destination's x runs one past the source's 7 planes


def test_coverage_of_an_oblique_matrix():
    from mudiff_hip import ops
    near = R.near_a_bound(OBLIQUE, SRC, DST)
    assert not near.any()                                    # (the matrix was chosen so: no voxel where a last-bit difference could decide)
    want = R.coverage(OBLIQUE, SRC, DST)
    got = VS.to_host_xyz(ops.known_coverage(np.vstack([OBLIQUE, [0, 0, 0, 1]]), SRC, DST, DEV))
    assert np.array_equal(got[~near], want[~near]) and 0 < int(want.sum()) < want.size


# ---------------------------------------------------------------------------------------------------
def _child(code, timeout=900):
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([REPO, PKG, os.path.join(REPO, 'tests'), os.environ.get('PYTHONPATH', '')]),
               MUD_DETERMINISTIC='1')
    for k in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE'):
        env.pop(k, None)
    p = subprocess.run([sys.executable, '-c', textwrap.dedent(code)], cwd=REPO, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=timeout)
    assert p.returncode == 0, p.stderr[-3000:]
    return p.stdout


@pytest.fixture(scope='module')
def sampler_runs():
    """sample_keyed on the tiny seeded model, B = 6, MUD_DETERMINISTIC=1: every call of the sampler tests in one child process."""
    out = _child(f'''
        import json, torch
        from oracle import mudiff_oracle as O
        from backbones.ncsnpp_generator_adagn_feat import NCSNpp, NCSNpp_adaptive
        from mudiff_hip import sampling as S
        cfg = O.default_config(**{VS.TINY_MODEL!r})
        g1, g2 = NCSNpp(cfg), NCSNpp_adaptive(cfg)
        g1.load_state_dict(O.make_state_dict(cfg, 'g1', 9)); g2.load_state_dict(O.make_state_dict(cfg, 'g2', 9))
        g1, g2 = g1.cuda().eval(), g2.cuda().eval()
        B, size, T = 6, cfg.image_size, cfg.num_timesteps
        g = torch.Generator().manual_seed(4)
        conds = [torch.tanh(torch.randn(B, 1, size, size, generator=g)).cuda() for _ in range(3)]
        known = torch.tanh(torch.randn(B, 1, size, size, generator=g)).cuda()
        half = torch.zeros(B, 1, size, size, dtype=torch.uint8, device='cuda')
        half[:, :, :, : size // 2] = 1
        half[0] = 0; half[1] = 1                                  # a row with nothing known and one with everything known
        zero = torch.zeros_like(half)
        sampler = S.GraphSampler(S.Posterior_Coefficients(cfg, 'cuda:0'), g1, g2, cfg, B, size, size, 'cuda:0')
        keys = torch.stack([torch.arange(B) + 3, torch.zeros(B, dtype=torch.int64)], 1)
        run = lambda **kw: sampler.sample_keyed(*conds, keys, 31, T, **kw)
        plain = run()
        none = run(known=known, known_mask=zero)
        a = run(known=known, known_mask=half)
        b = run(known=known, known_mask=half)
        r1 = run(known=known, known_mask=half, resample=1)
        r2 = run(known=known, known_mask=half, resample=2)
        r2b = run(known=known, known_mask=half, resample=2)
        poisoned = run(known=torch.where(half.bool(), known, torch.full_like(known, float('nan'))), known_mask=half)
        m, f = half.bool(), ~half.bool()
        bits = lambda x: x.view(torch.int32)
        refused = []
        for kw in (dict(known_mask=half), dict(resample=2), dict(known=known), dict(known=known, known_mask=half, resample=0),
                   dict(known=known[:, :, :4], known_mask=half), dict(known=known, known_mask=half.float())):
            try:
                run(**kw)
                refused.append(False)
            except ValueError:
                refused.append(True)
        print(json.dumps(dict(
            T=T, zero_mask_is_plain=bool(torch.equal(bits(none), bits(plain))), again=bool(torch.equal(bits(a), bits(b))),
            known_exact=bool(torch.equal(bits(a)[m], bits(known)[m])), free_changed=float((a - plain)[f].abs().max()),
            free_row_unchanged=bool(torch.equal(bits(a[0]), bits(plain[0]))), r1_is_default=bool(torch.equal(bits(r1), bits(a))),
            r2_finite=bool(torch.isfinite(r2).all()), r2_known_exact=bool(torch.equal(bits(r2)[m], bits(known)[m])),
            r2_differs=float((r2 - a)[f].abs().max()), r2_again=bool(torch.equal(bits(r2), bits(r2b))),
            poisoned_same=bool(torch.equal(bits(poisoned), bits(a))), finite=bool(torch.isfinite(a).all()), refused=refused,
            plain_after=bool(torch.equal(bits(run()), bits(plain))))))
    ''')
    return json.loads(out.strip().splitlines()[-1])


def test_sampler_keeps_the_known_voxels_bit_for_bit(sampler_runs):
    r = sampler_runs
    assert r['finite'] and r['known_exact'] and r['again']
    assert r['poisoned_same']                                 # what `known` holds outside the mask does not matter


def test_sampler_without_a_known_region_is_unchanged(sampler_runs):
    r = sampler_runs
    assert r['zero_mask_is_plain'] and r['plain_after'] and r['r1_is_default']
    assert r['free_row_unchanged']                            # a row with an all-zero mask, next to constrained ones


def test_sampler_conditions_the_free_region(sampler_runs):
    r = sampler_runs
    print(f"free region: max |constrained - plain| {r['free_changed']:.4f}; resample 2 vs 1 {r['r2_differs']:.4f}")
    assert r['T'] >= 2 and r['free_changed'] > 0


def test_sampler_resampling(sampler_runs):
    r = sampler_runs
    assert r['r2_finite'] and r['r2_known_exact'] and r['r2_again'] and r['r2_differs'] > 0


def test_sampler_refuses_bad_arguments(sampler_runs):
    assert sampler_runs['refused'] == [True] * 6


# ---------------------------------------------------------------------------------------------------
TOL = 5e-5                                                   # tests/test_slice_coupling_gpu.py: the same volume at two batch sizes
DROP = ['--known_drop_slices', '3:5']


def _phantom(shape, i):
    x, y, z = np.meshgrid(*(np.arange(float(n)) for n in shape), indexing='ij')
    return (120 + 60 * np.sin(x / (3 + i) + 0.3 * z) * np.cos(y / (4.5 - i) - 0.2 * z) + 4 * z).astype(np.float32)


def _k01(values):
    """to_range_0_1(normalise_volume(K)) as float32, on the host: the product with 0.5 is exact, the sum rounds once."""
    from mudiff_hip import volume as V
    k = np.asarray(V.normalise_volume(np.asarray(values, np.float64)), np.float32)
    return np.clip(k * np.float32(0.5) + np.float32(0.5), np.float32(0), np.float32(1))


@pytest.fixture(scope='module')
def runs(tmp_path_factory):
    """16 x 16 x 9 inputs and a fourth synthetic volume K, the tiny model, every run in one child process."""
    from mudiff_hip import volume as V
    tmp = tmp_path_factory.mktemp('known')
    VS.write_tiny_model(tmp)
    p, small = ({k: str(tmp / f'{k}{tag}.nii.gz') for k in ('flair', 't2', 't1', 'K')} for tag in ('', '_12'))
    for i, k in enumerate(p):
        V.write_nifti(p[k], _phantom((16, 16, 9), i), np.eye(4))
        V.write_nifti(small[k], _phantom((12, 12, 9), i), np.eye(4))
    trust = np.zeros((16, 16, 9), np.float32)
    trust[:8, 2:, 1:] = 1
    p['M'] = str(tmp / 'M.nii.gz')
    V.write_nifti(p['M'], trust, np.eye(4))
    shifted = np.eye(4)
    shifted[2, 3] = 2.5                                       # K5's plane k lies at z = k + 2.5 of the inputs' grid
    p['K5'] = str(tmp / 'K5.nii.gz')
    V.write_nifti(p['K5'], _phantom((16, 16, 5), 3), shifted)
    inputs = lambda q: ['--input_flair', q['flair'], '--input_t2', q['t2'], '--input_t1', q['t1']]      # noqa: E731
    known = ['--known_volume', p['K']]
    jobs = {'plain': (4, inputs(p)), 'known': (4, inputs(p) + known + DROP), 'known_b9': (9, inputs(p) + known + DROP),
            'known_dev': (4, inputs(p) + known + DROP + ['--device_intake']), 'mask': (4, inputs(p) + known + ['--known_mask', p['M'], '--gt_volume', p['K']]),
            'ens': (4, inputs(p) + known + DROP + ['--num_samples', '2']), 'gt': (4, inputs(p) + known + ['--gt_volume', p['K']]),
            'regrid': (4, inputs(p) + ['--known_volume', p['K5'], '--regrid']),
            'rb': (4, inputs(small) + ['--known_volume', small['K'], '--resize_back'] + DROP), 'r2': (4, inputs(p) + known + DROP + ['--known_resample', '2'])}
    steps = [VS.volume_step(k, VS.model_argv(tmp, 4, b) + a + ['--output_dir', str(tmp / k)]) for k, (b, a) in jobs.items()]
    manifest = tmp / 'cohort.tsv'
    manifest.write_text('id\tt1\tt1ce\tt2\tflair\tknown\ns0\t' + '\t'.join([p['t1'], '', p['t2'], p['flair'], p['K']]) + '\n')
    steps.append(VS.cohort_step('cohort', VS.model_argv(tmp, 4, 4) + DROP + ['--manifest', str(manifest), '--output_dir', str(tmp / 'cohort')]))
    log = VS.run_plan(tmp, steps, 900, ignore='RuntimeWarning')
    vol = lambda path: V.read_nifti(str(path))[0]             # noqa: E731
    return dict(tmp=tmp, log=log, p=p, small=small, shifted=shifted, vol=vol, trust=trust,
                pred=lambda k, suffix='': vol(tmp / k / f'predicted_t1ce{suffix}.nii.gz'),
                bytes=lambda k: VS.payload(str(tmp / k / 'predicted_t1ce.nii.gz')), report=lambda k: json.load(open(tmp / k / 'known_t1ce.json')))


def _dropped_mask(shape=(16, 16, 9)):
    m = np.ones(shape, bool)
    m[:, :, 3:6] = False
    return m


def test_written_volume_carries_the_known_voxels_exactly(runs):
    k01, known = _k01(runs['vol'](runs['p']['K'])), _dropped_mask()
    for job in ('known', 'known_b9', 'known_dev', 'r2'):
        pred = runs['pred'](job).astype(np.float32)
        assert pred.shape == (16, 16, 9) and np.isfinite(pred).all()
        assert np.array_equal(pred[known], k01[known]), job
        assert pred[~known].any() and (pred[~known] != k01[~known]).any(), job      # the dropped slices are synthesised
        rep = runs['report'](job)
        assert rep['known_voxels'] == int(known.sum()) == 6 * 256 and rep['slab'] == [0, 8] and rep['drop_slices'] == [[3, 5]]
        assert rep['known_per_slice'] == [256, 256, 256, 0, 0, 0, 256, 256, 256] and rep['fraction_of_slab'] == 6 / 9
        assert rep['terms'] == dict(coverage=2304, finite=2304, not_dropped=1536, slab=2304) and rep['resample'] == (2 if job == 'r2' else 1)
    assert (runs['pred']('known')[~known] != runs['pred']('plain')[~known]).any()          # conditioned on the known part
    assert (runs['pred']('r2')[~known] != runs['pred']('known')[~known]).any()


def test_resize_back_carries_the_known_voxels_exactly(runs):
    k01, known = _k01(runs['vol'](runs['small']['K'])), _dropped_mask((12, 12, 9))
    pred = runs['pred']('rb').astype(np.float32)
    assert pred.shape == (12, 12, 9) and np.array_equal(pred[known], k01[known])
    assert pred[~known].any() and (pred[~known] != k01[~known]).any()
    assert runs['report']('rb')['known_voxels'] == 6 * 144


def test_batch_size_intake_and_cohort_do_not_matter(runs):
    a, b = runs['pred']('known'), runs['pred']('known_b9')
    worst = float(np.abs(a - b).max())
    print(f'batch 4 vs batch 9: max |difference| {worst:.3e}')
    assert worst <= TOL and a.any()
    assert runs['bytes']('known') == runs['bytes']('known_dev') == VS.payload(str(runs['tmp'] / 'cohort' / 's0' / 'predicted_t1ce.nii.gz'))
    assert json.load(open(runs['tmp'] / 'cohort' / 's0' / 'known_t1ce.json')) == runs['report']('known')


def test_done_lines_and_files(runs):
    tmp, log = runs['tmp'], runs['log']
    for job in ('known', 'known_b9', 'known_dev', 'cohort'):
        assert VS.done_line(log[job]).endswith(' | known=0.667'), VS.done_line(log[job])
    assert VS.done_line(log['r2']).endswith(' | known=0.667 x2')
    assert VS.done_line(log['ens']).endswith(' | 2 samples per slice | known=0.667')
    assert VS.done_line(log['gt']).endswith(' | known=1.000') and VS.done_line(log['rb']).endswith(' | known=0.667')
    assert ' | known=' not in VS.done_line(log['plain']) and VS.done_line(log['plain']).endswith('slices=0..8')
    assert sorted(os.listdir(tmp / 'plain')) == ['predicted_t1ce.nii.gz']
    assert sorted(os.listdir(tmp / 'known')) == ['known_t1ce.json', 'predicted_t1ce.nii.gz']


def test_mask_file_and_scores(runs):
    k01 = _k01(runs['vol'](runs['p']['K']))
    known = runs['trust'] != 0
    pred = runs['pred']('mask').astype(np.float32)
    assert np.array_equal(pred[known], k01[known]) and (pred[~known] != k01[~known]).any()
    rep = runs['report']('mask')
    assert rep['terms']['mask'] == int(known.sum()) == rep['known_voxels'] == 8 * 14 * 8
    for job, n_known in (('mask', int(known.sum())), ('gt', 2304)):
        m = json.load(open(runs['tmp'] / job / 'metrics_t1ce.json'))
        assert m['regions'] == ['slab', 'brain', 'known', 'synthesised']
        assert m['metrics']['known']['voxels'] == n_known and m['metrics']['known']['voxels'] + m['metrics']['synthesised']['voxels'] == 2304
        assert m['metrics']['known']['mae'] == 0.0 and m['metrics']['known']['sse'] == 0.0
        assert sum(ln.startswith('[metrics] known:') for ln in runs['log'][job].splitlines()) == 1
        assert sum(ln.startswith('[metrics] synthesised:') for ln in runs['log'][job].splitlines()) == 1
    m = json.load(open(runs['tmp'] / 'gt' / 'metrics_t1ce.json'))['metrics']
    # everything known: prediction == ground truth, so every SSIM map value is a ratio of two equal fp64 expressions
    assert abs(m['known']['ssim3d'] - 1.0) <= 1e-12 and m['synthesised']['voxels'] == 0 and m['synthesised']['mae'] is None
    assert not os.path.exists(runs['tmp'] / 'known' / 'metrics_t1ce.json')


def test_ensemble_has_no_spread_on_the_known_voxels(runs):
    k01, known = _k01(runs['vol'](runs['p']['K'])), _dropped_mask()
    mean, std = runs['pred']('ens').astype(np.float32), runs['pred']('ens', '_std').astype(np.float32)
    assert np.array_equal(mean[known], k01[known]) and np.isfinite(std).all()
    assert not std[known].any() and std[~known].max() > 0 and std.min() >= 0


def test_a_resampled_partial_field_of_view(runs):
    src, ref = runs['shifted'], np.eye(4)
    want = R.coverage(np.linalg.solve(src, ref), (16, 16, 5), (16, 16, 9))
    assert int(want.sum()) == 4 * 256                          # the planes z = 3..6: 0 <= z - 2.5 <= 4
    rep = runs['report']('regrid')
    assert rep['known_voxels'] == rep['terms']['coverage'] == int(want.sum()) and rep['resampled'] == ['known_volume']
    assert rep['known_per_slice'] == [0, 0, 0, 256, 256, 256, 256, 0, 0]
    assert VS.done_line(runs['log']['regrid']).endswith(' | regrid=known_volume | known=0.444')
    pred = runs['pred']('regrid')
    assert np.isfinite(pred).all() and pred[:, :, :3].any() and pred[:, :, 7:].any()


def test_with_the_flags_the_bytes_are_those_of_the_separate_code_paths(runs):
    """The three modes share one constraint path (mudiff_hip.constraints): the runs with the flags write the bytes, and report the
    residuals, that the commit before it wrote (recorded there: tests/golden/constraint_parent_payloads.json)."""
    import hashlib
    from conftest import REPO
    with open(os.path.join(REPO, 'tests', 'golden', 'constraint_parent_payloads.json')) as f:
        recorded = json.load(f)['known']
    for job, suffix in (('known', ''), ('ens', ''), ('ens', '_std'), ('r2', '')):
        got = VS.payload(str(runs['tmp'] / job / f'predicted_t1ce{suffix}.nii.gz'))
        assert hashlib.sha256(got).hexdigest() == recorded[job + suffix], job + suffix
