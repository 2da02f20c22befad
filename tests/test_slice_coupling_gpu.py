"""GPU: slice-coupled sampling noise (csrc/ensemble.hip: mud_randn_keyed_coupled, ops.randn_keyed_coupled, GraphSampler.sample_keyed's
`coupling`, the volume pipeline's --slice_coupling / --through_plane) against the numpy restatement in tests/slice_coupling_ref.py, the
statistics of the draws on the device, and the direction of the effect on the seeded tiny model.  DESIGN.md section 5.23."""
import json
import math
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest
import torch

from conftest import PKG, REPO
import slice_coupling_ref as R
import volume_support as VS

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
TOL = 5e-5                                                   # tests/test_ensemble_gpu.py: the same samples at two batch sizes
JITTER = 1e-4                                                # the project's bound for run-to-run jitter
KEYS = [[0, 0], [1, 3], [2, 0], [7, 3], [1 << 40, 0]]        # slices 0, 1, 2: taps below slice 0 wrap to 2^64 - j
RADII = (0, 1, 3, 32)


def _half(radius):
    """Gaussian half taps of unit square sum for a given radius (radius 0: the single tap 1)."""
    sigma = max(radius, 1) / 3.0
    w = np.exp(-np.arange(radius + 1, dtype=np.float64) ** 2 / (2 * sigma * sigma))
    return w / math.sqrt(float(w[0] ** 2 + 2 * np.sum(w[1:] ** 2)))


# row_len -> the (seed, step, kind) draws checked at it: 4 = one whole block, 10 and 4099 = a ragged tail (4099: more than one workgroup
# per row), 100 = whole blocks, all three kinds at two steps
DRAWS = {4: [(5, 0, 0)], 10: [(1024, 1, 1)], 100: [(7, s, k) for s in (0, 3) for k in (0, 1, 2)], 4099: [((1 << 64) - 1, 2, 2)]}


@pytest.mark.parametrize('row_len', sorted(DRAWS))
def test_coupled_normals_are_the_restatement_bit_for_bit(row_len):
    from mudiff_hip import ops
    keys = torch.tensor(KEYS, device=DEV)
    for seed, step, kind in DRAWS[row_len]:
        noise = R.WhiteNoise(row_len, seed, step, kind)          # the white rows are shared by the four radii
        for radius in RADII:
            half = _half(radius)
            want = R.randn_keyed_coupled(KEYS, row_len, seed, step, kind, half, radius, noise)
            got = ops.randn_keyed_coupled(keys, row_len, seed, step, kind, half, radius).cpu().numpy()
            assert got.shape == want.shape == (len(KEYS), row_len)
            assert np.array_equal(got, want), (row_len, seed, step, kind, radius, int((got != want).sum()))
            # an output offset by one float (the scalar store path) holds the same values
            big = torch.full((len(KEYS) * row_len + 2,), 7.0, device=DEV)
            ops.randn_keyed_coupled(torch.tensor(KEYS), row_len, seed, step, kind, half, radius, out=big[1:-1])
            assert np.array_equal(big[1:-1].cpu().numpy().reshape(len(KEYS), row_len), want)
            assert float(big[0]) == 7.0 and float(big[-1]) == 7.0
            if radius == 0:
                assert torch.equal(ops.randn_keyed_coupled(keys, row_len, seed, step, kind, [1.0], 0), ops.randn_keyed(keys, row_len, seed, step, kind))
                assert np.array_equal(got, R.E.randn_keyed(KEYS, row_len, seed, step, kind))


def test_coupled_normals_refuse_bad_arguments():
    from mudiff_hip import MudiffHipError, ops
    for half, radius in (([1.0], 1), ([1.0] * 34, 33), ([float('nan')], 0), ([1.0, 0.5], -1)):
        with pytest.raises(MudiffHipError):
            ops.randn_keyed_coupled(torch.tensor([[0, 0]]), 8, 1, 0, 0, half, radius)
    with pytest.raises(MudiffHipError):
        ops.randn_keyed_coupled(torch.tensor([[-1, 0]]), 8, 1, 0, 0, [1.0], 0)              # the keys themselves stay >= 0
    with pytest.raises(MudiffHipError):
        ops.randn_keyed_coupled(torch.tensor([[0, 0]]), 8, 1, 0, 3, [1.0], 0)


def test_coupled_normals_do_not_depend_on_row_order_or_batching():
    from mudiff_hip import ops
    g = torch.Generator().manual_seed(3)
    keys = torch.stack([torch.randint(0, 200, (37,), generator=g), torch.randint(0, 16, (37,), generator=g)], 1)
    half, radius = _half(5), 5
    full = ops.randn_keyed_coupled(keys, 33 * 31, 11, 2, ops.KIND_NOISE, half, radius)
    perm = torch.randperm(37, generator=g)
    assert torch.equal(ops.randn_keyed_coupled(keys[perm], 33 * 31, 11, 2, ops.KIND_NOISE, half, radius), full[perm.to(DEV)])
    parts = [ops.randn_keyed_coupled(keys[a:b], 33 * 31, 11, 2, ops.KIND_NOISE, half, radius) for a, b in ((0, 5), (5, 6), (6, 30), (30, 37))]
    assert torch.equal(torch.cat(parts, 0), full)


def parent_bit_cases():
    """(name, output) of ops.randn_keyed_coupled at radius 0, 3 and 32 over the row lengths and row counts of tests/parent_bits.py, and
    into an output 4 bytes off a 16-byte boundary (row_len 8: the element path although the rows are whole quads)."""
    import parent_bits as P
    from mudiff_hip import ops
    for radius in (0, 3, 32):
        half = _half(radius)
        for rows in P.ROWS:
            keys = torch.stack([torch.arange(rows) * 5, torch.arange(rows) % 3], 1)         # slice 0: taps below it wrap
            for row_len in P.ROW_LENS:
                yield f'R{radius} {rows}x{row_len}', ops.randn_keyed_coupled(keys, row_len, 77 + row_len, rows, ops.KIND_NOISE, half, radius)
            out = P.off_by_one_float(torch.zeros(rows, 8, device=DEV))
            assert out.is_contiguous() and out.data_ptr() % 16 == 4
            yield f'R{radius} {rows}x8 unaligned', ops.randn_keyed_coupled(keys, 8, 7, 3, ops.KIND_Z, half, radius, out=out)


def test_the_bits_are_those_of_the_parent_commit():
    import parent_bits as P
    P.check('test_slice_coupling_gpu', parent_bit_cases())


def test_coupled_normals_moments_on_the_device():
    """64 consecutive slices x 65536 elements at sigma = 2 (R = 6): every row's mean within 6 / sqrt(L), its variance within
    6 sqrt(2 / L), and every pair's lag-d correlation within 6 / sqrt(L) of coupling_correlation, d = 1..2R + 2."""
    from mudiff_hip import ops, slice_coupling as SC
    n, L, sigma = 64, 1 << 16, 2.0
    half, radius = SC.coupling_taps(sigma)
    keys = torch.stack([torch.arange(n), torch.zeros(n, dtype=torch.int64)], 1)
    x = ops.randn_keyed_coupled(keys, L, 2024, 1, ops.KIND_NOISE, half, radius).double()
    mean, var = x.mean(1), x.var(1, unbiased=False)
    worst_mean, worst_var = float(mean.abs().max()), float((var - 1).abs().max())
    print(f'max |mean| {worst_mean:.5f} (bound {6 / math.sqrt(L):.5f})  max |var - 1| {worst_var:.5f} (bound {6 * math.sqrt(2 / L):.5f})')
    assert worst_mean <= 6 / math.sqrt(L) and worst_var <= 6 * math.sqrt(2 / L)
    worst = 0.0
    for d in range(1, 2 * radius + 3):
        rho = SC.coupling_correlation(sigma, d)
        worst = max(worst, float(((x[:-d] * x[d:]).mean(1) - rho).abs().max()))
    print(f'max |corr - rho| {worst:.5f} (bound {6 / math.sqrt(L):.5f})')
    assert worst <= 6 / math.sqrt(L)
    assert SC.coupling_correlation(sigma, 2 * radius + 1) == 0.0


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


def test_shared_draws_give_equal_rows_for_equal_conditions():
    """sample_keyed(coupling='shared') on the tiny seeded model, the three conditions constant along the batch (MUD_DETERMINISTIC=1): all
    rows agree within the run-to-run jitter bound, and the uncoupled keyed call's rows spread strictly more."""
    out = _child(f'''
        import json, torch
        from oracle import mudiff_oracle as O
        from backbones.ncsnpp_generator_adagn_feat import NCSNpp, NCSNpp_adaptive
        from mudiff_hip import sampling as S
        cfg = O.default_config(**{VS.TINY_MODEL!r})
        g1, g2 = NCSNpp(cfg), NCSNpp_adaptive(cfg)
        g1.load_state_dict(O.make_state_dict(cfg, 'g1', 9)); g2.load_state_dict(O.make_state_dict(cfg, 'g2', 9))
        g1, g2 = g1.cuda().eval(), g2.cuda().eval()
        B, size = 6, cfg.image_size
        g = torch.Generator().manual_seed(4)
        conds = [torch.tanh(torch.randn(1, 1, size, size, generator=g)).expand(B, 1, size, size).contiguous().cuda() for _ in range(3)]
        sampler = S.GraphSampler(S.Posterior_Coefficients(cfg, 'cuda:0'), g1, g2, cfg, B, size, size, 'cuda:0')
        keys = torch.stack([torch.arange(B) + 3, torch.zeros(B, dtype=torch.int64)], 1)
        spread = lambda x: float((x - x[:1]).abs().max())
        shared = sampler.sample_keyed(*conds, keys, 31, cfg.num_timesteps, coupling='shared')
        plain = sampler.sample_keyed(*conds, keys, 31, cfg.num_timesteps)
        again = sampler.sample_keyed(*conds, keys, 31, cfg.num_timesteps, coupling=None)
        print(json.dumps(dict(shared=spread(shared), plain=spread(plain), same=bool(torch.equal(plain, again)),
                              finite=bool(torch.isfinite(shared).all()))))
    ''')
    res = json.loads(out.strip().splitlines()[-1])
    print(f"row-to-row spread: shared {res['shared']:.3e}, uncoupled {res['plain']:.3e}")
    assert res['finite'] and res['same']
    assert res['shared'] <= JITTER, res
    assert res['plain'] > res['shared'], res


# ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def runs(tmp_path_factory):
    """16 x 16 x 9 inputs that vary smoothly in z, the tiny model, every run in one child process."""
    from mudiff_hip import volume as V
    tmp = tmp_path_factory.mktemp('coupled')
    VS.write_tiny_model(tmp)
    x, y, z = np.meshgrid(np.arange(16.0), np.arange(16.0), np.arange(9.0), indexing='ij')
    p = {k: str(tmp / f'{k}.nii.gz') for k in ('flair', 't2', 't1')}
    for i, k in enumerate(p):
        vol = 120 + 60 * np.sin(x / (3 + i) + 0.3 * z) * np.cos(y / (4 - i) - 0.2 * z) + 4 * z
        V.write_nifti(p[k], vol.astype(np.float32), np.eye(4))
    inputs = ['--input_flair', p['flair'], '--input_t2', p['t2'], '--input_t1', p['t1']]
    jobs = {'plain': (4, ['--through_plane']), 'sc4': (4, ['--slice_coupling', '4', '--through_plane']),
            'sc4_b9': (9, ['--slice_coupling', '4']), 'sc4_dev': (4, ['--slice_coupling', '4', '--device_intake']),
            'ens': (4, ['--num_samples', '2', '--slice_coupling', '2']), 'shared': (4, ['--slice_coupling', 'shared'])}
    steps = [VS.volume_step(k, VS.model_argv(tmp, 4, b) + inputs + a + ['--output_dir', str(tmp / k)]) for k, (b, a) in jobs.items()]
    manifest = tmp / 'cohort.tsv'
    manifest.write_text('id\tt1\tt1ce\tt2\tflair\ns0\t' + '\t'.join([p['t1'], '', p['t2'], p['flair']]) + '\n')
    steps.append(VS.cohort_step('cohort', VS.model_argv(tmp, 4, 4) + ['--slice_coupling', '4', '--through_plane', '--manifest', str(manifest),
                                                                     '--output_dir', str(tmp / 'cohort')]))
    log = VS.run_plan(tmp, steps, 900, ignore='RuntimeWarning')
    return dict(tmp=tmp, log=log, pred=lambda k: VS.payload(str(tmp / k / 'predicted_t1ce.nii.gz')))


def _volume(path):
    from mudiff_hip import volume as V
    return V.read_nifti(str(path))[0]


def test_slice_coupling_end_to_end(runs):
    tmp, log = runs['tmp'], runs['log']
    assert VS.done_line(log['sc4']).endswith(' | slice_coupling=4') and VS.done_line(log['shared']).endswith(' | slice_coupling=shared')
    assert 'slice_coupling' not in VS.done_line(log['plain'])
    reps = {k: json.load(open(tmp / k / 'through_plane_t1ce.json')) for k in ('plain', 'sc4')}
    for k, rep in reps.items():
        assert rep['slab'] == [0, 8] and rep['mask'] == 'slab' and len(rep['prediction']['dz']) == 8
        assert sum(ln.startswith('[through-plane] slab 0..8') for ln in log[k].splitlines()) == 1
        assert not os.path.exists(tmp / k / 'metrics_t1ce.json')
    assert not os.path.exists(tmp / 'sc4_b9' / 'through_plane_t1ce.json')
    dz = {k: rep['prediction']['mean_dz'] for k, rep in reps.items()}
    print(f"mean_dz: default {dz['plain']:.6f}, --slice_coupling 4 {dz['sc4']:.6f}, ratio {dz['sc4'] / dz['plain']:.4f}")
    assert dz['sc4'] < dz['plain']
    assert runs['pred']('sc4') != runs['pred']('plain')
    # the same volume whatever the batch size (the generators' kernel choices depend on it: within the ensemble tests' tolerance)
    a, b = _volume(tmp / 'sc4' / 'predicted_t1ce.nii.gz'), _volume(tmp / 'sc4_b9' / 'predicted_t1ce.nii.gz')
    assert a.shape == (16, 16, 9) and float(np.abs(a - b).max()) <= TOL and a.any()
    # host and device intake, and a one-subject cohort, write the same bytes
    assert runs['pred']('sc4') == runs['pred']('sc4_dev') == VS.payload(str(tmp / 'cohort' / 's0' / 'predicted_t1ce.nii.gz'))
    assert VS.done_line(log['cohort']).endswith(' | slice_coupling=4')
    assert json.load(open(tmp / 'cohort' / 's0' / 'through_plane_t1ce.json'))['prediction'] == reps['sc4']['prediction']


def test_slice_coupling_with_an_ensemble(runs):
    tmp = runs['tmp']
    assert VS.done_line(runs['log']['ens']).endswith(' | 2 samples per slice | slice_coupling=2')
    mean, std = _volume(tmp / 'ens' / 'predicted_t1ce.nii.gz'), _volume(tmp / 'ens' / 'predicted_t1ce_std.nii.gz')
    assert mean.shape == std.shape == (16, 16, 9) and np.isfinite(mean).all() and np.isfinite(std).all()
    assert mean.any() and std.any() and std.min() >= 0.0 and 0.0 <= mean.min() and mean.max() <= 1.0
