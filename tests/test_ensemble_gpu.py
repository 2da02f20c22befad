"""GPU: N-sample ensembles (csrc/ensemble.hip, ops.randn_keyed / ops.ensemble_stats, GraphSampler.sample_keyed,
mudiff_hip.ensemble.sample_ensemble, the drivers' --num_samples) against the numpy restatement in tests/ensemble_ref.py and the eager
sampler, plus the independence of an ensemble from batch size, chunking and sharding."""
import json
import os
import re
import subprocess
import sys
import textwrap

import numpy as np
import pytest
import torch

from conftest import PKG, REPO
from helpers import SMALL_CFGS
import ensemble_ref as R
from oracle import mudiff_oracle as O

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
TOL = 5e-5


def _ulp_diff(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    ia = np.where(ia < 0, -(ia & 0x7fffffff), ia)                  # sign-magnitude -> a monotone integer line
    ib = np.where(ib < 0, -(ib & 0x7fffffff), ib)
    return np.abs(ia - ib)


def _child(code, timeout=900):
    """Run `code` in a fresh interpreter with MUD_DETERMINISTIC=1 (read at import): every GroupNorm then reduces in a fixed order, so
    two sampler runs on the same inputs at the same batch size give the same bits."""
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([REPO, PKG, os.path.join(REPO, 'tests'), os.environ.get('PYTHONPATH', '')]),
               MUD_DETERMINISTIC='1')
    for k in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE'):
        env.pop(k, None)
    p = subprocess.run([sys.executable, '-c', textwrap.dedent(code)], cwd=REPO, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=timeout)
    assert p.returncode == 0, p.stderr[-3000:]
    return p.stdout


def _gens(cfg, seed=1234):
    from backbones.ncsnpp_generator_adagn_feat import NCSNpp, NCSNpp_adaptive
    g1, g2 = NCSNpp(cfg), NCSNpp_adaptive(cfg)
    g1.load_state_dict(O.make_state_dict(cfg, 'g1', seed)); g2.load_state_dict(O.make_state_dict(cfg, 'g2', seed))
    return g1.to(DEV).eval(), g2.to(DEV).eval()


# ---------------------------------------------------------------------------------------------------
def test_keyed_normals_match_the_restatement():
    from mudiff_hip import ops
    keys = [[0, 0], [3, 1], [160, 7], [(1 << 40) + 3, (1 << 31) - 1], [5, 0]]
    for row_len, seed, step, kind in ((100, 1024, 0, ops.KIND_Z), (103, 7, 3, ops.KIND_NOISE), (64, (1 << 64) - 1, (1 << 24) - 1, 0),
                                      (1, 0, 2, 1), (6, 99, 1, 2)):
        want = R.randn_keyed(keys, row_len, seed, step, kind)
        got = ops.randn_keyed(torch.tensor(keys, device=DEV), row_len, seed, step, kind).cpu().numpy()
        assert got.shape == want.shape
        assert _ulp_diff(got, want).max() <= 1, (row_len, seed, step, kind)
        # an unaligned output (the scalar store path) holds the same values
        big = torch.empty(len(keys) * row_len + 1, device=DEV)
        ops.randn_keyed(torch.tensor(keys), row_len, seed, step, kind, out=big[1:])
        assert np.array_equal(big[1:].cpu().numpy().reshape(len(keys), row_len), got)
    # the draws of different kinds, steps, samples and seeds differ
    base = ops.randn_keyed(torch.tensor([[1, 1]]), 64, 5, 1, 1)
    for k2 in ([[1, 1], 64, 5, 1, 2], [[1, 1], 64, 5, 2, 1], [[1, 2], 64, 5, 1, 1], [[2, 1], 64, 5, 1, 1], [[1, 1], 64, 6, 1, 1]):
        other = ops.randn_keyed(torch.tensor([k2[0]]), *k2[1:])
        assert not torch.equal(base, other), k2


def test_keyed_normals_do_not_depend_on_row_order_or_batching():
    from mudiff_hip import ops
    g = torch.Generator().manual_seed(3)
    keys = torch.stack([torch.randint(0, 200, (37,), generator=g), torch.randint(0, 16, (37,), generator=g)], 1)
    full = ops.randn_keyed(keys, 32 * 32, 11, 2, ops.KIND_NOISE)
    perm = torch.randperm(37, generator=g)
    assert torch.equal(ops.randn_keyed(keys[perm], 32 * 32, 11, 2, ops.KIND_NOISE), full[perm.to(DEV)])
    parts = [ops.randn_keyed(keys[a:b], 32 * 32, 11, 2, ops.KIND_NOISE) for a, b in ((0, 5), (5, 6), (6, 30), (30, 37))]
    assert torch.equal(torch.cat(parts, 0), full)


def parent_bit_cases():
    """(name, output) of ops.randn_keyed over the row lengths and row counts of tests/parent_bits.py, and into an output 4 bytes off a
    16-byte boundary (row_len 8: the element path although the rows are whole quads)."""
    import parent_bits as P
    from mudiff_hip import ops
    for rows in P.ROWS:
        keys = torch.stack([torch.arange(rows) * 5 + 2, torch.arange(rows) % 3], 1)
        for row_len in P.ROW_LENS:
            yield f'{rows}x{row_len}', ops.randn_keyed(keys, row_len, 1024 + row_len, rows, ops.KIND_Z)
        out = P.off_by_one_float(torch.zeros(rows, 8, device=DEV))
        assert out.is_contiguous() and out.data_ptr() % 16 == 4
        yield f'{rows}x8 unaligned', ops.randn_keyed(keys, 8, 7, 3, ops.KIND_NOISE, out=out)


def test_the_bits_are_those_of_the_parent_commit():
    import parent_bits as P
    P.check('test_ensemble_gpu', parent_bit_cases())


def test_keyed_normals_moments():
    from mudiff_hip import ops
    keys = torch.stack([torch.arange(256) // 4, torch.arange(256) % 4], 1)
    x = ops.randn_keyed(keys, 1 << 16, 2024, 0, ops.KIND_X_INIT).double()            # 2^24 draws
    assert x.numel() == 1 << 24
    mean, var = float(x.mean()), float(x.var())
    assert abs(mean) < 1e-3 and abs(var - 1.0) < 2e-3, (mean, var)


# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N', [2, 3, 8, 33])
def test_ensemble_stats_bit_identical_to_the_restatement(N):
    from mudiff_hip import ops
    rng = np.random.default_rng(N)
    for shape in ((3, 16, 20), (2, 7, 9)):                               # hw % 4 == 0 (vector path) and odd hw (scalar path)
        x = rng.uniform(-1.6, 1.6, (shape[0], N) + shape[1:]).astype(np.float32)
        x[0, :, 0, :3] = [-1.0, 1.0, 0.0]
        x[1, N - 1, 2, 3] = np.nan                                        # NaN in one sample of one pixel
        x[1, 0, 3, 1] = np.nan                                            # and in the first sample of another
        xd = torch.from_numpy(x).to(DEV)
        for pm in ((1.0, 0.0, -np.inf, np.inf), (0.5, 0.5, 0.0, 1.0)):
            mean, std = ops.ensemble_stats(xd, *pm)
            wm, ws = R.ensemble_stats(x, *pm)
            gm, gs = mean.cpu().numpy(), std.cpu().numpy()
            assert np.array_equal(gm, wm, equal_nan=True) and np.array_equal(gs, ws, equal_nan=True), (N, shape, pm)
            assert np.array_equal(gm.view(np.int32)[~np.isnan(gm)], wm.view(np.int32)[~np.isnan(wm)])
            assert np.isnan(gm[1, 2, 3]) and np.isnan(gs[1, 2, 3]) and np.isnan(gm[1, 3, 1]) and np.isnan(gs[1, 3, 1])
            assert np.isfinite(gm[0]).all() and (gs[0] >= 0).all()
        # an unaligned sample buffer takes the scalar path with the same results
        big = torch.empty(xd.numel() + 1, device=DEV)
        big[1:] = xd.reshape(-1)
        m2, s2 = ops.ensemble_stats(big[1:].view(xd.shape), 0.5, 0.5, 0.0, 1.0)
        wm, ws = R.ensemble_stats(x, 0.5, 0.5, 0.0, 1.0)
        assert np.array_equal(m2.cpu().numpy(), wm, equal_nan=True) and np.array_equal(s2.cpu().numpy(), ws, equal_nan=True)


# ---------------------------------------------------------------------------------------------------
def test_sample_ensemble_matches_the_eager_sampler_and_the_restatement():
    from mudiff_hip import ensemble, ops
    from mudiff_hip import sampling as S
    cfg = O.default_config(**SMALL_CFGS['s32'])
    g1, g2 = _gens(cfg)
    n, N, seed, off = 3, 3, 77, 10
    g = torch.Generator().manual_seed(5)
    conds = [torch.tanh(torch.randn(n, 1, 32, 32, generator=g)).to(DEV) for _ in range(3)]
    mean, std, samples = ensemble.sample_ensemble(cfg, g1, g2, conds, N, seed, batch_size=4, slice_offset=off, return_samples=True)
    assert tuple(samples.shape) == (n, N, 32, 32) and tuple(mean.shape) == tuple(std.shape) == (n, 32, 32)
    # eager sample_from_model on the 9 items at once, with the same keyed draws injected
    keys = torch.tensor([[off + i, j] for i in range(n) for j in range(N)])
    idx = (keys[:, 0] - off).to(DEV)
    x0 = ops.randn_keyed(keys, 32 * 32, seed, 0, ops.KIND_X_INIT).view(-1, 1, 32, 32)
    zs = [ops.randn_keyed(keys, cfg.nz, seed, k, ops.KIND_Z) for k in range(cfg.num_timesteps)]
    ns = [ops.randn_keyed(keys, 32 * 32, seed, k, ops.KIND_NOISE).view(-1, 1, 32, 32) for k in range(cfg.num_timesteps)]
    coef = S.Posterior_Coefficients(cfg, DEV)
    eager = S.sample_from_model(coef, g1, conds[0][idx], g2, conds[1][idx], conds[2][idx], cfg.num_timesteps, x0, None, cfg, zs=zs, noises=ns)
    err = float((eager[:, 0].view(n, N, 32, 32) - samples).abs().max())
    assert err <= TOL, err
    wm, ws = R.ensemble_stats(samples.cpu().numpy())
    assert np.array_equal(mean.cpu().numpy(), wm) and np.array_equal(std.cpu().numpy(), ws)
    m01, s01, x01 = ensemble.sample_ensemble(cfg, g1, g2, conds, N, seed, batch_size=4, slice_offset=off, map_0_1=True, return_samples=True)
    wm, ws = R.ensemble_stats(x01.cpu().numpy(), 0.5, 0.5, 0.0, 1.0)
    assert np.array_equal(m01.cpu().numpy(), wm) and np.array_equal(s01.cpu().numpy(), ws)
    assert float((x01 - samples).abs().max()) <= TOL                    # the samples themselves are never mapped
    assert float(m01.min()) >= 0.0 and float(m01.max()) <= 1.0
    assert float(std.min()) >= 0.0 and float(std.max()) > 0.0            # the draws do differ between samples


def test_ensemble_is_independent_of_batch_chunk_and_shards(tmp_path):
    """In a child with MUD_DETERMINISTIC=1: (B=3, chunk=2) against (B=8, chunk=5) within the tolerance (the generators' kernel choices
    depend on B); two slice_offset shards at B=3, concatenated, bit-identical to one run at B=3."""
    out = _child(f'''
        import json, torch
        from helpers import SMALL_CFGS
        from oracle import mudiff_oracle as O
        from backbones.ncsnpp_generator_adagn_feat import NCSNpp, NCSNpp_adaptive
        from mudiff_hip import ensemble
        cfg = O.default_config(**SMALL_CFGS['s32'])
        g1, g2 = NCSNpp(cfg), NCSNpp_adaptive(cfg)
        g1.load_state_dict(O.make_state_dict(cfg, 'g1', 1234)); g2.load_state_dict(O.make_state_dict(cfg, 'g2', 1234))
        g1, g2 = g1.cuda().eval(), g2.cuda().eval()
        g = torch.Generator().manual_seed(8)
        conds = [torch.tanh(torch.randn(5, 1, 32, 32, generator=g)).cuda() for _ in range(3)]
        a = ensemble.sample_ensemble(cfg, g1, g2, conds, 3, 42, batch_size=3, chunk=2, return_samples=True)
        b = ensemble.sample_ensemble(cfg, g1, g2, conds, 3, 42, batch_size=8, chunk=5, return_samples=True)
        s0 = ensemble.sample_ensemble(cfg, g1, g2, [c[:2] for c in conds], 3, 42, batch_size=3, return_samples=True)
        s1 = ensemble.sample_ensemble(cfg, g1, g2, [c[2:] for c in conds], 3, 42, batch_size=3, slice_offset=2, return_samples=True)
        d = [float((x - y).abs().max()) for x, y in zip(a, b)]
        eq = [bool(torch.equal(torch.cat([x, y], 0), z)) for x, y, z in zip(s0, s1, a)]
        print(json.dumps(dict(diff=d, equal=eq)))
    ''')
    res = json.loads(out.strip().splitlines()[-1])
    assert max(res['diff']) <= TOL, res
    assert all(res['equal']), res


# ---------------------------------------------------------------------------------------------------
def _write_volumes(root, n, hw, seed):
    rng = np.random.default_rng(seed)
    os.makedirs(os.path.join(root, 'test'), exist_ok=True)
    for mod in ('T1', 'T2', 'FLAIR', 'T1CE'):
        np.save(os.path.join(root, 'test', mod + '.npy'), (rng.standard_normal((n, hw, hw)) * 2).astype(np.float32))


_LOG = re.compile(r'Average PSNR: (\S+) dB  SSIM: (\S+)  MAE: (\S+) over (\d+) slices \(global range \[(\S+), (\S+)\]\)')
_ENS = re.compile(r'\)  ensemble: (\d+) samples, mean std (\S+)$', re.M)


def test_driver_num_samples_end_to_end(tmp_path):
    """`python -m mudiff_hip.driver --device_metrics --num_samples 3` (MUD_DETERMINISTIC=1, 7 slices in batches of 4): the pred PNGs are
    the quantised ensemble means of an in-process run (a deterministic child), a std PNG exists for every slice, and the log line keeps
    its format with the ensemble note appended."""
    from PIL import Image
    data = tmp_path / 'data'
    _write_volumes(str(data), n=7, hw=32, seed=5)
    cfg = O.default_config(**SMALL_CFGS['s32'])
    out = tmp_path / 'out'
    os.makedirs(out / 'exp7')
    for which, name in (('g1', 'gen_diffusive_1'), ('g2', 'gen_diffusive_2')):
        torch.save({'module.' + k: v for k, v in O.make_state_dict(cfg, which, 1234).items()}, out / 'exp7' / f'{name}.pth')
    flags = ['--input_path', str(data), '--output_path', str(out), '--exp', 'exp7', '--target_modality', 'T2', '--image_size', '32',
             '--num_channels_dae', '32', '--ch_mult', '1', '2', '4', '--attn_resolutions', '16', '--batch_size', '4', '--device_metrics',
             '--num_samples', '3']
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([REPO, PKG, os.environ.get('PYTHONPATH', '')]), MUD_DETERMINISTIC='1')
    for k in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE'):
        env.pop(k, None)
    p = subprocess.run([sys.executable, '-m', 'mudiff_hip.driver'] + flags, cwd=REPO, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    m = _LOG.search(p.stderr)
    assert m and m.group(4) == '7', p.stderr[-2000:]
    e = _ENS.search(p.stderr)
    assert e and e.group(1) == '3', p.stderr[-2000:]
    npz = tmp_path / 'inproc.npz'
    _child(f'''
        import numpy as np, torch
        from backbones.ncsnpp_generator_adagn_feat import NCSNpp, NCSNpp_adaptive
        from mudiff_hip import driver, ensemble
        args = driver.parse_args({flags!r})
        torch.manual_seed(42)
        g1, g2 = NCSNpp(args).cuda(), NCSNpp_adaptive(args).cuda()
        driver.load_checkpoint_with_fallback(args.output_path, args.exp, g1, 'gen_diffusive_1', device='cuda:0')
        driver.load_checkpoint_with_fallback(args.output_path, args.exp, g2, 'gen_diffusive_2', device='cuda:0')
        src = driver.SliceSource('test', args.input_path, args.target_modality)
        c1, c2, c3, y = src.batch(0, len(src))
        mean, std = ensemble.sample_ensemble(args, g1, g2, [c.cuda() for c in (c1, c2, c3)], 3, args.ensemble_seed, batch_size=4)
        np.savez({str(npz)!r}, mean=mean.cpu().numpy(), std=std.cpu().numpy(), gt=y[:, 0].numpy())
    ''')
    z = np.load(npz)
    mean, std, gt = z['mean'], z['std'], z['gt']
    gmin, gmax = float(min(mean.min(), gt.min())), float(max(mean.max(), gt.max()))
    assert (float(m.group(5)), float(m.group(6))) == (round(gmin, 4), round(gmax, 4))
    from mudiff_hip import driver
    want = driver.to_uint8(list(mean), gmin, gmax)
    png = out / 'generated_samples'
    assert sorted(os.listdir(png / 'pred')) == [f'pred_{i:05d}.png' for i in range(7)]
    assert sorted(os.listdir(png / 'std')) == [f'std_{i:05d}.png' for i in range(7)]
    for i in range(7):
        assert np.array_equal(np.array(Image.open(png / 'pred' / f'pred_{i:05d}.png')), want[i]), i
    smax = float(std.max())
    stdq = driver.to_uint8(list(std), 0.0, smax)
    for i in range(7):
        assert np.array_equal(np.array(Image.open(png / 'std' / f'std_{i:05d}.png')), stdq[i]), i
    assert abs(float(e.group(2)) - float(std.astype(np.float64).mean())) <= 1e-6


def test_predict_volume_num_samples_end_to_end(tmp_path):
    """--num_samples 3 on synthetic NIfTIs: the mean and std volumes are written with the inputs' geometry, std >= 0, planes outside the
    centre window are zero, and the mean is within the tolerance of an in-process sample_ensemble of the same slices."""
    from mudiff_hip import ensemble
    from mudiff_hip import volume as V
    cfg = O.default_config(image_size=16, num_channels_dae=16, ch_mult=[1, 2], attn_resolutions=(4,), num_res_blocks=1)
    exp = tmp_path / 'results' / 'exp0'
    exp.mkdir(parents=True)
    for which, name in (('g1', 'gen_diffusive_1'), ('g2', 'gen_diffusive_2')):
        torch.save({'module.' + k: v for k, v in O.make_state_dict(cfg, which, 9).items()}, str(exp / f'{name}.pth'))
    rng = np.random.default_rng(0)
    aff = np.diag([1.0, 1.0, 2.5, 1.0]); aff[:3, 3] = (-8, -8, 3)
    paths = {}
    for m in ('flair', 't2', 't1'):
        v = (100 + 50 * rng.random((16, 16, 9))) * (rng.random((16, 16, 9)) > 0.2)
        paths[m] = str(tmp_path / f'{m}.nii.gz')
        V.write_nifti(paths[m], v.astype(np.float32), aff)
    argv = ['--target_modality', 'T1CE', '--exp', 'exp0', '--output_path', str(tmp_path / 'results'), '--image_size', '16',
            '--num_channels_dae', '16', '--ch_mult', '1', '2', '--attn_resolutions', '4', '--num_res_blocks', '1', '--slice_half_range', '2',
            '--batch_size', '4', '--input_flair', paths['flair'], '--input_t2', paths['t2'], '--input_t1', paths['t1'], '--num_samples', '3',
            '--seed', '31', '--output_dir', str(tmp_path / 'out')]
    args = V.build_argparser(argv)
    mean_path, std_path = V.predict_volume(args)
    assert mean_path.endswith('predicted_t1ce.nii.gz') and std_path.endswith('predicted_t1ce_std.nii.gz')
    mean, a, _ = V.read_nifti(mean_path)
    std, _, _ = V.read_nifti(std_path)
    assert mean.shape == std.shape == (16, 16, 9) and np.allclose(a, aff)
    for vol in (mean, std):
        assert not vol[:, :, :2].any() and not vol[:, :, 7:].any()
    assert mean[:, :, 2:7].any() and std[:, :, 2:7].any() and std.min() >= 0.0 and 0.0 <= mean.min() and mean.max() <= 1.0
    # in-process: the same preprocessing, generators and keys
    from backbones.ncsnpp_generator_adagn_feat import NCSNpp, NCSNpp_adaptive
    g1, g2 = NCSNpp(args).to(DEV), NCSNpp_adaptive(args).to(DEV)
    V.load_checkpoint(str(exp / '{}.pth'), g1, 'gen_diffusive_1', DEV)
    V.load_checkpoint(str(exp / '{}.pth'), g2, 'gen_diffusive_2', DEV)
    stacks = [np.stack(V.load_and_preprocess_volume(paths[m], 2)[0], 0) for m in ('flair', 't2', 't1')]
    conds = V.upload_conds(stacks, 16, DEV)
    m2, s2 = ensemble.sample_ensemble(args, g1, g2, conds, 3, 31, batch_size=4, map_0_1=True)
    err = float(np.abs(np.moveaxis(mean[:, :, 2:7], 2, 0) - m2.cpu().numpy()).max())
    assert err <= TOL, err
    assert float(np.abs(np.moveaxis(std[:, :, 2:7], 2, 0) - s2.cpu().numpy()).max()) <= TOL
