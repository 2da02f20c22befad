"""GPU: lockstep sampling (GraphSampler.sample_lockstep; constraints.Constraint.lockstep; thick_volume.BandMeasurement; DESIGN.md section
5.29) on the tiny model: S = 16, one GraphSampler with B = 5, 7 slices of 2 samples (14 rows: batches of 5, 5 and a padded 4), and the
n = 12 thick-volume geometry of tests/test_band_gpu.py for the constraint.  In a child process with MUD_DETERMINISTIC=1 (read at import):
every GroupNorm then reduces in a fixed order."""
import numpy as np
import pytest
import torch

import band_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
BAR = 1e-3                # the project's per-step parity bar, max-abs


def test_lockstep_equals_keyed_sampling_and_keeps_the_thick_slices():
    import os
    import subprocess
    import sys
    from conftest import PKG, REPO
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([REPO, PKG, os.path.join(REPO, 'tests'), os.environ.get('PYTHONPATH', '')]), MUD_DETERMINISTIC='1')
    c = subprocess.run([sys.executable, '-c', 'import test_lockstep_gpu as T; T.lockstep_checks(); print("LOCKSTEP-OK")'], cwd=REPO, env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    print(c.stdout[-3000:])
    assert c.returncode == 0 and 'LOCKSTEP-OK' in c.stdout, c.stdout[-3000:] + c.stderr[-3000:]


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)


def lockstep_checks():
    """The body of the test (run in its child process)."""
    import volume_support as VS
    from oracle import mudiff_oracle as O
    from backbones.ncsnpp_generator_adagn_feat import NCSNpp, NCSNpp_adaptive
    from mudiff_hip import ensemble as E, ops, sampling as Sm, thick_volume as TV
    assert ops.DETERMINISTIC
    cfg = O.default_config(**VS.TINY_MODEL)
    g1, g2 = NCSNpp(cfg), NCSNpp_adaptive(cfg)
    g1.load_state_dict(O.make_state_dict(cfg, 'g1', 9)); g2.load_state_dict(O.make_state_dict(cfg, 'g2', 9))
    g1, g2 = g1.to(DEV).eval(), g2.to(DEV).eval()
    B, S, T = 5, 16, int(cfg.num_timesteps)
    sampler = Sm.GraphSampler(Sm.Posterior_Coefficients(cfg, DEV), g1, g2, cfg, B, S, S, DEV)
    g = np.random.default_rng(29)

    # ---- without a constraint: what sample_keyed gives the same rows
    n, N = 7, 2
    rows = n * N
    c7 = [_dev(np.tanh(g.standard_normal((n, 1, S, S))).astype(np.float32)) for _ in range(3)]
    sl, sm = torch.arange(n).repeat(N), torch.arange(N).repeat_interleave(n)
    keys = torch.stack([sl + 4, sm], 1)
    conds = [c.index_select(0, sl.to(DEV)) for c in c7]
    lock = sampler.sample_lockstep(conds, keys, 31, T)
    assert tuple(lock.shape) == (rows, 1, S, S) and torch.isfinite(lock).all()
    keyed = torch.empty_like(lock)
    for lo in range(0, rows, B):
        m = min(B, rows - lo)
        idx = torch.tensor(list(range(lo, lo + m)) + [lo + m - 1] * (B - m))
        keyed[lo:lo + m] = sampler.sample_keyed(*(c[idx.to(DEV)] for c in conds), keys[idx], 31, T)[:m]
    diff = float((lock - keyed).abs().max())
    print(f'lockstep against sample_keyed: max |difference| {diff:.3e}, bit-equal {torch.equal(lock, keyed)}')
    assert diff <= BAR
    assert torch.equal(sampler.sample_lockstep(c7, keys, 31, T, cond_index=sl), lock)     # the conditions by index
    # ---- the rows in another order: other batches, the same result (bitwise: tests/test_thick_volume_gpu.py holds --known_thick to
    # the same bytes at another --batch_size on this model)
    perm = torch.from_numpy(np.random.default_rng(3).permutation(rows))
    moved = sampler.sample_lockstep([c[perm.to(DEV)] for c in conds], keys[perm], 31, T)
    back = torch.empty_like(moved)
    back[perm.to(DEV)] = moved
    print(f'lockstep, permuted rows: max |difference| {float((back - lock).abs().max()):.3e}')
    assert torch.equal(back, lock)
    for bad in (dict(resample=2), dict(cond_index=sl + 1)):
        with pytest.raises(ValueError, match='sample_lockstep'):
            sampler.sample_lockstep(c7, keys, 31, T, **{**dict(cond_index=sl), **bad})

    # ---- a thick volume over 12 thin slices: centres 1.25 + 2.5 j, 3 thin slices thick (m = 4, bandwidth 1; thin slice 11 is free)
    n = 12
    A, centres, _ = R.weights(n, 1.25, 2.5, 3.0, 'box')
    c12 = [_dev(np.tanh(g.standard_normal((n, 1, S, S))).astype(np.float32)) for _ in range(3)]
    k = np.tanh(g.standard_normal((n, S * S))).astype(np.float32)
    y = R.measure(k, A).astype(np.float32)
    sl, sm = torch.arange(n).repeat(N), torch.arange(N).repeat_interleave(n)
    keys = torch.stack([sl, sm], 1)
    meas = TV.BandMeasurement(_dev(y).view(-1, S, S), A, centres=centres)
    assert meas.lockstep and meas.tables.bw == 1 and meas.m == 4 and meas.chunk_end(0, 5) == n
    free = sampler.sample_lockstep(c12, keys, 31, T, cond_index=sl)
    out = sampler.sample_lockstep(c12, keys, 31, T, constraint=meas, cond_index=sl)
    x_new = sampler.lockstep_x_new.clone()
    meas.record_volume(out, x_new)
    assert not torch.equal(out, free)
    flat = lambda v: v.reshape(N, n, S * S).cpu().numpy()                                # noqa: E731
    worst = 0.0
    for s in range(N):
        res = np.abs(R.measure(flat(out)[s], A) - y.astype(np.float64))
        rb = R.bound_residual(flat(x_new)[s], y, A)
        worst = max(worst, float(np.max(res / rb)))
        assert (res <= rb).all()
        assert torch.equal(out[s * n + 11], free[s * n + 11])                            # under no thick slice: free, and keyed
        assert not torch.equal(out[s * n], free[s * n])
    print(f'lockstep with a thick volume: worst clean residual / bound {worst:.3f}, report {meas.residual.cpu().tolist()}')
    assert float(meas.residual.max()) < 1e-5 and meas.finish()['max_residual'] == float(meas.residual.max())
    again = sampler.sample_lockstep(c12, keys, 31, T, constraint=meas, cond_index=sl, coupling='shared', resample=2)
    assert torch.isfinite(again).all()
    for s in range(N):
        res = np.abs(R.measure(flat(again)[s], A) - y.astype(np.float64))
        assert (res <= R.bound_residual(flat(sampler.lockstep_x_new)[s], y, A)).all()
    with pytest.raises(ValueError, match='whole stacks'):
        sampler.sample_lockstep(c12, keys[:-1], 31, T, constraint=meas, cond_index=sl[:-1])

    # ---- an ensemble takes the same road: its samples are the lockstep rows, whatever the chunk
    mean, std, every = E.sample_ensemble(cfg, g1, g2, c12, N, 31, sampler=sampler, constraint=TV.BandMeasurement(_dev(y).view(-1, S, S), A),
                                         return_samples=True, chunk=3)
    assert torch.equal(every, out.view(N, n, S, S).transpose(0, 1)) and torch.isfinite(mean).all() and torch.isfinite(std).all()
    real = torch.cuda.mem_get_info
    torch.cuda.mem_get_info = lambda *a: (1 << 10, 1 << 40)
    try:
        with pytest.raises(ValueError, match='--num_samples'):
            E.sample_ensemble(cfg, g1, g2, c12, N, 31, sampler=sampler, constraint=TV.BandMeasurement(_dev(y).view(-1, S, S), A))
    finally:
        torch.cuda.mem_get_info = real
