"""N-sample ensemble inference: every slice sampled N times, reduced to a per-pixel mean and spread.

The sampler is stochastic (x_init, every step's z and posterior noise), so one draw per slice hides how much a synthesis varies.
Here the (slice, sample) items of a stack are packed slice-major into the captured batch of a sampling.GraphSampler, with every
Gaussian keyed by (seed, global slice, sample, step, kind) (ops.randn_keyed), and each slice's N samples are reduced on the device
by ops.ensemble_stats (fp64, in sample order).  The result does not depend on the batch size (beyond the generators' own kernel
choices, which depend on B), the chunking or how slices are sharded over ranks: `slice_offset` is the global index of the first
slice, so shards draw what a single run would.

    mean, std = sample_ensemble(args, g1, g2, conds, num_samples=8, seed=1024, map_0_1=True)
"""
from __future__ import annotations

import math

import torch

from . import ops

CHUNK_BYTES = 1 << 30      # default bound of the [chunk, N, S, S] sample buffer


def default_chunk(num_samples, size, n):
    """Slices per chunk: the most whose samples fit into CHUNK_BYTES (at least 1, at most n)."""
    per_slice = 4 * int(num_samples) * int(size) * int(size)
    return max(1, min(max(int(n), 1), CHUNK_BYTES // per_slice))


def premap(map_0_1):
    """(scale, shift, lo, hi) of ops.ensemble_stats: ops.to_range_0_1's [-1,1] -> [0,1], or the identity."""
    return (0.5, 0.5, 0.0, 1.0) if map_0_1 else (1.0, 0.0, -math.inf, math.inf)


def sample_ensemble(args, gen1, gen2, conds, num_samples, seed, batch_size=32, slice_offset=0, chunk=None, sampler=None, map_0_1=False,
                    return_samples=False, coupling=None):
    """conds: three device tensors [n,1,S,S] (S = args.image_size) -> (mean, std) device fp32 [n,S,S] over `num_samples` (>= 2) samples
    per slice, plus the raw samples [n,N,S,S] with `return_samples`.  `map_0_1`: the statistics are those of the samples mapped to
    [0,1] (ops.to_range_0_1); the returned samples are never mapped.

    Items (slice i, sample j) run slice-major in batches of the sampler's B (`sampler`, a sampling.GraphSampler for these generators
    and this image size, else one is captured at `batch_size`); the last batch of a chunk is padded by repeating its last item.  At most
    `chunk` slices' samples are held at a time (default: a buffer of at most 1 GiB).  Slice i is keyed as slice_offset + i.
    `coupling`: GraphSampler.sample_keyed's (mudiff_hip.slice_coupling): sample j of neighbouring slices then shares part of its draws;
    the keys stay global, so shards and chunks still draw what a single run would."""
    from . import sampling as S
    N = int(num_samples)
    if N < 2:
        raise ValueError(f'sample_ensemble: num_samples must be >= 2, got {N}')
    if int(slice_offset) < 0:
        raise ValueError(f'sample_ensemble: slice_offset must be >= 0, got {slice_offset}')
    c1, c2, c3 = conds
    n, size = int(c1.shape[0]), int(args.image_size)
    for c in conds:
        if tuple(c.shape) != (n, 1, size, size) or not c.is_cuda:
            raise ValueError(f'sample_ensemble: conditions must be device tensors [{n}, 1, {size}, {size}], got {tuple(c.shape)}')
    device = c1.device
    T = int(args.num_timesteps)
    if sampler is None:
        sampler = S.GraphSampler(S.Posterior_Coefficients(args, device), gen1, gen2, args, int(batch_size), size, size, device)
    elif (sampler.H, sampler.W) != (size, size) or sampler.g1 is not gen1 or sampler.g2 is not gen2:
        raise ValueError('sample_ensemble: the sampler was built for other generators or another image size')
    B = sampler.B
    chunk = default_chunk(N, size, n) if chunk is None else int(chunk)
    if chunk < 1:
        raise ValueError(f'sample_ensemble: chunk must be >= 1, got {chunk}')
    scale, shift, lo, hi = premap(map_0_1)
    mean = torch.empty(n, size, size, device=device, dtype=torch.float32)
    std = torch.empty_like(mean)
    every = torch.empty(n, N, size, size, device=device, dtype=torch.float32) if return_samples else None
    buf = None
    for s0 in range(0, n, chunk):
        s1 = min(s0 + chunk, n)
        if every is not None:
            out = every[s0:s1]
        else:
            if buf is None:
                buf = torch.empty(min(chunk, n), N, size, size, device=device, dtype=torch.float32)
            out = buf[:s1 - s0]
        flat = out.view(-1, size, size)
        q0, q1 = s0 * N, s1 * N                                  # items of this chunk, slice-major
        for b0 in range(q0, q1, B):
            m = min(B, q1 - b0)
            items = torch.arange(b0, b0 + B).clamp_(max=b0 + m - 1)          # padding repeats the last item
            sl = items // N
            keys = torch.stack([sl + int(slice_offset), items % N], 1)
            idx = sl.to(device)
            res = sampler.sample_keyed(c1.index_select(0, idx), c2.index_select(0, idx), c3.index_select(0, idx), keys, seed, T, coupling=coupling)
            flat[b0 - q0:b0 - q0 + m] = res[:m, 0]
        mean[s0:s1], std[s0:s1] = ops.ensemble_stats(out, scale, shift, lo, hi)
    return (mean, std, every) if return_samples else (mean, std)
