"""N-sample ensemble inference: every slice sampled N times, reduced to a per-pixel mean and spread.

The sampler is stochastic (x_init, every step's z and posterior noise), so one draw per slice hides how much a synthesis varies.
Here the (slice, sample) items of a stack are packed slice-major into the captured batch of a sampling.GraphSampler, with every
Gaussian keyed by (seed, global slice, sample, step, kind) (ops.randn_keyed), and each slice's N samples are reduced on the device
by ops.ensemble_stats (fp64, in sample order).  The result does not depend on the batch size (beyond the generators' own kernel
choices, which depend on B), the chunking or how slices are sharded over ranks: `slice_offset` is the global index of the first
slice, so shards draw what a single run would.

    mean, std = sample_ensemble(args, g1, g2, conds, num_samples=8, seed=1024, map_0_1=True)
    mean, std, q = sample_ensemble(..., quantiles=(0.05, 0.5, 0.95))      # q [3,n,S,S]: the interval's bounds and the median (section 5.24)
"""
from __future__ import annotations

import math

import torch

from . import ops

CHUNK_BYTES = 1 << 30      # default bound of the [chunk, N, S, S] sample buffer
MAX_QUANTILES, MAX_QUANTILE_SAMPLES = 8, 64      # ops.ensemble_quantiles: fractions per call, samples per pixel


def default_chunk(num_samples, size, n):
    """Slices per chunk: the most whose samples fit into CHUNK_BYTES (at least 1, at most n)."""
    per_slice = 4 * int(num_samples) * int(size) * int(size)
    return max(1, min(max(int(n), 1), CHUNK_BYTES // per_slice))


def check_quantiles(quantiles):
    """-> the fractions as a tuple of floats; ValueError unless there are 1 to MAX_QUANTILES of them, each finite and in [0, 1]."""
    try:
        q = tuple(float(v) for v in quantiles)
    except (TypeError, ValueError):
        raise ValueError(f'quantiles must be a sequence of fractions in [0, 1], got {quantiles!r}') from None
    if not 1 <= len(q) <= MAX_QUANTILES or not all(math.isfinite(v) and 0.0 <= v <= 1.0 for v in q):
        raise ValueError(f'quantiles: need 1 to {MAX_QUANTILES} fractions in [0, 1], got {list(q)}')
    return q


def premap(map_0_1):
    """(scale, shift, lo, hi) of ops.ensemble_stats: ops.to_range_0_1's [-1,1] -> [0,1], or the identity."""
    return (0.5, 0.5, 0.0, 1.0) if map_0_1 else (1.0, 0.0, -math.inf, math.inf)


def sample_ensemble(args, gen1, gen2, conds, num_samples, seed, batch_size=32, slice_offset=0, chunk=None, sampler=None, map_0_1=False,
                    return_samples=False, coupling=None, quantiles=None, known=None, resample=1, kspace=None, thick=None,
                    constraint=None):
    """conds: three device tensors [n,1,S,S] (S = args.image_size) -> (mean, std) device fp32 [n,S,S] over `num_samples` (>= 2) samples
    per slice, plus the raw samples [n,N,S,S] with `return_samples`.  `map_0_1`: the statistics are those of the samples mapped to
    [0,1] (ops.to_range_0_1); the returned samples are never mapped.

    Items (slice i, sample j) run slice-major in batches of the sampler's B (`sampler`, a sampling.GraphSampler for these generators
    and this image size, else one is captured at `batch_size`); the last batch of a chunk is padded by repeating its last item.  At most
    `chunk` slices' samples are held at a time (default: a buffer of at most 1 GiB).  Slice i is keyed as slice_offset + i.
    `coupling`: GraphSampler.sample_keyed's (mudiff_hip.slice_coupling): sample j of neighbouring slices then shares part of its draws;
    the keys stay global, so shards and chunks still draw what a single run would.
    `quantiles`: a tuple of 1 to 8 fractions in [0, 1] (num_samples <= MAX_QUANTILE_SAMPLES): the per-pixel quantiles of each slice's
    samples under the same pre-map (ops.ensemble_quantiles; 0.5 is the median), taken from the chunk buffer right
    after the statistics, are returned as one more tensor [K,n,S,S] at the end of the tuple.  None returns exactly what it did before.
    `known`, `kspace`, `thick` (at most one): what of the target was acquired - (known [n,1,S,S], mask uint8
    [n,1,S,S]) per slice on the device, a kspace.KSpaceMeasurement or a thick.ThickMeasurement for these n slices, with `resample` what
    GraphSampler.sample_keyed takes; or `constraint`, any of them as one object of mudiff_hip.constraints (its own `resample` counts).
    Every sample of slice i is drawn under it and handed to its `record`.  Thick slices couple the L thin slices of a (slab, sample), so
    a measured slab's items run sample-major - each sample's L slices together, never split over two batches (constraints.batches) -
    and a chunk ends before a slab it would cut (the constraint's `chunk_end`).  Free slices keep their item order.  A constraint that couples the whole stack
    (`lockstep`: thick_volume.BandMeasurement, section 5.29) makes the whole n one chunk and every item advance together
    (GraphSampler.sample_lockstep): ValueError naming --num_samples when 2 N n S^2 x 4 bytes exceed the free device memory."""
    from . import sampling as S
    from .constraints import batches, of_prediction
    constraint, resample = of_prediction('sample_ensemble', constraint, known, kspace, thick, resample)
    N = int(num_samples)
    if N < 2:
        raise ValueError(f'sample_ensemble: num_samples must be >= 2, got {N}')
    if quantiles is not None:
        quantiles = check_quantiles(quantiles)
        if N > MAX_QUANTILE_SAMPLES:
            raise ValueError(f'sample_ensemble: quantiles need num_samples <= {MAX_QUANTILE_SAMPLES} (the sorting network of '
                             f'ops.ensemble_quantiles), got {N}')
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
    qmaps = None if quantiles is None else torch.empty(len(quantiles), n, size, size, device=device, dtype=torch.float32)
    buf = None
    constraint.over(n, 'sample_ensemble')
    if constraint.lockstep:                  # the constraint couples the whole stack: all N n items advance together (section 5.29)
        out = _sample_lockstep(sampler, conds, constraint, N, n, size, seed, T, int(slice_offset), coupling, resample, every)
        mean[:], std[:] = ops.ensemble_stats(out, scale, shift, lo, hi)
        if qmaps is not None:
            qmaps[:] = ops.ensemble_quantiles(out, quantiles, scale, shift, lo, hi)
        res = (mean, std, every) if return_samples else (mean, std)
        return res if qmaps is None else res + (qmaps,)
    chunks, s0 = [], 0
    while s0 < n:
        s1 = constraint.chunk_end(s0, min(s0 + chunk, n))
        chunks.append((s0, s1))
        s0 = s1
    for s0, s1 in chunks:
        if every is not None:
            out = every[s0:s1]
        else:
            if buf is None:
                buf = torch.empty(min(chunk, n), N, size, size, device=device, dtype=torch.float32)
            out = buf[:s1 - s0]
        flat = out.view(-1, size, size)
        units = []
        for u in constraint.units(s0, s1):
            units += [[(i, j) for i in u] for j in range(N)]      # a free slice: slice-major; a slab: sample-major, each sample's slices one unit
        for items in batches(units, B):
            m = len(items)
            items = items + [items[-1]] * (B - m)                    # padding repeats the last item
            sl, sm = (torch.as_tensor(v, dtype=torch.int64) for v in zip(*items))
            keys = torch.stack([sl + int(slice_offset), sm], 1)
            bound = constraint.for_rows([i for i, _ in items], [j for _, j in items], m)
            idx = sl.to(device)
            res = sampler.sample_keyed(c1.index_select(0, idx), c2.index_select(0, idx), c3.index_select(0, idx), keys, seed, T, coupling=coupling,
                                       constraint=bound, resample=resample)
            constraint.record(bound, res, sampler.thick_x_new)
            flat[((sl[:m] - s0) * N + sm[:m]).to(device)] = res[:m, 0]
        mean[s0:s1], std[s0:s1] = ops.ensemble_stats(out, scale, shift, lo, hi)
        if qmaps is not None:
            qmaps[:, s0:s1] = ops.ensemble_quantiles(out, quantiles, scale, shift, lo, hi)
    res = (mean, std, every) if return_samples else (mean, std)
    return res if qmaps is None else res + (qmaps,)


def lockstep_bytes(N, n, size, m=0):
    """What GraphSampler.sample_lockstep holds for N samples of n slices: the state and the steps' results, 2 N n S^2 x 4 bytes, and the
    constraint's workspace of m rows per sample."""
    return (2 * N * n + N * m) * size * size * 4


def _sample_lockstep(sampler, conds, constraint, N, n, size, seed, T, slice_offset, coupling, resample, every):
    """sample_ensemble under a constraint that couples the whole stack: rows sample-major (row j n + i: slice i of sample j), one
    GraphSampler.sample_lockstep over them, -> the samples [n,N,S,S] (into `every` when given).  The memory is counted first."""
    device = conds[0].device
    need = lockstep_bytes(N, n, size, getattr(constraint, 'm', 0))
    free = torch.cuda.mem_get_info(device)[0]
    if need > free:
        raise ValueError(f'sample_ensemble: a constraint over the whole stack keeps all {N} x {n} samples on the device, {need / 2 ** 30:.2f} GiB '
                         f'with {free / 2 ** 30:.2f} GiB free: lower --num_samples')
    sl = torch.arange(n, dtype=torch.int64).repeat(N)
    sm = torch.arange(N, dtype=torch.int64).repeat_interleave(n)
    keys = torch.stack([sl + slice_offset, sm], 1)
    X = sampler.sample_lockstep(conds, keys, seed, T, constraint=constraint, coupling=coupling, resample=resample, cond_index=sl)
    constraint.record_volume(X, sampler.lockstep_x_new)
    out = every if every is not None else torch.empty(n, N, size, size, device=device, dtype=torch.float32)
    out.copy_(X.view(N, n, size, size).transpose(0, 1))
    return out


# ---------------------------------------------------------------------------------------------------
# the volume pipeline's flags for the order statistics (mudiff_hip.volume, mudiff_hip.cohort)
# ---------------------------------------------------------------------------------------------------
def quantile_suffix(q):
    """The file-name suffix of a fraction's map: the fraction x 1000, zero-padded (0.05 -> '_q050', 0.5 -> '_q500', 0.975 -> '_q975')."""
    return f'_q{int(round(float(q) * 1000.0)):03d}'


class QuantilePlan:
    """What --ensemble_quantiles, --ensemble_center and --coverage ask of one run: `computed`, the ascending fractions one
    ops.ensemble_quantiles call makes; `written`, those that get a file of their own (--ensemble_quantiles' and --coverage's);
    `center`, 'mean' or 'median' (the median then goes to predicted_<t>.nii.gz); `coverage`, None or (q_lo, q_hi)."""

    def __init__(self, asked, center, coverage):
        self.asked, self.center, self.coverage = tuple(asked), center, coverage
        self.written = tuple(sorted(set(self.asked) | set(coverage or ())))
        self.computed = tuple(sorted(set(self.written) | ({0.5} if center == 'median' else set())))

    def index(self, q):
        return self.computed.index(q)


def quantile_plan(args):
    """The QuantilePlan of a parsed namespace (check_flags' ValueError on a bad combination), or None when none of the three flags is set:
    the run is then exactly the one it was before they existed."""
    asked = getattr(args, 'ensemble_quantiles', None)
    center = getattr(args, 'ensemble_center', None) or 'mean'
    coverage = getattr(args, 'coverage', None)
    if asked is None and center == 'mean' and coverage is None:
        return None
    in_range = lambda v: math.isfinite(v) and 0.0 <= v <= 1.0      # noqa: E731
    if asked is not None:
        asked = [float(v) for v in asked]
        if not 1 <= len(asked) <= MAX_QUANTILES or not all(in_range(v) for v in asked):
            raise ValueError(f'--ensemble_quantiles takes 1 to {MAX_QUANTILES} fractions in [0, 1], got {asked}')
        if any(b <= a for a, b in zip(asked, asked[1:])):
            raise ValueError(f'--ensemble_quantiles: the fractions must be strictly increasing, got {asked}')
    if center not in ('mean', 'median'):
        raise ValueError(f"--ensemble_center must be 'mean' or 'median', got {center!r}")
    if coverage is not None:
        coverage = tuple(float(v) for v in coverage)
        if len(coverage) != 2 or not all(in_range(v) for v in coverage):
            raise ValueError(f'--coverage takes two fractions Q_LO Q_HI in [0, 1], got {list(coverage)}')
        if coverage[0] >= coverage[1]:
            raise ValueError(f'--coverage: Q_LO must be below Q_HI, got {coverage[0]:g} and {coverage[1]:g}')
    flag = '--ensemble_quantiles' if asked is not None else '--coverage' if coverage is not None else '--ensemble_center median'
    N = getattr(args, 'num_samples', None)
    if N is None:
        raise ValueError(f'{flag} needs --num_samples (the quantiles are taken over an ensemble)')
    if N > MAX_QUANTILE_SAMPLES:
        raise ValueError(f'{flag} needs --num_samples <= {MAX_QUANTILE_SAMPLES} (got {N})')
    if coverage is not None and getattr(args, 'gt_volume', None) is None and not getattr(args, 'score', False):
        raise ValueError('--coverage needs --gt_volume (--score on a cohort): the interval is counted against a ground truth')
    plan = QuantilePlan(asked or (), center, coverage)
    if len(plan.computed) > MAX_QUANTILES:
        raise ValueError(f'--ensemble_quantiles, --coverage and --ensemble_center median ask for {len(plan.computed)} quantiles together: '
                         f'at most {MAX_QUANTILES}')
    names = [quantile_suffix(q) for q in plan.written]
    if len(set(names)) != len(names):
        raise ValueError(f'{flag}: two fractions of {list(plan.written)} round to one file name ({", ".join(names)})')
    return plan


def done_suffix(args):
    """What a [done] line gains under the flags (nothing without them)."""
    plan = quantile_plan(args)
    if plan is None:
        return ''
    return (' | center=median' if plan.center == 'median' else '') + (
        ' | quantiles=' + ','.join(format(q, 'g') for q in plan.written) if plan.written else '')


def add_flags(p):
    p = p.later() if hasattr(p, 'later') else p          # volume.VolumeParser: the lists of the parsers before this one are pinned
    p.add_argument('--ensemble_quantiles', type=float, nargs='+', default=None, metavar='Q',
                   help='with --num_samples N <= 64: 1 to 8 strictly increasing fractions in [0, 1]; the per-voxel quantile of the '
                        "[0,1]-mapped samples at each goes to predicted_<t>_q<1000 Q>.nii.gz (0.05 -> _q050) through everything the mean's "
                        'volume goes through (mudiff_hip.ensemble, DESIGN.md section 5.24)')
    p.add_argument('--ensemble_center', type=str, default='mean', choices=['mean', 'median'],
                   help="what an ensemble writes to predicted_<t>.nii.gz, and so what --gt_volume scores and --through_plane measures: the "
                        "per-voxel mean (default) or, with 'median', the 0.5 quantile; _std stays the std about the mean")
    p.add_argument('--coverage', type=float, nargs=2, default=None, metavar=('Q_LO', 'Q_HI'),
                   help='with --num_samples and --gt_volume: write the two quantile maps and count how often the ground truth lies between '
                        'them, per region, on the GPU (mudiff_hip.volume_coverage) -> coverage_<t>.json and one [coverage] line per region; '
                        'Q_HI - Q_LO is the mass between two sample quantiles, not a guaranteed coverage')
