"""What the ways of sampling a partly acquired target share (--known_volume, --known_kspace, --known_thick, --known_multislice,
--known_sense): after every reverse step the result is projected onto what was measured, at that step's noise level, with a
keyed draw.

A *prediction-level* constraint (Constraint: KnownVoxels here, kspace.KSpaceMeasurement, thick.ThickMeasurement,
multislice.MultisliceMeasurement, sense.SenseMeasurement) describes the n slices one prediction samples; volume.predict_slices and ensemble.sample_ensemble form
their batches from it and know nothing else of it.  Its for_rows gives the *batch-level* constraint of one captured batch (KnownRows,
KSpaceRows, SlabRows, SlabKSpaceRows, SenseRows): `check(sampler)`, once, and `apply(sampler, x_new, keys_dev, seed, step, clean)`, one unchecked
launch into sampler.x per executed step, for GraphSampler.sample_keyed.

A constraint that couples the whole stack along z (thick_volume.BandMeasurement, --known_thick_volume; section 5.29) has no batch-level
form: it declares `lockstep` and the samplers hand it the whole state of the prediction after every step
(GraphSampler.sample_lockstep).

The pieces a mode takes from here instead of writing them again: level_tables (what every apply hands its launch), _kspace_batch and
_slab_tables_fit (the checks of a batch measured in k-space, and of slab tables against a batch), relative_residual (the |d| / |y| of
every report), and for the flags need_known_volume and need_keyed_seed.  Next to them: thick.SlabbedMeasurement, thick.select_slabs and
thick.slab_options for anything measured in slabs, kspace.pattern_options for a sampling pattern, thick_volume.interpolate for the
through-plane baseline."""
from __future__ import annotations

import collections
import json
import os

import torch

from . import ops


def batches(units, B, flag='--batch_size'):
    """units: the run's items in order, grouped: a list of lists, each inner list the items that must share a batch (a measured slab's
    thin slices; one item for a free slice).  -> [(items of the batch, in order)] of at most B items each: a batch is closed early before
    a unit that would not fit.  ValueError naming `flag` for a unit longer than B."""
    out, cur = [], []
    for u in units:
        if len(u) > B:
            raise ValueError(f'{flag} {B} is smaller than a slab of {len(u)} thin slices: a measured slab must travel in one batch')
        if len(cur) + len(u) > B:
            out.append(cur)
            cur = []
        cur = cur + list(u)
    if cur:
        out.append(cur)
    return out


class Constraint:
    """A prediction-level constraint over the local slices 0..n-1, and its defaults: no constraint at all (FREE).
    `for_rows(slices, samples, m)` -> the batch-level constraint of the batch whose row r holds local slice slices[r] of sample samples[r]
    (None: all 0); the first m rows are real, the others padding that repeats the last item.  `record(bound, x, x_new)` takes what the
    sampler returned for that batch, x [B,1,S,S], and the sampler's thick_x_new.  A measurement with a report of its own
    (volume._measurement_outputs) also declares `tag` (its log tag and its report's file name; `finish()` is the report), `baseline()`
    (None, or (file name stem, [n,S,S] map in [-1,1] terms): what one would have without the model) and `baseline_through_plane`."""
    n, resample, tag, baseline_through_plane = None, 1, None, False
    # True: the constraint couples the whole stack along z, so no batch can hold what it couples.  The samplers then advance every
    # (slice, sample) of the prediction one reverse step and constrain them all at once (GraphSampler.sample_lockstep, DESIGN.md
    # section 5.29) through `check_volume(sampler, rows)`, once, `apply_volume(sampler, x_new, x, keys_dev, seed, step, clean)`, one
    # launch over the [rows,1,S,S] state x_new -> x per executed step (rows sample-major: row j n + i is slice i of sample j; the
    # rows' levels: sampler.t_rows), and `record_volume(x, x_new)` for what the sampler returned.
    lockstep = False

    def done_suffix(self):
        return ''                            # what a [done] line gains

    def over(self, n, who):
        if self.n not in (None, n):
            raise ValueError(f'{who}: the constraint is of {self.n} slices, the conditions of {n}')

    def units(self, lo, hi):
        return [[i] for i in range(lo, hi)]  # the local slices lo..hi-1 in order, grouped into the lists that must share a batch

    def chunk_end(self, s0, s1):
        return s1                            # where an ensemble's chunk that starts at s0 and would end before s1 may end

    def for_rows(self, slices, samples, m):
        return None

    def record(self, bound, x, x_new):
        return None

    def write_json(self, output_dir, target):
        path = os.path.join(output_dir, f'{self.tag}_{target.lower()}.json')
        with open(path, 'w') as f:
            json.dump(self.finish(), f, indent=1)
        return path


FREE = Constraint()


class KnownVoxels(Constraint):
    """--known_volume for the samplers: known_region.sampler_inputs' pair.  A padded row repeats the last item's stack and mask."""

    def __init__(self, known, mask, resample=1):
        self.known, self.mask, self.resample = known, mask, int(resample)
        self.n = None if known is None else int(known.shape[0])

    def for_rows(self, slices, samples, m):
        idx = torch.as_tensor(slices, dtype=torch.int64, device=self.known.device)
        return KnownRows(self.known.index_select(0, idx), self.mask.index_select(0, idx))


def relative_residual(d, den):
    """|d| / den over d's last axis, 0 where den is 0: the data-consistency residual of every measurement's report (d [..., k, len]
    against den [k], the measurements' norms)."""
    r = torch.linalg.vector_norm(d, dim=-1)
    return torch.where(den > 0, r / den.clamp_min(1e-30), torch.zeros_like(r))


def need_known_volume(args, flag):
    """`flag` measures --known_volume K; a cohort's namespace is excepted: its K is the manifest's `known` column."""
    cohort = getattr(args, 'manifest', None) is not None or getattr(args, 'brats_root', None) is not None
    if getattr(args, 'known_volume', None) is None and not cohort:
        raise ValueError(f'{flag} needs --known_volume')


def need_keyed_seed(args, flag, why='its draws are keyed'):
    if not 0 <= int(getattr(args, 'seed', 0)) < 1 << 64:
        raise ValueError(f'{flag} needs a --seed in [0, 2^64) ({why})')


def of_prediction(who, constraint, known, kspace, thick, resample):
    """The keywords of volume.predict_slices / ensemble.sample_ensemble, `known` = (known, mask) -> (the one prediction-level constraint
    or FREE, resample: a `constraint`'s own, else the keyword).  ValueError for more than one."""
    given = [v for v in (constraint, known, kspace, thick) if v is not None]
    if len(given) > 1:
        raise ValueError(f'{who}: known, kspace and thick are mutually exclusive')
    if not given:
        return FREE, 1
    con = given[0] if known is None else KnownVoxels(known[0], known[1], resample)
    return con, con.resample if constraint is not None else resample


# ---------------------------------------------------------------------------------------------------
# what the batch-level constraints share: `sampler` is the GraphSampler (its B, H, W, x, t and level tables)
# ---------------------------------------------------------------------------------------------------
def level_tables(sampler):
    """(a_s_cum, sigmas_cum): the two tables every constraint launch takes after its t and offset."""
    return sampler._diffusion_tables()[:2]


def _kspace_batch(word, sampler, y, mask, slab=None):
    """A batch measured in k-space: the sampler's grid is square and one the transform takes, y is complex64 [count,S,S] and mask uint8
    [1 or count,S,S] -> (y, mask on the sampler's device, the slab tables or None).  count: B, or with `slab` = (members, weights, gains)
    the groups of ops.slab_tables of it.  Leaves the complex workspace on the sampler: one per sampler, [B,S,S] (groups <= B)."""
    B, H, W = sampler.B, sampler.H, sampler.W
    if H != W or not ops.kspace_size_ok(H):
        raise ValueError(f'GraphSampler.sample_keyed: {word} needs a square grid whose size is a power of two in [16, 512], got {H} x {W}')
    tab = None if slab is None else ops.slab_tables(*slab)
    want = (B if tab is None else tab[0].shape[0], H, W)
    if y.dtype != torch.complex64 or tuple(y.shape) != want or mask.dtype != torch.uint8 or tuple(mask.shape) not in (want, (1,) + want[1:]):
        raise ValueError(f'GraphSampler.sample_keyed: {word} = (y complex64 {want}, mask uint8 [1 or {want[0]}, {H}, {W}]'
                         f'{"" if tab is None else ", ..."}), got {y.dtype} {tuple(y.shape)} and {mask.dtype} {tuple(mask.shape)}')
    if getattr(sampler, '_ks_work', None) is None:
        sampler._ks_work = torch.empty((B, H, W), device=sampler.x.device, dtype=torch.complex64)
    return y.to(sampler.x.device).contiguous(), mask.to(sampler.x.device).contiguous(), tab


def _slab_tables_fit(word, sampler, tab):
    """Slab tables against the batch: at most B groups, of at most ops.SLAB_MAX_MEMBERS rows each, all of them rows of the batch."""
    (groups, L), B, top = tab[0].shape, sampler.B, int(tab[0].max(initial=-1))
    if groups > B or L > ops.SLAB_MAX_MEMBERS or top >= B:
        raise ValueError(f'GraphSampler.sample_keyed: {word} names {groups} groups of {L} rows up to row {top} for a batch of {B} (at most '
                         f'{ops.SLAB_MAX_MEMBERS} rows a group)')


class KnownRows(collections.namedtuple('KnownRows', 'known mask')):
    """GraphSampler.sample_keyed's `known`, `known_mask`: [B,1,H,W] fp32 and uint8."""

    def check(self, sampler):
        (known, mask), shape = self, tuple(sampler.x.shape)
        if mask is None:
            raise ValueError('GraphSampler.sample_keyed: known needs known_mask')
        if tuple(known.shape) != shape or tuple(mask.shape) != shape or mask.dtype != torch.uint8:
            raise ValueError(f'GraphSampler.sample_keyed: known (fp32) and known_mask (uint8) must be {shape}, got '
                             f'{tuple(known.shape)} and {mask.dtype} {tuple(mask.shape)}')
        self.dev = known.to(sampler.x.device, torch.float32).contiguous(), mask.to(sampler.x.device).contiguous()

    def apply(self, sampler, x_new, keys_dev, seed, step, clean):
        ops.known_constrain_into(sampler.x, x_new, *self.dev, keys_dev, seed, step, ops.KIND_KNOWN, sampler.t, 0, *level_tables(sampler), clean=clean)


class KSpaceRows(collections.namedtuple('KSpaceRows', 'y mask idx', defaults=(None,))):
    """GraphSampler.sample_keyed's `kspace`: y complex64 [B,S,S], mask uint8 [1 or B,S,S].  `idx`: the local slices of the real rows
    (KSpaceMeasurement.for_rows; None from the keyword)."""

    def check(self, sampler):
        self.dev = _kspace_batch('kspace', sampler, self.y, self.mask)[:2]

    def apply(self, sampler, x_new, keys_dev, seed, step, clean):
        ops.kspace_constrain_into(sampler.x, x_new, *self.dev, sampler._ks_work, keys_dev, seed, step, ops.KIND_KSPACE, sampler.t, 0,
                                  *level_tables(sampler), clean=clean)


class SlabRows(collections.namedtuple('SlabRows', 'thick gids')):
    """GraphSampler.sample_keyed's `thick` = (y fp32 [groups,H,W], members, weights, gains), and `gids`: the measured slab of each group
    (ThickMeasurement.for_rows; None from the keyword)."""

    def check(self, sampler):
        y, members, weights, gains = self.thick
        tab = ops.slab_tables(members, weights, gains)
        want = (tab[0].shape[0], sampler.H, sampler.W)
        if y.dtype != torch.float32 or tuple(y.shape) != want:
            raise ValueError(f'GraphSampler.sample_keyed: thick y must be fp32 {want}, got {y.dtype} {tuple(y.shape)}')
        _slab_tables_fit('thick', sampler, tab)
        self.dev = y.to(sampler.x.device).contiguous(), tab

    def apply(self, sampler, x_new, keys_dev, seed, step, clean):
        ops.slab_constrain_into(sampler.x, x_new, *self.dev, keys_dev, seed, step, ops.KIND_THICK, sampler.t, 0, *level_tables(sampler), clean=clean)
        sampler.thick_x_new = x_new          # what the last constraint was given (the graph's own buffer, until the next replay)


class SlabKSpaceRows(collections.namedtuple('SlabKSpaceRows', 'multislice gids', defaults=(None,))):
    """The batch-level constraint of accelerated thick slices, for GraphSampler.sample_keyed(constraint=):
    `multislice` = (y complex64 [groups,S,S], mask uint8 [1 or groups,S,S], members, weights, gains), the tables as SlabRows', and `gids`:
    the measured slab of each group (multislice.MultisliceMeasurement.for_rows; None from a caller's own tuple)."""

    def check(self, sampler):
        y, mask, *slab = self.multislice
        dev = _kspace_batch('multislice', sampler, y, mask, slab)
        _slab_tables_fit('multislice', sampler, dev[2])
        self.dev = dev

    def apply(self, sampler, x_new, keys_dev, seed, step, clean):
        ops.slab_kspace_constrain_into(sampler.x, x_new, *self.dev, sampler._ks_work, keys_dev, seed, step, ops.KIND_MULTISLICE, sampler.t, 0,
                                       *level_tables(sampler), clean=clean)
        sampler.thick_x_new = x_new          # what the last constraint was given (the graph's own buffer, until the next replay)


class SenseRows(collections.namedtuple('SenseRows', 'ahy mask maps lam iters idx', defaults=(None,))):
    """The batch-level constraint of a target acquired accelerated on several coils, for GraphSampler.
    sample_keyed(constraint=): `ahy` fp32 [B,S,S] = A^H y, `mask` uint8 [1 or B,S,S] (as given: not symmetrised), `maps` complex64
    [Nc,S,S] or [1 or B,Nc,S,S], `lam` and `iters` of the proximal step; `idx`: the local slices of the real rows
    (sense.SenseMeasurement.for_rows; None from a caller's own tuple).  Leaves the workspace on the sampler (one per sampler and coil
    count) and, after every step, sampler.sense_x_new and sampler.sense_cg_res [B] (on itself: `x_new`, and `cg_max`, the largest
    sense_cg_res of the batch's steps so far)."""

    def check(self, sampler):
        B, H, W = sampler.B, sampler.H, sampler.W
        if H != W or not ops.kspace_size_ok(H):
            raise ValueError(f'GraphSampler.sample_keyed: sense needs a square grid whose size is a power of two in [16, 512], got {H} x {W}')
        ahy, mask, maps, lam, iters = self[:5]
        maps = maps[None] if maps.dim() == 3 else maps
        if ahy.dtype != torch.float32 or tuple(ahy.shape) != (B, H, W) or mask.dtype != torch.uint8 or tuple(mask.shape) not in ((B, H, W), (1, H, W)) or \
                maps.dtype != torch.complex64 or maps.dim() != 4 or maps.shape[0] not in (1, B) or tuple(maps.shape[2:]) != (H, W) or \
                not 1 <= maps.shape[1] <= ops.SENSE_MAX_COILS:
            raise ValueError(f'GraphSampler.sample_keyed: sense = (ahy fp32 {(B, H, W)}, mask uint8 [1 or {B}, {H}, {W}], maps complex64 '
                             f'[1 or {B}, 1..{ops.SENSE_MAX_COILS}, {H}, {W}], ...), got {ahy.dtype} {tuple(ahy.shape)}, {mask.dtype} '
                             f'{tuple(mask.shape)} and {maps.dtype} {tuple(maps.shape)}')
        if not (float(lam) >= 0.0 and float(lam) < float('inf')) or not 1 <= int(iters) <= ops.SENSE_MAX_ITERS:
            raise ValueError(f'GraphSampler.sample_keyed: sense needs a finite lambda >= 0 and iters in [1, {ops.SENSE_MAX_ITERS}], got {lam} and {iters}')
        need = ops.sense_ws_floats(B, maps.shape[1], H)
        if getattr(sampler, '_sense_work', None) is None or sampler._sense_work.numel() < need:
            sampler._sense_work = torch.empty(need, device=sampler.x.device, dtype=torch.float32)
            sampler.sense_cg_res = torch.zeros(B, device=sampler.x.device, dtype=torch.float32)
        dev = sampler.x.device
        self.dev = ahy.to(dev).contiguous(), mask.to(dev).contiguous(), maps.to(dev).contiguous(), float(lam), int(iters)

    def apply(self, sampler, x_new, keys_dev, seed, step, clean):
        ops.sense_constrain_into(sampler.x, x_new, *self.dev, sampler.sense_cg_res, sampler._sense_work, keys_dev, seed, step, ops.KIND_SENSE, sampler.t,
                                 0, *level_tables(sampler), clean=clean)
        sampler.sense_x_new = self.x_new = x_new      # what the last constraint was given (the graph's own buffer, until the next replay)
        self.cg_max = sampler.sense_cg_res.clone() if step == 0 else torch.maximum(self.cg_max, sampler.sense_cg_res)      # over all steps


def of_batch(constraint, known, known_mask, kspace, thick, resample):
    """The keywords of GraphSampler.sample_keyed (`thick`: a tuple, or an object with its attributes) -> the one batch-level constraint
    or None.  ValueError for more than one, for known_mask without known, and for resample != 1 with none."""
    given = [v for v in (constraint, known, kspace, thick) if v is not None]
    if len(given) > 1:
        raise ValueError('GraphSampler.sample_keyed: known, kspace and thick are mutually exclusive')
    if known is None and known_mask is not None or not given and resample != 1:
        raise ValueError('GraphSampler.sample_keyed: known_mask and resample need known (resample: or kspace, or thick)')
    if known is not None:
        return KnownRows(known, known_mask)
    if kspace is not None:
        return KSpaceRows(*kspace)
    if thick is not None:
        return SlabRows(tuple(thick) if isinstance(thick, (tuple, list)) else (thick.y, thick.members, thick.weights, thick.gains), None)
    return constraint
