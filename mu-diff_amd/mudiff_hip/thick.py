"""Sample a target that was acquired with thick slices (--known_thick; csrc/slab.hip: mud_slab_constrain, mud_slab_average; DESIGN.md
section 5.27).

--known_volume keeps acquired voxels and --known_kspace acquired Fourier coefficients of each slice.  The most common way a contrast is
partly there is a third one: the target is a 2D multi-slice scan with thick slices (5 mm, perhaps with a gap) while the conditioning
contrasts are 3D at 1 mm, so every thick slice is a weighted average of several thin slices of the grid that is predicted.  A synthesis
model guided by such a measurement is through-plane super-resolution.  With --known_thick L the thin slices of --known_volume K are
measured retrospectively and the sampler keeps the measured averages:

    K --known_region's road--> the prediction's grid --norm, resize--> k [n,S,S] --ops.slab_average--> y_j = sum_l w_l k_{z_j + l} --> sampler

A slab j is L consecutive thin slices from z_j = O + j (L + G) of the *volume* (--thick_offset O, --thick_gap G: unmeasured thin slices
between slabs), so --slice_half_range, shards and chunks do not move the slabs.  The weights w_l > 0 sum to 1 (--thick_profile: box, or
gauss with FWHM = L slices).  Slabs do not overlap, so A A^T is diagonal and the constraint is an exact orthogonal projection: after the
reverse step executed with t = i the slab average of x is replaced by that of q_sample(k, i), after the last by y itself, and everything
orthogonal to the profile is left as the model made it (GraphSampler.sample_keyed's `thick`, kind ops.KIND_THICK; the draw and
--known_resample: mudiff_hip.constraints, section 5.24a).

A slab is measured when every one of its slices lies in the sampled range, K is known on every pixel of every one of them (finite and
fully covered after resampling: known_region's sense) and --known_drop_slices names none of them: the flag then means `this thick slice
was not acquired`.  The slices of an unmeasured slab, the gap slices and a partial last slab are sampled freely.  --known_mask and
--known_kspace are refused.

The constraint couples the rows of a batch, so the batching keeps a measured (slab, sample) group inside one batch (`batches`): a batch
is closed early before a group that would not fit and padded as the last batch is.  The kernel sums in the table's order and the draws
are keyed, so the written bytes do not depend on --batch_size.

There is no final paste.  Consistency holds on the sampler's grid: thick_<t>.json lists, per slab, |A x - y| / |y| of the sampler's
result before it is mapped to [0,1] (the largest over an ensemble's samples).  It does not survive clipping, --resize_back, the median
or the quantile maps.  --thick_interp also writes thick_interp_<t>.nii.gz, what one would have without the model: piecewise linear along
z through (slab centre, y_j) over the measured slabs, constant beyond the first and last centre.

Scope: the retrospective model with non-overlapping profiles, K given on (or resampled onto) the thin grid and measured here - the
protocol section 5.26 uses for k-space.  A NIfTI that is itself thick (its own slice spacing, slabs that cut thin slices in fractions,
overlapping profiles: a banded A A^T) is --known_thick_volume's (mudiff_hip.thick_volume, section 5.29: a constraint of its own, over
the whole stack).  Thick slices that are also undersampled in-plane are --known_multislice's (mudiff_hip.multislice, section 5.28), not
this flag's with --known_kspace.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from .constraints import batches      # noqa: F401  (the batching that keeps a slab whole)
from .constraints import Constraint, SlabRows, need_keyed_seed, need_known_volume, relative_residual
from .thick_volume import interpolate

PROFILES = ('box', 'gauss')
MAX_L = 16                           # ops.SLAB_MAX_MEMBERS


def add_flags(p):
    p = p.later() if hasattr(p, 'later') else p          # volume.VolumeParser: the lists of the parsers before this one are pinned
    p.add_argument('--known_thick', type=int, default=None, metavar='L',
                   help=f'with --known_volume K: K was acquired with thick slices.  Every L (1..{MAX_L}) consecutive thin slices of K are '
                        'averaged under the slice profile and the sampler re-imposes those averages after every reverse step '
                        '(mudiff_hip.thick, DESIGN.md section 5.27); --known_drop_slices then means `this thick slice was not acquired`')
    p.add_argument('--thick_gap', type=int, default=None, metavar='G', help='with --known_thick: unmeasured thin slices between slabs (default 0)')
    p.add_argument('--thick_offset', type=int, default=None, metavar='O',
                   help='with --known_thick: the thin slice of the volume where the first slab starts (default 0)')
    p.add_argument('--thick_profile', type=str, default=None, choices=list(PROFILES),
                   help='with --known_thick: the slice profile, box (equal weights, the default) or gauss (FWHM = L slices)')
    p.add_argument('--thick_interp', action='store_true',
                   help='with --known_thick: also write thick_interp_<t>.nii.gz, the thick slices interpolated linearly along z (what one '
                        'would have without the model; scored too under --gt_volume)')


def thickness(flag, L):
    """--known_thick's / --multislice_thick's L, refused first of all of slab_options' checks."""
    if int(L) != L or not 1 <= L <= MAX_L:
        raise ValueError(f'{flag} must be an integer in [1, {MAX_L}] (thin slices per slab), got {L}')
    return int(L)


def slab_options(flag, prefix, L, gap, offset, profile):
    """The slab layout of --known_thick (`flag`; its dependents are `prefix`gap, ...) or --multislice_thick as given (None: the default)
    -> dict(L, gap, offset, profile).  ValueError naming the flag for a bad value."""
    L = thickness(flag, L)
    gap, offset = 0 if gap is None else gap, 0 if offset is None else offset
    if int(gap) != gap or gap < 0:
        raise ValueError(f'{prefix}gap must be an integer >= 0, got {gap}')
    if int(offset) != offset or offset < 0:
        raise ValueError(f'{prefix}offset must be an integer >= 0, got {offset}')
    profile = 'box' if profile is None else profile
    if profile not in PROFILES:
        raise ValueError(f'{prefix}profile must be one of {PROFILES}, got {profile!r}')
    return dict(L=L, gap=int(gap), offset=int(offset), profile=profile)


def options_from(args):
    """A namespace's --known_thick / --thick_* flags (any may be missing) -> None without --known_thick, else dict(L, gap, offset,
    profile, interp).  ValueError, naming the flag, for a dependent flag without --known_thick, --known_thick without --known_volume (a
    cohort's namespace excepted: its K is the manifest's `known` column) or with --known_kspace or --known_mask, and a bad value."""
    L = getattr(args, 'known_thick', None)
    gap, offset, profile = (getattr(args, f, None) for f in ('thick_gap', 'thick_offset', 'thick_profile'))
    interp = bool(getattr(args, 'thick_interp', False))
    if L is None:
        for flag, given in (('--thick_gap', gap is not None), ('--thick_offset', offset is not None), ('--thick_profile', profile is not None),
                            ('--thick_interp', interp)):
            if given:
                raise ValueError(f'{flag} needs --known_thick')
        return None
    thickness('--known_thick', L)                         # (a bad L is named before a missing --known_volume)
    need_known_volume(args, '--known_thick')
    if getattr(args, 'known_kspace', None) is not None:
        raise ValueError('--known_thick cannot be combined with --known_kspace (in-plane undersampling of thick slices is out of scope)')
    if getattr(args, 'known_mask', None) is not None:
        raise ValueError('--known_thick cannot be combined with --known_mask (a thick slice is measured whole; use --known_drop_slices '
                         'for thick slices that were not acquired)')
    slab = slab_options('--known_thick', '--thick_', L, gap, offset, profile)
    need_keyed_seed(args, '--known_thick')
    return dict(slab, interp=interp)


# ---------------------------------------------------------------------------------------------------
# the profile and the layout: numpy, functions of the flags alone
# ---------------------------------------------------------------------------------------------------
def profile_weights(L, profile='box'):
    """fp64 [L], w_l > 0, sum 1.  box: 1 / L; gauss: w_l ~ exp(-4 ln 2 (l - (L - 1) / 2)^2 / L^2), a Gaussian of FWHM = L slices."""
    L = int(L)
    if not 1 <= L <= MAX_L:
        raise ValueError(f'profile_weights: L must be in [1, {MAX_L}], got {L}')
    if profile == 'box':
        w = np.ones(L, np.float64)
    elif profile == 'gauss':
        d = np.arange(L, dtype=np.float64) - (L - 1) / 2.0
        w = np.exp(-4.0 * math.log(2.0) * d * d / float(L * L))
        w = 0.5 * (w + w[::-1])                          # symmetric to the bit
    else:
        raise ValueError(f'profile_weights: profile must be one of {PROFILES}, got {profile!r}')
    return w / w.sum()


def layout(Z, L, gap=0, offset=0):
    """The slabs of a volume of Z thin slices: [(first, last, complete)] with first = offset + j (L + gap) < Z; a last slab that the volume
    cuts short has last = Z - 1 and complete False (it is never measured)."""
    Z, L, gap, offset = int(Z), int(L), int(gap), int(offset)
    if L < 1 or gap < 0 or offset < 0:
        raise ValueError(f'layout: need L >= 1, gap >= 0 and offset >= 0, got {L}, {gap}, {offset}')
    return [(z, min(z + L, Z) - 1, z + L <= Z) for z in range(offset, Z, L + gap)]


# ---------------------------------------------------------------------------------------------------
# the measurement of one prediction
# ---------------------------------------------------------------------------------------------------
class SlabbedMeasurement(Constraint):
    """What the measurements of slabs share (ThickMeasurement; multislice.MultisliceMeasurement): `y` [G,S,S] on the device, one
    measurement per measured slab of the n local slices; the slabs - `starts` [G], `group_of` int [n], `weights`, `gains` fp32 [L], `L` -
    and what follows from them alone: the units that must share a batch, where an ensemble's chunk may end, and the member rows of a
    batch's groups; `report`, `resample` (--known_resample), `options`; and the residuals that `record` collects and `finish` reports.
    A measurement says what it compares in `difference`."""

    def __init__(self, y, starts, n, weights, report, resample, options):
        from . import ops
        self.y, self.report, self.resample, self.options = y, report, int(resample), options
        self.y_norm = torch.linalg.vector_norm(y.flatten(1), dim=1) if y.shape[0] else torch.zeros(0, device=y.device)
        self.residual = torch.zeros(y.shape[0], device=y.device, dtype=torch.float32)
        self.x_norm = torch.zeros_like(self.residual)
        self.starts, self.n = [int(s) for s in starts], int(n)
        self.weights = np.ascontiguousarray(weights, dtype=np.float32)
        self.gains = ops.slab_gains(self.weights)[0]
        self.L = int(self.weights.shape[0])
        self.group_of = np.full(self.n, -1, np.int64)
        for g, s in enumerate(self.starts):
            self.group_of[s:s + self.L] = g

    def units(self, lo=0, hi=None):
        """The local slices lo..hi-1 in order as batches() takes them: a measured slab's L slices together, every other slice alone.
        ValueError when the range cuts a measured slab."""
        hi = self.n if hi is None else hi
        out, i = [], lo
        while i < hi:
            g = int(self.group_of[i])
            if g < 0:
                out.append([i])
                i += 1
                continue
            s = self.starts[g]
            if s < lo or s + self.L > hi or i != s:
                raise ValueError(f'thick slices: the range {lo}..{hi - 1} cuts the measured slab {s}..{s + self.L - 1}')
            out.append(list(range(s, s + self.L)))
            i = s + self.L
        return out

    def chunk_end(self, s0, s1):
        """An ensemble's chunk ends before a measured slab that it would cut."""
        chunk = s1 - s0
        if s1 < self.n and self.group_of[s1] >= 0 and self.group_of[s1] == self.group_of[s1 - 1]:
            s1 = self.starts[int(self.group_of[s1])]
        if s1 <= s0:
            raise ValueError(f'sample_ensemble: a chunk of {chunk} slices is smaller than a slab of {self.L} thin slices')
        return s1

    def group_rows(self, slices, samples=None, m=None):
        """The batch whose row r holds local slice slices[r] of sample samples[r] (None: all 0); a row from m on, or with slice -1, is
        padding, in no group -> (members int32 [groups, L], the measured slab of each group).  Every measured slab that a row touches
        must be in the batch whole, per sample; its rows enter the table in slice order."""
        samples = [0] * len(slices) if samples is None else [int(s) for s in samples]
        found = {}
        for r, (i, j) in enumerate(zip(slices[:m], samples)):
            g = int(self.group_of[i]) if i >= 0 else -1
            if g >= 0:
                found.setdefault((g, j), {})[int(i) - self.starts[g]] = r
        members, gids = [], []
        for (g, j), rows in found.items():
            if sorted(rows) != list(range(self.L)):
                raise ValueError(f'thick slices: the batch holds {len(rows)} of the {self.L} thin slices of a measured slab (sample {j})')
            members.append([rows[l] for l in range(self.L)])
            gids.append(g)
        return np.asarray(members, np.int32).reshape(len(members), self.L), gids

    def record(self, bound, x, x_new=None):
        """x [B,1,S,S]: what the sampler returned (in [-1,1], before any map) for the batch that for_rows bound = (the operands, which
        end in members, weights, gains; the measured slab of each group): keeps, per slab, the largest |difference| / |y| seen (an
        ensemble records every sample), and the largest |A |x_new|| of what the last constraint was given (GraphSampler.thick_x_new; x
        itself without it): with |y|, what the residual's rounding scales with."""
        from . import ops
        operands, gids = bound
        if gids.numel() == 0:
            return
        members, weights = operands[-3], operands[-2]
        x_new = x if x_new is None else x_new
        ax = ops.slab_average(x_new[:, 0].abs().contiguous(), members, weights)
        self.x_norm.scatter_reduce_(0, gids, torch.linalg.vector_norm(ax.flatten(1), dim=1), 'amax')
        d = self.difference(operands, ops.slab_average(x[:, 0].contiguous(), members, weights))
        self.residual.scatter_reduce_(0, gids, relative_residual(d.flatten(1), self.y_norm.index_select(0, gids)), 'amax')

    def finish(self):
        """The report with the residuals put in (None for a slab that was not measured)."""
        res, yn, xn = self.residual.cpu().tolist(), self.y_norm.cpu().tolist(), self.x_norm.cpu().tolist()
        g = 0
        for s in self.report['slabs']:
            s['residual'], s['y_norm'], s['x_norm'] = (res[g], yn[g], xn[g]) if s['measured'] else (None, None, None)
            g += 1 if s['measured'] else 0
        self.report['max_residual'] = max(res, default=None)
        return self.report


class ThickMeasurement(SlabbedMeasurement):
    """What the samplers take for one prediction of n thin slices (the sampled range s0..s1; local index i = slice s0 + i): `y` fp32
    [G,S,S] on the device, the measured slabs' averages; `starts` [G], each measured slab's first local index; `group_of` int [n], the
    measured slab of a slice or -1; `weights`, `gains` fp32 [L] (numpy: the host tables of ops.slab_constrain); `report`: thick_<t>.json;
    `resample`: --known_resample.  A later intake of really thick data only has to fill the same fields."""

    tag, baseline_through_plane = 'thick', True
    done_suffix = lambda self: suffix(self)      # noqa: E731
    baseline = lambda self: ('thick_interp', self.interpolated()) if self.options['interp'] else None      # noqa: E731

    def for_rows(self, slices, samples=None, m=None):
        """group_rows' batch -> constraints.SlabRows = (GraphSampler.sample_keyed's `thick` tuple, the measured slab of each group)."""
        members, gids = self.group_rows(slices, samples, m)
        idx = torch.as_tensor(gids, dtype=torch.int64, device=self.y.device)
        return SlabRows((self.y.index_select(0, idx), members, self.weights, self.gains), idx)

    def difference(self, operands, ax):
        """A x - y of the batch's groups: `record` keeps |A x - y| / |y|."""
        return ax - operands[0]

    def interpolated(self):
        """interpolate_slabs of the slab averages."""
        return interpolate_slabs(self.y, self.starts, self.L, self.n)


def interpolate_slabs(y, starts, L, n):
    """y fp32 [G,S,S], one image per measured slab of L slices from local index starts[j] -> [n,S,S] in [-1,1] terms:
    thick_volume.interpolate through the slab centres - the thick slices as one would resample them without the model."""
    return interpolate(y, np.asarray(starts, np.float64) + (L - 1) / 2.0, n)


def select_slabs(region, s0, s1, S, options, device):
    """known_region.KnownRegion and the slab layout of `options` (L, gap, offset, profile) for the thin slices s0..s1 on the S x S grid
    -> (k [n,1,S,S]: K as the sampler sees it; starts: the measured slabs' first local index; slabs: every slab of the volume as the
    report lists it; w32: the profile, fp32 [L]; and the fields every report of slabs holds, in two dicts: those before `slabs` and
    those after it).  A slab is measured when it is complete, inside the range, and K is known on every
    pixel of every one of its slices."""
    from . import known_region as KR
    L = options['L']
    k, vmask = KR.sampler_inputs(region, s0, s1, S, device)                      # [n,1,S,S] each, resized like the conditions
    whole = [bool(v) for v in (vmask.flatten(1).min(1).values != 0).cpu().tolist()]      # every pixel of the slice known
    w = profile_weights(L, options['profile'])
    slabs, starts = [], []
    for first, last, complete in layout(region.mask.shape[2], L, options['gap'], options['offset']):
        measured = complete and first >= s0 and last <= s1 and all(whole[first - s0:last - s0 + 1])
        slabs.append(dict(first=first, last=last, measured=bool(measured)))
        if measured:
            starts.append(first - s0)
    w32 = w.astype(np.float32)
    head = dict(L=L, gap=options['gap'], offset=options['offset'], profile=options['profile'], weights=[float(v) for v in w32],
                sum_w2=float((w32.astype(np.float64) ** 2).sum()), image_size=S, slab=[s0, s1])
    tail = dict(measured_slabs=len(starts), drop_slices=region.report['drop_slices'], resample=region.resample,
                resampled=region.report['resampled'])
    return k, starts, slabs, w32, head, tail


def measure(region, s0, s1, size, options, device):
    """known_region.KnownRegion (K on the prediction's grid: --norm applied, its known mask = coverage AND finite AND not dropped AND
    sampled range) -> ThickMeasurement for the thin slices s0..s1 on the S x S sampler grid."""
    from . import ops
    S, L = int(size), options['L']
    k, starts, slabs, w32, head, tail = select_slabs(region, int(s0), int(s1), S, options, device)
    if starts:
        members = np.asarray([list(range(s, s + L)) for s in starts], np.int32)
        y = ops.slab_average(k[:, 0].contiguous(), members, w32)
    else:
        y = torch.zeros(0, S, S, device=device, dtype=torch.float32)
    return ThickMeasurement(y, starts, int(k.shape[0]), w32, dict(head, slabs=slabs, **tail), region.resample, options)


def suffix(measurement):
    """What a [done] line gains (nothing without --known_thick)."""
    if measurement is None:
        return ''
    r = measurement.report
    return f" | thick={r['L']}+{r['gap']} {r['profile']} ({r['measured_slabs']}/{len(r['slabs'])} slabs)"

