"""Keep the acquired part of the target (--known_volume; csrc/known_region.hip: mud_known_constrain, mud_known_coverage; DESIGN.md section
5.25).

The target contrast is often partly there: a FLAIR that covers part of the head, a T1CE with a dozen slices ruined by motion.  With
--known_volume K the sampler re-imposes the acquired voxels at the matching noise level after every reverse step (RePaint, Lugmayr et al.
2022; GraphSampler.sample_keyed's `known`), so that the free region is sampled conditioned on them, and the written volume carries them
exactly:

    K [, M] --the road of --gt_volume / --eval_mask--> the prediction's grid --AND--> known region --> sampler (every step) --> final paste

K is the target contrast as far as it was acquired, M (--known_mask, optional) says which voxels of K to trust (non-zero), and
--known_drop_slices A:B takes whole slices of the prediction grid out (inclusive).  K is not co-registered: it must already lie in the
first input's frame, exactly as --gt_volume must.  Both go through volume_prepare.read_for_evaluation / evaluation_grid: reoriented by
their own affine under --reorient, resampled onto the prediction's grid under --regrid / --conform (K by --regrid_interp behind
--antialias, M by nearest neighbour); without those flags their shape must be the grid's.

The known region on the prediction grid is the AND of: mud_known_coverage of K's grid matrix (the voxels interpolated from acquired
voxels alone; all ones when K was not resampled), K finite, M non-zero (when given), the slice not dropped, the slice inside the slab.
K is normalised by --norm like any target, the percentiles or moments being those of K's own non-zero voxels - which differs from a full
acquisition's when little is known (unmeasured).  At the sampler's resolution (--image_size differs from the in-plane size) K is resized
like the conditions (ops.resize_bilinear) and a pixel is known where the bilinear resize of the *unknown* indicator is exactly 0: exact,
because a sum of zeros is zero.

The run draws with keys (global slice, 0) and --seed, as --slice_coupling does, so the result does not depend on --batch_size.  Before
writing, every written map gets a final paste on the output grid (mud_known_constrain with clean = 1), after --resize_back and before
--conform_back / --reorient_back: the mean, median and quantile maps take ops.to_range_0_1 of the normalised K at the known voxels, the
std takes 0.  known_<t>.json next to the prediction holds the voxel counts of each term, the known voxels per slice, the fraction of the
slab that is known and --known_resample; the [done] line gains ` | known=<fraction>[ x<R>]`; under --gt_volume the scores gain the regions
`known` (slab AND known) and `synthesised` (slab AND NOT known).
"""
from __future__ import annotations

import collections
import json
import os

import numpy as np
import torch

REGION_NAMES = ('known', 'synthesised')


def add_flags(p):
    p = p.later() if hasattr(p, 'later') else p          # volume.VolumeParser: the lists of the parsers before this one are pinned
    p.add_argument('--known_volume', type=str, default=None, metavar='K',
                   help='the target contrast as far as it was acquired (NIfTI, in the first input\'s frame: it is not co-registered): its '
                        'voxels are re-imposed at the matching noise level after every reverse step, so that the rest is sampled conditioned '
                        'on them, and the written prediction carries them exactly (mudiff_hip.known_region, DESIGN.md section 5.25)')
    p.add_argument('--known_mask', type=str, default=None, metavar='M', help='with --known_volume: non-zero = trust this voxel of K (NIfTI on K\'s grid)')
    p.add_argument('--known_drop_slices', type=str, nargs='+', default=None, metavar='A:B',
                   help='with --known_volume: slices A..B (inclusive) of the prediction grid to distrust, e.g. ruined by motion')
    p.add_argument('--known_resample', type=int, default=1, metavar='R',
                   help='with --known_volume: execute every reverse step R times, re-noising one level in between (RePaint, jump length 1): '
                        'the free region harmonises with the known one, at R times the sampling time')


def parse_drop_slices(values):
    """['A:B', ...] -> [(A, B)] with 0 <= A <= B; ValueError naming the flag otherwise."""
    out = []
    for v in values or ():
        parts = str(v).split(':')
        try:
            a, b = (int(x) for x in parts) if len(parts) == 2 else (None, None)
        except ValueError:
            a = b = None
        if a is None or a < 0 or b < a:
            raise ValueError(f'--known_drop_slices takes ranges A:B of slices with 0 <= A <= B, got {v!r}')
        out.append((a, b))
    return out


def options_from(args):
    """A namespace's --known_* flags (any may be missing) -> None without --known_volume, else dict(volume, mask, drop [(a, b)], resample).
    ValueError, naming the flag, for a dependent flag without --known_volume (a cohort's namespace excepted: its K is the manifest's
    `known` column) and for a bad value."""
    volume, mask = getattr(args, 'known_volume', None), getattr(args, 'known_mask', None)
    drop, resample = getattr(args, 'known_drop_slices', None), getattr(args, 'known_resample', 1)
    resample = 1 if resample is None else resample
    if volume is None:
        if getattr(args, 'manifest', None) is not None or getattr(args, 'brats_root', None) is not None:
            return None                                   # a cohort: K comes from the manifest, per subject; the other flags from here
        own_grid = (getattr(args, 'known_thick_volume', None) is not None or          # (mudiff_hip.thick_volume and mudiff_hip.lowres_volume
                    getattr(args, 'known_lowres_volume', None) is not None)           #  take --known_resample too)
        for flag, given in (('--known_mask', mask is not None), ('--known_drop_slices', drop is not None),
                            ('--known_resample', resample != 1 and not own_grid)):
            if given:
                raise ValueError(f'{flag} needs --known_volume')
        return None
    if int(resample) != resample or resample < 1:
        raise ValueError(f'--known_resample must be an integer >= 1, got {resample}')
    from .constraints import need_keyed_seed
    need_keyed_seed(args, '--known_volume')
    return dict(volume=volume, mask=mask, drop=parse_drop_slices(drop), resample=int(resample))


def suffix(region):
    """What a [done] line gains (nothing without --known_volume)."""
    if region is None:
        return ''
    return f" | known={region.report['fraction_of_slab']:.3f}" + (f' x{region.resample}' if region.resample > 1 else '')


# ---------------------------------------------------------------------------------------------------
# K and M on the prediction's grid
# ---------------------------------------------------------------------------------------------------
KnownInputs = collections.namedtuple('KnownInputs', 'values trust coverage shape resampled options')
KnownInputs.__doc__ = """K on the prediction's grid: `values` [X,Y,Z] (float), `trust` [X,Y,Z] or None (M), `coverage` uint8 [X,Y,Z]
(mud_known_coverage; None = all ones: K was not resampled), `shape` of the grid, `resampled`: the names of what was resampled, `options`:
options_from's dict."""


def read_inputs(known, intake_options):
    """(host work only) The files of options_from's dict as volume_prepare.read_for_evaluation reads them -> (K, M or None)."""
    from .volume_prepare import read_for_evaluation
    return read_for_evaluation(known['volume'], intake_options), read_for_evaluation(known['mask'], intake_options)


def on_grid(first, files, known, intake_options, device, align=None):
    """K and M (read_inputs') on the grid the prediction will have (volume_prepare.evaluation_grid: `first` is the first input as
    read_for_evaluation reads it, or its RawVolume) -> KnownInputs.  ValueError for a shape that differs from the grid's when nothing
    resamples."""
    from . import ops
    from . import volume_prepare as VP
    from . import volume_regrid as VR
    K, M = files
    grid, K, M, _, resample, found = VP.evaluation_grid(first, K, M, intake_options, device, align)
    shape = tuple(int(v) for v in grid[0])
    coverage, done = None, []
    if resample:
        ref_world = VR.world_affine_of(grid[1], grid[2])
        src_world = VR.world_affine_of(K.affine, K.header)
        if len(K.shape) != 3:
            raise ValueError(f'--known_volume: expected a 3D volume, got shape {tuple(K.shape)}')
        if not VR.same_grid(K.shape, src_world, shape, ref_world):
            cov = ops.known_coverage(VR.grid_matrix(src_world, ref_world), K.shape, shape, device)
            coverage = np.ascontiguousarray(cov.cpu().numpy().transpose(2, 1, 0))
        K, M, done = VR.eval_onto_grid(shape, ref_world, K, M, device, names=('known_volume', 'known_mask'), interp=intake_options.interp,
                                       found=found, **(dict(antialias=True) if intake_options.antialias else {}))
    for name, v in (('--known_volume', K), ('--known_mask', M)):
        if v is not None and tuple(np.shape(v)) != shape:
            raise ValueError(f'{name}: shape {tuple(np.shape(v))} differs from the prediction grid {shape} (pass --regrid to resample it)')
    return KnownInputs(np.asarray(K), None if M is None else np.asarray(M), coverage, shape, done, known)


# ---------------------------------------------------------------------------------------------------
# the known region
# ---------------------------------------------------------------------------------------------------
class KnownRegion:
    """The known region of one prediction: `mask` bool [X,Y,Z]; `norm` float32 [X,Y,Z], K under --norm in [-1,1] (0 where K is not
    finite); `k01` float32 [X,Y,Z], ops.to_range_0_1 of it: what the written maps carry; `report`: known_<t>.json; `resample`: R."""

    def __init__(self, mask, norm, k01, report, resample):
        self.mask, self.norm, self.k01, self.report, self.resample = mask, norm, k01, report, int(resample)


def compose_mask(coverage, finite, trust, drop, s0, s1):
    """The AND of the definition -> (bool [X,Y,Z], the voxel counts of each term inside nothing but itself)."""
    shape = finite.shape
    in_slab = np.zeros(shape[2], bool)
    in_slab[s0:s1 + 1] = True
    kept = np.ones(shape[2], bool)
    for a, b in drop:
        kept[a:b + 1] = False
    terms = collections.OrderedDict()
    terms['coverage'] = np.ones(shape, bool) if coverage is None else np.asarray(coverage) != 0
    terms['finite'] = np.asarray(finite, bool)
    if trust is not None:
        terms['mask'] = np.asarray(trust) != 0
    terms['not_dropped'] = np.broadcast_to(kept[None, None, :], shape)
    terms['slab'] = np.broadcast_to(in_slab[None, None, :], shape)
    mask = np.ones(shape, bool)
    for t in terms.values():
        mask = mask & t
    return mask, {k: int(np.count_nonzero(t)) for k, t in terms.items()}


def compose(inputs, ref, norm, device):
    """KnownInputs and the prediction's ref = (shape, affine, header, s0, s1) -> KnownRegion.  ValueError when the grid is not ref's."""
    from . import ops
    from .volume import normalise_volume
    shp, s0, s1 = tuple(int(v) for v in ref[0]), int(ref[3]), int(ref[4])
    if inputs.shape != shp:
        raise ValueError(f'--known_volume: on the grid {inputs.shape}, the prediction is on {shp}')
    finite = np.isfinite(inputs.values)
    values = inputs.values if finite.all() else np.where(finite, inputs.values, 0.0)
    mask, counts = compose_mask(inputs.coverage, finite, inputs.trust, inputs.options['drop'], s0, s1)
    knorm = np.ascontiguousarray(normalise_volume(values, norm), dtype=np.float32)
    k01 = ops.to_range_0_1(torch.from_numpy(knorm).to(device)).cpu().numpy()
    slab = shp[0] * shp[1] * (s1 - s0 + 1)
    known = int(np.count_nonzero(mask))
    report = dict(shape=list(shp), slab=[s0, s1], terms=counts, known_voxels=known, slab_voxels=slab,
                  fraction_of_slab=known / slab if slab else 0.0, known_per_slice=[int(np.count_nonzero(mask[:, :, z])) for z in range(s0, s1 + 1)],
                  drop_slices=[list(r) for r in inputs.options['drop']], resample=inputs.options['resample'], resampled=list(inputs.resampled))
    return KnownRegion(mask, knorm, k01, report, inputs.options['resample'])


def sampler_inputs(region, s0, s1, size, device):
    """-> (known fp32 [n,1,S,S] in [-1,1], mask uint8 [n,1,S,S]) for GraphSampler.sample_keyed, n = s1 - s0 + 1: the slab's planes,
    resized like the conditions when the in-plane size is not S; a pixel is then known where the resized unknown indicator is exactly 0."""
    from . import ops
    planes = lambda a, dt: torch.from_numpy(np.ascontiguousarray(np.moveaxis(a[:, :, s0:s1 + 1], 2, 0), dtype=dt)).to(device)[:, None]      # noqa: E731
    known, mask = planes(region.norm, np.float32), planes(region.mask, np.uint8)
    if tuple(known.shape[-2:]) != (size, size):
        known = ops.resize_bilinear(known.contiguous(), (size, size))
        unknown = ops.resize_bilinear((mask == 0).float().contiguous(), (size, size))
        mask = (unknown == 0).to(torch.uint8)
    return known.contiguous(), mask.contiguous()


def constraint_for(region, s0, s1, size, args, device):
    """What the samplers take for the run's K (mudiff_hip.constraints): under --known_thick, --known_kspace, --known_multislice or
    --known_sense K is measured that way instead (thick.measure, kspace.measure, multislice.measure, sense.measure), else its known voxels themselves
    (constraints.KnownVoxels of sampler_inputs)."""
    from . import kspace, multislice, sense, thick
    from .constraints import KnownVoxels
    for module, more in ((thick, ()), (kspace, (args.seed,)), (multislice, (args.seed,)), (sense, (args.seed,))):
        options = module.options_from(args)
        if options is not None:
            return module.measure(region, s0, s1, size, options, *more, device)
    return KnownVoxels(*sampler_inputs(region, s0, s1, size, device), region.resample)


def paste(vol, region, device, std=False):
    """A map as it is about to be written (host [X,Y,Z], fp32) with the known voxels put in (mud_known_constrain, clean): region.k01, or 0
    for an ensemble's std -> a new host array of the same shape."""
    from . import ops
    v = torch.from_numpy(np.ascontiguousarray(vol, dtype=np.float32)).to(device)
    if tuple(v.shape) != region.mask.shape:
        raise ValueError(f'known region {region.mask.shape} and written volume {tuple(v.shape)} differ in shape')
    k = torch.zeros_like(v) if std else torch.from_numpy(region.k01).to(device)
    m = torch.from_numpy(np.ascontiguousarray(region.mask, dtype=np.uint8)).to(device)
    return ops.known_constrain(v.view(1, -1), k.view(1, -1), m.view(1, -1), None, 0, None, None, clean=True).view(v.shape).cpu().numpy()


def region_bits(region, s0, s1, first_bit):
    """uint8 [n,X,Y]: bit first_bit = known, bit first_bit + 1 = synthesised, on the slab's planes (every plane of it is in the slab)."""
    m = np.ascontiguousarray(np.moveaxis(region.mask[:, :, s0:s1 + 1], 2, 0))
    return (m.astype(np.uint8) << first_bit) | ((~m).astype(np.uint8) << (first_bit + 1))


def write_json(region, output_dir, target):
    path = os.path.join(output_dir, f'known_{target.lower()}.json')
    with open(path, 'w') as f:
        json.dump(region.report, f, indent=1)
    return path
