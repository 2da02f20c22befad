"""The one input-preparation stage of the volume pipeline (DESIGN.md sections 5.10 - 5.18): every entry point - volume.predict_volume
on the host, with --device_intake, and mudiff_hip.cohort - reads a subject's files, hands them to prepare_inputs and normalises what
comes back, on the host (volume.host_stacks) or on the device (volume_intake.condition_from_raw).

    IntakeOptions.from_args(args)                         what --norm / --regrid / --coregister / --bias_correct / --denoise / --foreground / --brain_extract / --reorient ask for, built once
    prepare_inputs(named_raws, options, device)           reorient; denoise; foreground; first input = the grid; coregister; regrid, or check the shape; brain mask; bias-correct
    IntakeReport                                          what that did, by modality name: the [done] line's tail and the report files
"""
from __future__ import annotations

import collections

import numpy as np

from . import volume_bias as VB
from . import volume_brain as VBR
from . import volume_conform as VCF
from . import volume_coreg as VC
from . import volume_denoise as VD
from . import volume_foreground as VF
from . import volume_regrid as VR
from . import volume_reorient as VO
from .volume import regrid_suffix
from .volume_intake import slab_range


class IntakeOptions(collections.namedtuple('IntakeOptions', 'norm regrid coreg bias half_range foreground brain interp reorient conform antialias denoise',
                                           defaults=('percentile', False, None, None, 80, None, None, 'linear', None, None, False, None))):
    """norm: --norm; regrid: --regrid; coreg / bias / denoise / foreground: the keyword arguments of volume_coreg.coregister /
    volume_bias.correct / volume_denoise.denoise / volume_foreground.foreground, or None without --coregister / --bias_correct / --denoise /
    --foreground; half_range: --slice_half_range (the slab is part of the reference geometry); brain: the keyword arguments of volume_brain.brain_mask plus
    `source` (--brain_from or None) and `mask_out`, or None without --brain_extract; interp: --regrid_interp (how --regrid / --coregister
    resample an image: 'linear' or 'cubic'); reorient: dict(target=the orientation code of --reorient_to), or None without --reorient;
    conform: dict(shape, spacing, target) of --conform_shape / --conform_spacing / --conform_to (the keyword arguments of
    volume_conform.conform_grid), or None without --conform; antialias: --antialias as a bool (on by default under --conform, off otherwise).
    `foreground`, `brain`, `interp`, `reorient`, `conform` and `antialias` sit before `denoise`, not
    at the end: tests/test_volume_denoise_host.py pins `denoise` as the last field, and every positional use stops at half_range."""
    __slots__ = ()

    @classmethod
    def from_args(cls, args):
        """The only place that knows the flags' defaults (a namespace that did not come from volume.make_parser may lack any of them)."""
        get = lambda name, default: getattr(args, name, default)      # noqa: E731
        coreg = bias = denoise = foreground = brain = reorient = None
        if get('coregister', False):
            coreg = dict(strides=tuple(int(s) for s in get('coregister_strides', None) or (4, 2, 1)),
                         max_mm=float(get('coregister_max_mm', 20.0)), max_deg=float(get('coregister_max_deg', 15.0)))
        if get('bias_correct', False):
            bias = dict({k: type(v)(get('bias_' + k, v)) for k, v in VB.DEFAULTS.items()}, field=bool(get('bias_field_out', False)))
        if get('denoise', False):
            sigma = get('denoise_sigma', None)
            denoise = dict(sigma=None if sigma is None else float(sigma), search=int(get('denoise_search', VD.DEFAULTS['search'])),
                           patch=int(get('denoise_patch', VD.DEFAULTS['patch'])), beta=float(get('denoise_beta', VD.DEFAULTS['beta'])),
                           rician=bool(get('denoise_rician', False)))
        if get('foreground', False):
            foreground = dict(bins=int(get('foreground_bins', VF.DEFAULTS['bins'])), open=int(get('foreground_open', VF.DEFAULTS['open'])),
                              keep_holes=bool(get('foreground_keep_holes', False)), mask_out=bool(get('foreground_mask_out', False)))
        if get('brain_extract', False):
            source = get('brain_from', None)
            brain = dict(bins=int(get('brain_bins', VBR.DEFAULTS['bins'])), erode_mm=float(get('brain_erode_mm', VBR.DEFAULTS['erode_mm'])),
                         dilate_mm=float(get('brain_dilate_mm', VBR.DEFAULTS['dilate_mm'])), keep_holes=bool(get('brain_keep_holes', False)),
                         source=None if source is None else str(source), mask_out=bool(get('brain_mask_out', False)))
        if get('reorient', False):
            reorient = dict(target=VO.check_target(get('reorient_to', None) or VO.DEFAULT_TARGET))
        conform = None
        if get('conform', False):
            spacing = get('conform_spacing', None)
            conform = dict(shape=VCF._shape3(get('conform_shape', None) or VCF.DEFAULT_SHAPE),
                           spacing=VCF._spacing3(VCF.DEFAULT_SPACING if spacing is None else spacing),
                           target=VO.check_target(get('conform_to', VCF.DEFAULT_TARGET)))
        antialias = get('antialias', None)
        antialias = conform is not None if antialias is None else antialias in (True, 'on')
        return cls(get('norm', 'percentile'), bool(get('regrid', False)), coreg, bias, int(get('slice_half_range', 80)), foreground, brain,
                   str(get('regrid_interp', 'linear')), reorient, conform, antialias, denoise)


class IntakeReport:
    """What the preparation did to one subject, by modality name: `regridded` [name] (a caller appends the evaluation inputs --regrid
    resampled: `report.regridded += names`), `coreg` [(name, report)], `bias` [(name, report, field or None)], `denoise` [(name,
    report)], `foreground` [(name, report, the masked volume or None)], `brain` [(the source's name, report, the uint8 [X,Y,Z] host mask or
    None)]: one entry per subject; `reorient` [(name, entry)] (volume_reorient.ReorientPlan.entry); `interp` (--regrid_interp) and
    `nonfinite`, the non-finite voxels a cubic resampling or the anti-aliasing low-pass read as 0; `conform` [(name, entry)]
    (volume_conform.entry) with `conform_grid`, the grid's name ('240x240x155@1mm'); `lowpass`: a low-pass actually ran (--antialias)."""

    def __init__(self, regridded=(), interp='linear', nonfinite=0, lowpass=False):
        self.regridded, self.coreg, self.bias, self.denoise, self.foreground, self.brain = list(regridded), [], [], [], [], []
        self.interp, self.nonfinite = interp, int(nonfinite)
        self.reorient = []
        self.conform, self.conform_grid, self.lowpass = [], None, bool(lowpass)

    def suffix(self):
        """What a [done] line gains: ` | regrid=... | interp=cubic | coreg=... | bias=... | denoise=... | foreground=... | brain=... | reorient=... | conform=... | antialias=on`, each part only when
        its list is not empty."""
        return (regrid_suffix(self.regridded) + VR.interp_suffix(self.interp, self.nonfinite) + VC.coreg_suffix(self.coreg) + VB.bias_suffix(self.bias) + VD.denoise_suffix(self.denoise) +
                VF.foreground_suffix(self.foreground) + VBR.brain_suffix(self.brain) + VO.reorient_suffix(self.reorient) +
                VCF.conform_suffix(self.conform, self.conform_grid) + VCF.antialias_suffix(self.lowpass))

    def write(self, output_dir, target, affine, header):
        """coreg_<t>.json, bias_<t>.json (and the fields --bias_field_out asked for) , denoise_<t>.json and foreground_<t>.json (and the masks
        --foreground_mask_out asked for) and brain_<t>.json (and the mask --brain_mask_out asked for, on the grid of `affine` / `header`)
        and reorient_<t>.json and conform_<t>.json next to the prediction; nothing when empty."""
        if self.coreg:
            VC.write_reports(self.coreg, output_dir, target)
        if self.bias:
            VB.write_reports(self.bias, output_dir, target, affine, header)
        if self.denoise:
            VD.write_reports(self.denoise, output_dir, target)
        if self.foreground:
            VF.write_reports(self.foreground, output_dir, target, affine, header)
        if self.brain:
            VBR.write_reports(self.brain, output_dir, target, affine, header)
        if self.reorient:
            VO.write_reports(self.reorient, output_dir, target)
        if self.conform:
            VCF.write_reports(self.conform, output_dir, target, self.conform_grid)


def prepare_inputs(named_raws, options, device, labels=None):
    """A subject's inputs on the first input's grid, corrected.  named_raws: [(modality name, RawVolume)] in MODALITY_ORDERS order (the
    caller has read the files); labels: {name: what an error message calls that input} (the name itself by default; the device paths
    name the file).  -> (volumes on the grid, ref = (shape, affine, header, s0, s1) of the first input, IntakeReport).

    Under --reorient every input, the first included, is first brought to the target orientation on its own grid by its own affine
    (volume_reorient.reorient: a permutation and flips of the storage axes, the affine and header changed to match; an input stored that
    way already is left as it is), and everything below sees the reoriented list: the first input's reoriented geometry is `ref`, so that
    the slab runs along the target's third axis; an input tilted by more than volume_reorient.OBLIQUE_WARN_DEG gets a warning line.
    Under --denoise every input, the first included, is then replaced by its non-local-means estimate on its own grid
    (volume_denoise.denoise: same shape, affine and header), and everything below sees the denoised list.
    Under --foreground every input, the first included, then has the voxels outside its foreground mask set to exactly 0, on its own grid
    (volume_foreground.foreground: same shape, affine and header again), and everything below sees the masked list.
    The first input defines the grid and is never registered or resampled.  Every later one is aligned to it under --coregister
    (volume_coreg.coregister -> world; its search stays trilinear), then resampled under --regrid or --coregister (volume_regrid.regrid_to
    with --regrid_interp: untouched when it is on the grid already); otherwise it must have the first one's shape.  Under --brain_extract one brain mask is then estimated from one input
    on that grid (volume_brain.source_of picks it; volume_brain.brain_mask) and every input has the voxels outside it set to exactly 0; a
    mask that could not be estimated leaves the inputs as they are (the report's `kept` is 0).
    Under --conform (options.conform) the grid is not the first input's own but volume_conform.conform_grid of it:
    `ref` holds that grid's shape, affine, volume_conform.conformed_header and slab.  The later inputs are still coregistered against the
    unresampled first input, and then every input, the first included, goes through one regrid_to onto the conform grid (one
    interpolation per input; an input that is on that grid already is left untouched); the brain mask and the bias correction follow on
    the conform grid.  With options.antialias every such resampling (--regrid's and --coregister's too) low-passes what it downsamples.  Under --bias_correct every input, the first
    included, is then divided by its bias field (volume_bias.correct).  ValueError for an input that is not 3D or a --brain_from that is
    not among the inputs, before any device work."""
    label = lambda name: (labels or {}).get(name, name)      # noqa: E731
    for name, raw in named_raws:
        if len(raw.shape) != 3:
            raise ValueError(f'{label(name)}: expected a 3D volume, got shape {raw.shape}')
    brain = None if options.brain is None else dict(options.brain)
    if brain is not None:
        source, mask_out = VBR.source_of([name for name, _ in named_raws], brain.pop('source', None)), brain.pop('mask_out', False)
    report = IntakeReport(interp=options.interp)
    if options.reorient is not None:
        turned = []
        for name, raw in named_raws:
            vol, found = VO.reorient(raw, device, **options.reorient)
            report.reorient.append((name, found))
            VO.warn_oblique(label(name), found)
            turned.append((name, vol))
        named_raws = turned
    if options.denoise is not None:
        cleaned = []
        for name, raw in named_raws:
            vol, found = VD.denoise(raw, device, **options.denoise)
            report.denoise.append((name, found))
            cleaned.append((name, vol))
        named_raws = cleaned
    if options.foreground is not None:
        masked = []
        for name, raw in named_raws:
            vol, found = VF.foreground(raw, device, **options.foreground)
            report.foreground.append((name, found, vol if options.foreground['mask_out'] and vol is not raw else None))
            masked.append((name, vol))
        named_raws = masked
    first = named_raws[0][1]
    ref = (first.shape, first.affine, first.header) + slab_range(first.shape[2], options.half_range)
    ref_world = VR.world_affine_of(first.affine, first.header)
    if options.conform is not None:
        grid_shape, ref_world = VCF.conform_grid(first.shape, ref_world, **options.conform)
        ref = (grid_shape, ref_world, VCF.conformed_header(grid_shape, ref_world, first.header)) + slab_range(grid_shape[2], options.half_range)
        report.conform_grid = VCF.grid_name(grid_shape, options.conform['spacing'])
    def corrected(name, vol):
        if options.bias is not None:
            vol, found = VB.correct(vol, device, **options.bias)
            report.bias.append((name, found, vol.field if options.bias['field'] else None))
        return vol

    prepared = []
    for k, (name, raw) in enumerate(named_raws):
        vol = raw
        if k == 0 and options.conform is None:                # the first input (not `raw is first`: one volume may be given twice)
            pass
        elif options.conform is not None or options.regrid or options.coreg is not None:
            world = None
            if k and options.coreg is not None:
                world, found = VC.coregister(first, raw, device, **options.coreg)
                report.coreg.append((name, found))
            seen = {}
            how = {} if options.interp == 'linear' else dict(mode=options.interp, found=seen)      # (the default call as it ever was)
            if options.antialias:
                how.update(found=seen, antialias=True, name=label(name))
            vol = VR.regrid_to(raw, ref[0], ref_world, device, header=ref[2], world=world, **how)
            report.nonfinite += seen.get('nonfinite', 0)
            report.lowpass = report.lowpass or bool(seen.get('lowpass'))
            if options.conform is not None:
                moved = world is not None and not np.array_equal(np.asarray(world, np.float64), np.eye(4))
                M = VR.grid_matrix(VR.world_affine_of(raw.affine, raw.header), world @ ref_world if moved else ref_world)
                report.conform.append((name, VCF.entry(raw, M, vol is not raw, seen.get('nonfinite', 0), options.antialias)))
            elif vol is not raw:
                report.regridded.append(name)
        elif raw.shape != ref[0]:
            raise ValueError(f'All input volumes must share shape. Got {raw.shape} vs {ref[0]} for {label(name)}')
        prepared.append(corrected(name, vol) if brain is None else vol)      # (the mask needs every input on the grid first)
    if brain is not None:
        names = [name for name, _ in named_raws]
        mask, found = VBR.brain_mask(prepared[names.index(source)], device, **brain)
        found['source'] = source
        report.brain.append((source, found, VBR.host_mask(mask) if mask_out and mask is not None else None))
        if mask is not None:
            prepared = [VBR.apply_mask(vol, mask, device) for vol in prepared]
        prepared = [corrected(name, vol) for name, vol in zip(names, prepared)]
    return prepared, ref, report
