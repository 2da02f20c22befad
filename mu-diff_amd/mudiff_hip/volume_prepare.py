"""The one input-preparation stage of the volume pipeline (DESIGN.md sections 5.10 - 5.22) and the subject-level plan around it: every
entry point - volume.predict_volume on the host, with --device_intake, and mudiff_hip.cohort - reads a subject's files, hands them to
prepare_inputs and normalises what comes back, on the host (volume.host_stacks) or on the device (volume_intake.condition_from_raw).

    STAGES                                                one line per stage: its module (add_flags, options_from, the suffixes, write_reports)
    IntakeOptions.from_args(args)                         what --norm, --slice_half_range and every stage's flags ask for, built once
    prepare_inputs(named_raws, options, device)           reorient; denoise; unring; foreground; first input = the grid [conformed, aligned]; coregister; regrid, or check the shape; brain mask; bias-correct
    IntakeReport                                          what that did, by modality name: the [done] line's tail and the report files
    read_for_evaluation, evaluation_inputs                --gt_volume / --eval_mask on the grid the prediction will have
    output_writer                                         --reorient_back / --conform_back around a writer

A stage's flags, their defaults and their checks live in the stage's own module (add_flags, options_from): nothing here lists them.
"""
from __future__ import annotations

import collections

import numpy as np

from . import volume_align as VA
from . import volume_bias as VB
from . import volume_brain as VBR
from . import volume_conform as VCF
from . import volume_coreg as VC
from . import volume_denoise as VD
from . import volume_foreground as VF
from . import volume_intake as VI
from . import volume_regrid as VR
from . import volume_reorient as VO
from . import volume_unring as VU
from .volume_intake import slab_range

# One line per stage, in the order of the flags, of the [done] line's parts and of the report files.  `parts`: (the module's suffix
# function, the IntakeReport attributes it takes); `written`: the attributes (and `affine` / `header`, the prediction's) that its
# write_reports takes after (entries, output_dir, target), the first of them being the entries; None for a stage without a report file.
# Functions are looked up in the module when they are called: a test may replace them there.
Stage = collections.namedtuple('Stage', 'module parts written')
STAGES = (
    Stage(VR, (('regrid_suffix', 'regridded'), ('interp_suffix', 'interp nonfinite')), None),
    Stage(VC, (('coreg_suffix', 'coreg'),), 'coreg'),
    Stage(VB, (('bias_suffix', 'bias'),), 'bias affine header'),
    Stage(VD, (('denoise_suffix', 'denoise'),), 'denoise'),
    Stage(VF, (('foreground_suffix', 'foreground'),), 'foreground affine header'),
    Stage(VBR, (('brain_suffix', 'brain'),), 'brain affine header'),
    Stage(VO, (('reorient_suffix', 'reorient'),), 'reorient'),
    Stage(VCF, (('conform_suffix', 'conform conform_grid'), ('antialias_suffix', 'lowpass')), 'conform conform_grid'),
    Stage(VU, (('unring_suffix', 'unring'),), 'unring'),
    Stage(VA, (('align_suffix', 'align'),), 'align'),
)


class IntakeOptions(collections.namedtuple('IntakeOptions', 'norm regrid coreg bias half_range foreground brain interp reorient conform antialias unring align denoise',
                                           defaults=('percentile', False, None, None, 80, None, None, 'linear', None, None, False, None, None, None))):
    """norm: --norm; half_range: --slice_half_range (the slab is part of the reference geometry); every other field is what one stage's
    options_from made of that stage's flags (its docstring says what): regrid and interp (volume_regrid), coreg, bias, denoise,
    foreground, brain, reorient, conform and antialias (volume_conform), unring, align.  `foreground`, `brain`, `interp`, `reorient`, `conform`,
    `antialias`, `unring` and `align` sit before `denoise`, not at the end: tests/test_volume_denoise_host.py pins `denoise` as the last field, and every
    positional use stops at half_range."""
    __slots__ = ()

    @classmethod
    def from_args(cls, args):
        """A namespace that did not come from volume.make_parser may lack any flag: a stage's options_from knows its defaults.
        ValueError, naming the flag, for a value a stage refuses."""
        fields = dict(norm=getattr(args, 'norm', cls._field_defaults['norm']),
                      half_range=int(getattr(args, 'slice_half_range', cls._field_defaults['half_range'])))
        for stage in STAGES:
            fields.update(stage.module.options_from(args))
        return cls(**fields)

    @property
    def eval_as_stored(self):
        """The evaluation inputs are read as stored (volume_intake.read_nifti_raw), geometry included, because the device reorients or
        resamples them; otherwise they are read as arrays (volume.read_nifti) and only compared."""
        return self.regrid or self.reorient is not None or self.conform is not None


class IntakeReport:
    """What the preparation did to one subject, by modality name: `regridded` [name], `coreg` [(name, report)], `bias` [(name, report,
    field or None)], `denoise` [(name, report)], `foreground` [(name, report, the masked volume or None)], `brain` [(the source's name,
    report, the uint8 [X,Y,Z] host mask or None)]: one entry per subject; `reorient` [(name, entry)] (volume_reorient.ReorientPlan.entry);
    `interp` (--regrid_interp) and `nonfinite`, the non-finite voxels a cubic resampling or the anti-aliasing low-pass read as 0; `conform`
    [(name, entry)] (volume_conform.entry) with `conform_grid`, the grid's name ('240x240x155@1mm'); `lowpass`: a low-pass actually ran
    (--antialias); `align` [(the first input's name, report)] (volume_align.estimate); `unring` [(name, report)]
    (volume_unring.unring)."""

    def __init__(self, regridded=(), interp='linear', nonfinite=0, lowpass=False):
        self.regridded, self.coreg, self.bias, self.denoise, self.foreground, self.brain = list(regridded), [], [], [], [], []
        self.interp, self.nonfinite = interp, int(nonfinite)
        self.reorient = []
        self.conform, self.conform_grid, self.lowpass = [], None, bool(lowpass)
        self.align = []
        self.unring = []

    def add_evaluation(self, resampled, found):
        """What evaluation_inputs did, after the inputs' own: the names it resampled, and its `found`."""
        self.regridded += resampled
        self.nonfinite += found.get('nonfinite', 0)
        self.lowpass = self.lowpass or bool(found.get('lowpass'))

    def suffix(self):
        """What a [done] line gains: ` | regrid=... | interp=cubic | coreg=... | bias=... | denoise=... | foreground=... | brain=... |
        reorient=... | conform=... | antialias=on | unring=... | align=...`, each part only when there is something to say (STAGES' order)."""
        return ''.join(getattr(stage.module, name)(*(getattr(self, k) for k in takes.split())) for stage in STAGES for name, takes in stage.parts)

    def write(self, output_dir, target, affine, header):
        """Every stage's report file (and the volumes its *_out flag asked for, on the grid of `affine` / `header` where they carry none)
        next to the prediction, in STAGES' order; a stage with nothing to report writes nothing, not even the directory."""
        have = dict(vars(self), affine=affine, header=header)
        for stage in STAGES:
            takes = (stage.written or '').split()
            if takes and have[takes[0]]:
                stage.module.write_reports(have[takes[0]], output_dir, target, *(have[k] for k in takes[1:]))


def read_for_evaluation(path, options):
    """One file the evaluation needs (the first input, --gt_volume, --eval_mask; None stays None) for evaluation_inputs: a RawVolume as
    stored under options.eval_as_stored, else volume.read_nifti's (array, affine, header).  Host work only: a cohort calls it on its
    prefetch thread."""
    from . import volume as V
    if path is None:
        return None
    return VI.read_nifti_raw(path) if options.eval_as_stored else V.read_nifti(path)


def evaluation_inputs(first, gt, label, options, device, names, wording, align=None):
    """The evaluation inputs on the grid the prediction will have, checked (volume_metrics.eval_inputs_on_grid: `names`, `wording`).
    first, gt, label (or None): read_for_evaluation's, or for `first` the RawVolume a caller has read anyway.  The grid is the first
    input's own; under --reorient that input's once reoriented (volume_reorient.reference_of: no voxel of it is moved), each evaluation
    input being reoriented by its own affine first; under --conform the conform grid of that (volume_conform.reference_of).  Under
    --regrid or --conform what is not on the grid is resampled onto it (--regrid_interp; the label volume by nearest neighbour), the
    ground truth behind the low-pass of --antialias.  Under --align the conform grid is the turned one, T @ its affine: `align` is
    estimate_alignment's result when the caller has it; otherwise the plane is estimated here, from `first`, and left in found['align']
    for the caller to hand to prepare_inputs, so that a subject's plane is estimated once.  -> ((gt, label), the names of what was resampled, `found` of
    volume_regrid.eval_onto_grid): IntakeReport.add_evaluation takes the last two."""
    from . import volume_metrics as VM
    grid, gt, label, gt_affine, resample, found = evaluation_grid(first, gt, label, options, device, align)
    evaluation, resampled = VM.eval_inputs_on_grid(grid, gt, label, gt_affine, resample, options.half_range, device, names=names, wording=wording,
                                                   interp=options.interp, found=found, **(dict(antialias=True) if options.antialias else {}))
    return evaluation, resampled, found


def evaluation_grid(first, gt, label, options, device, align=None):
    """The first half of evaluation_inputs, for a caller that resamples by itself (mudiff_hip.known_region): -> (grid = (shape, affine,
    header) the prediction will have, gt and label reoriented where --reorient asks for it, the ground truth's affine, whether what is
    not on the grid is to be resampled onto it, `found` with the alignment under --align)."""
    geometry = lambda v: (v.shape, v.affine, v.header) if hasattr(v, 'header') else (v[0].shape, v[1], v[2])      # noqa: E731
    grid, gt_affine = geometry(first), geometry(gt)[1]
    if not options.eval_as_stored:
        gt, label = gt[0], None if label is None else label[0]
    resample = options.regrid or options.conform is not None
    if options.reorient is not None:
        grid = VO.reference_of(first, **options.reorient)[0]
        gt, label, gt_affine = VO.eval_inputs(gt, label, device, options.reorient['target'], as_arrays=not resample)
    if options.conform is not None:
        grid = VCF.reference_of(grid, options.conform)
    found = {}
    if options.align is not None:
        found['align'] = align = align or estimate_alignment(first, options, device)
        grid = (grid[0], aligned_affine(align[0], grid[1]), None)
    return grid, gt, label, gt_affine, resample, found


def output_writer(write, first_raw, options, ref, device, reorient_back=False, conform_back=False):
    """`write(path, vol, affine, header)` (volume.write_nifti, or a cohort's deferred writer) wrapped for --reorient_back and
    --conform_back: the prediction arrives on the grid `ref` it was sampled on; --conform_back, outermost, resamples it onto the first
    input's own grid (under --reorient: that grid reoriented), and --reorient_back, innermost, returns it to the storage order of
    `first_raw`, the first input as read."""
    if options.reorient is not None and reorient_back:
        write = VO.write_back(write, first_raw, **options.reorient)
    if options.conform is not None and conform_back:
        write = VCF.write_back(write, VCF.first_on_own_grid(first_raw, options), ref[0], ref[1], device, options.interp, options.antialias)
    return write


def _on_own_grid(named_raws, options, device, report, label):
    """--reorient, --denoise, --unring and --foreground: every input on its own grid (prepare_inputs says what each does) -> the new list.
    label: name -> what a warning line calls the input; None prints no warning line (the caller prints it: warn_first)."""
    if options.reorient is not None:
        turned = []
        for name, raw in named_raws:
            vol, found = VO.reorient(raw, device, **options.reorient)
            report.reorient.append((name, found))
            if label is not None:
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
    if options.unring is not None:                       # on the input's own grid: a resampling moves the ripples off the lattice the method relies on
        unrung = []
        for name, raw in named_raws:
            vol, found = VU.unring(raw, device, name='the first input' if label is None else label(name), **options.unring)
            report.unring.append((name, found))
            unrung.append((name, vol))
        named_raws = unrung
    if options.foreground is not None:
        masked = []
        for name, raw in named_raws:
            vol, found = VF.foreground(raw, device, **options.foreground)
            report.foreground.append((name, found, vol if options.foreground['mask_out'] and vol is not raw else None))
            masked.append((name, vol))
        named_raws = masked
    return named_raws


class Alignment(collections.namedtuple('Alignment', 'T report first stages')):
    """estimate_alignment's result: T and report (volume_align.estimate's), `first` - the first input as the plane was estimated from it,
    after --reorient / --denoise / --unring / --foreground - and `stages`, the IntakeReport of those four stages for it, so that prepare_inputs
    takes the first input from here and runs none of them on it again."""
    __slots__ = ()


def estimate_alignment(first_raw, options, device):
    """--align for a caller that needs the plane before prepare_inputs runs (the evaluation inputs): the first input as read, taken through
    --reorient / --denoise / --unring / --foreground as prepare_inputs takes it (no warning line: prepare_inputs prints it, with the input's name),
    then volume_align.estimate -> an Alignment, for prepare_inputs' and evaluation_inputs' `align`."""
    stages = IntakeReport()
    (_, first), = _on_own_grid([(None, first_raw)], options, device, stages, None)
    T, report = VA.estimate(first, device, **options.align)
    return Alignment(T, report, first, stages)


def aligned_affine(T, conform_affine):
    """T @ the conform grid's affine: the grid's centre column on the plane found, its left-right axis along the plane's normal; the
    affine itself, untouched, for T = I (the fallback)."""
    T = np.asarray(T, np.float64)
    return conform_affine if np.array_equal(T, np.eye(4)) else T @ np.asarray(conform_affine, np.float64)


def prepare_inputs(named_raws, options, device, labels=None, align=None):
    """A subject's inputs on the first input's grid, corrected.  named_raws: [(modality name, RawVolume)] in MODALITY_ORDERS order (the
    caller has read the files); labels: {name: what an error message calls that input} (the name itself by default; the device paths
    name the file).  -> (volumes on the grid, ref = (shape, affine, header, s0, s1) of the first input, IntakeReport).

    Under --reorient every input, the first included, is first brought to the target orientation on its own grid by its own affine
    (volume_reorient.reorient: a permutation and flips of the storage axes, the affine and header changed to match; an input stored that
    way already is left as it is), and everything below sees the reoriented list: the first input's reoriented geometry is `ref`, so that
    the slab runs along the target's third axis; an input tilted by more than volume_reorient.OBLIQUE_WARN_DEG gets a warning line.
    Under --denoise every input, the first included, is then replaced by its non-local-means estimate on its own grid
    (volume_denoise.denoise: same shape, affine and header), and everything below sees the denoised list.
    Under --unring every input, the first included, then has its truncation ringing removed on its own grid (volume_unring.unring: same
    shape, affine and header; before --foreground, whose mask re-zeroes what the correction's sinc tails put into the background).
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
    the conform grid.  Under --align (options.align) the mid-sagittal plane of the first input, as it is at this
    point, is estimated (volume_align.estimate; with `align`, estimate_alignment's result, the plane and the first input as it is at this
    point are taken from there: neither the estimate nor the four stages above run on the first input twice) and the
    conform grid's affine becomes T @ itself: still one regrid_to per input, now onto the turned grid.  With options.antialias every such resampling (--regrid's and --coregister's too) low-passes what it downsamples.  Under --bias_correct every input, the first
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
    if isinstance(align, Alignment):                     # the first input has been through these stages: its entries and its warning line first
        name = named_raws[0][0]
        for stage in ('reorient', 'denoise', 'unring', 'foreground'):
            getattr(report, stage).extend((name,) + tuple(entry[1:]) for entry in getattr(align.stages, stage))
        for _, found in report.reorient:
            VO.warn_oblique(label(name), found)
        named_raws = [(name, align.first)] + _on_own_grid(named_raws[1:], options, device, report, label)
    else:
        named_raws = _on_own_grid(named_raws, options, device, report, label)
    first = named_raws[0][1]
    ref = (first.shape, first.affine, first.header) + slab_range(first.shape[2], options.half_range)
    ref_world = VR.world_affine_of(first.affine, first.header)
    if options.conform is not None:
        grid_shape, ref_world = VCF.conform_grid(first.shape, ref_world, **options.conform)
        if options.align is not None:
            T, found = align[:2] if align else VA.estimate(first, device, **options.align)
            report.align.append((named_raws[0][0], found))
            ref_world = aligned_affine(T, ref_world)
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
