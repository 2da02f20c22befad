"""Cohort volume prediction: a whole test split in one process (the volume pipeline of mudiff_hip.volume, once per subject).

    python -m mudiff_hip.cohort --manifest cohort.tsv --target_modality T1CE --exp <exp> --output_dir out [--score] [volume.py's flags]
    python -m mudiff_hip.cohort --brats_root DIR --subjects test.list --target_modality T1CE --exp <exp> --output_dir out --score

What one process buys: the checkpoints are loaded, the weights packed and the sampler's hipGraphs captured once (one GraphSampler per
(batch, image_size), reused for every subject); a small host thread pool reads and gunzips subject i+1 while the GPU samples subject i
and compresses and writes subject i-1; the inputs go through volume_prepare.prepare_inputs like a single run's, and intake and
re-assembly run on the device (mudiff_hip.volume_intake).  All GPU work stays on one
stream in this process.

Every subject is sampled with --seed exactly as a separate `python -m mudiff_hip.volume` run would sample it, so each written volume
is that run's file, bit for bit.  (--calibrate is the exception it has to be: it runs once, on the first subject.)

A bad subject - a missing or unreadable file, volumes of different shapes, an in-plane size the flags cannot write back - is reported
and skipped; the run goes on and exits non-zero at the end.  A GPU error is not caught: it ends the run.

Outputs: <output_dir>/<id>/predicted_<t>.nii.gz (plus _std, the _q<PPP> quantile maps, metrics_<t>.json and coverage_<t>.json when
applicable; under --coverage the report gains a `coverage` block: mean and std over subjects of each region's empirical coverage and
mean interval width) and <output_dir>/cohort_<t>.json: the
per-subject rows, per region and metric the mean, the population standard deviation (ddof = 0) and the subject count, and the seconds
of every stage summed over the cohort.  With --norm zscore the moments of every volume are computed on the
prefetch thread, the [done] lines end in ` | norm=zscore`, and the reports carry "norm": "zscore" (a default run's are unchanged).
An input stage (volume_prepare.STAGES; each module's header says what it does, volume.make_parser's help what its flags are) works on
the main thread, between the read and the intake, exactly as in a single run: its report file goes next to each subject's prediction
and the subject's [done] line names what it did.  The evaluation inputs go onto the grid the prediction will have on the main thread
too (volume_prepare.evaluation_inputs); the prefetch thread only reads them (volume_prepare.read_for_evaluation).  --reorient_back and
--conform_back wrap the deferred writer (volume_prepare.output_writer): the resampling onto the first input's own grid runs on the main
thread, the compression and the write on the pool.  A subject whose manifest row has a `known` (and `known_mask`) cell is sampled with
that subject's --known_volume / --known_mask (mudiff_hip.known_region; --known_drop_slices and --known_resample
come from the command line): known_<t>.json goes next to its prediction and the regions known / synthesised join the aggregate.  Under
--known_kspace, --known_thick or --known_multislice (and the --kspace_* / --thick_* / --multislice_* flags, all from the command line)
that `known` volume was acquired undersampled in k-space, with thick slices or both instead (mudiff_hip.kspace, mudiff_hip.thick,
mudiff_hip.multislice; DESIGN.md sections 5.26 - 5.28): kspace_<t>.json, thick_<t>.json or multislice_<t>.json goes next to the
prediction, and a `known_mask` cell fails that subject.  --known_sense (and the --sense_* flags; mudiff_hip.sense, section 5.32) measures
it through several coils instead, with sense_<t>.json.
"""
from __future__ import annotations

import collections
import concurrent.futures as cf
import copy
import csv
import json
import math
import os
import sys
import struct
import time
import zlib

METRICS = ('psnr', 'ssim3d', 'mae')
MODALITIES = ('t1', 't1ce', 't2', 'flair')
QUEUE_DEPTH = 2                    # subjects read ahead, and written volumes in flight: memory stays flat whatever the cohort's size
Subject = collections.namedtuple('Subject', 'id inputs gt mask known known_mask', defaults=(None, None))      # inputs: {'T1': path, ...}; the rest: path or None


# ---------------------------------------------------------------------------------------------------
# which subjects
# ---------------------------------------------------------------------------------------------------
def read_manifest(path):
    """TSV with a header row: id, t1, t1ce, t2, flair and optionally gt, mask, known, known_mask (an empty cell is `not given`; the last
    two: the subject's --known_volume / --known_mask, mudiff_hip.known_region).  Relative paths are relative to the manifest."""
    base = os.path.dirname(os.path.abspath(path))
    with open(path, newline='') as f:
        rows = list(csv.DictReader(f, delimiter='\t'))
    if not rows:
        raise ValueError(f'{path}: no subjects')
    missing = [c for c in ('id',) + MODALITIES if c not in rows[0]]
    if missing:
        raise ValueError(f'{path}: the header lacks the column(s) {", ".join(missing)}')
    where = lambda v: (v if os.path.isabs(v) else os.path.join(base, v)) if v else None      # noqa: E731
    out = []
    for r in rows:
        sid = (r['id'] or '').strip()
        if not sid:
            raise ValueError(f'{path}: a row without an id')
        out.append(Subject(sid, {m.upper(): where((r[m] or '').strip()) for m in MODALITIES}, where((r.get('gt') or '').strip()),
                           where((r.get('mask') or '').strip()), where((r.get('known') or '').strip()),
                           where((r.get('known_mask') or '').strip())))
        if out[-1].known_mask and not out[-1].known:
            raise ValueError(f'{path}: {sid} has a known_mask without a known volume')
    if len({s.id for s in out}) != len(out):
        raise ValueError(f'{path}: subject ids must be unique')
    return out


def brats_subjects(root, list_path, target):
    """The BraTS layout: <root>/<id>/<id>_{t1,t1ce,t2,flair,seg}.nii.gz for every id in the list file (one per line; blank lines and
    # comments are skipped).  The target contrast's own file is the ground truth, seg the mask."""
    with open(list_path) as f:
        ids = [ln.strip() for ln in f if ln.strip() and not ln.lstrip().startswith('#')]
    if not ids:
        raise ValueError(f'{list_path}: no subjects')
    p = lambda sid, what: os.path.join(root, sid, f'{sid}_{what}.nii.gz')                      # noqa: E731
    return [Subject(sid, {m.upper(): p(sid, m) for m in MODALITIES}, p(sid, target.lower()), p(sid, 'seg')) for sid in ids]


# ---------------------------------------------------------------------------------------------------
# the cohort's table
# ---------------------------------------------------------------------------------------------------
def subject_row(sid, report):
    """One row of the table from a metrics_<t>.json report: {id, metrics: {region: {psnr, ssim3d, mae, voxels}}}."""
    return dict(id=sid, metrics={name: {k: report['metrics'][name][k] for k in METRICS + ('voxels',)} for name in report['regions']})


def aggregate(rows, keys=METRICS):
    """Per region and metric (`keys`) over the subjects that have a finite value: mean, std (population, ddof = 0) and count, summed in fp64 in
    row order.  A region no subject has (or only with null / infinite scores) reports null."""
    regions = []
    for r in rows:
        regions += [name for name in r['metrics'] if name not in regions]
    out = {}
    for name in regions:
        out[name] = {}
        for k in keys:
            vals = [r['metrics'][name][k] for r in rows if name in r['metrics']]
            vals = [float(v) for v in vals if v is not None and math.isfinite(v)]
            if not vals:
                out[name][k] = dict(mean=None, std=None, count=0)
                continue
            mean = math.fsum(vals) / len(vals)
            out[name][k] = dict(mean=mean, std=math.sqrt(math.fsum((v - mean) ** 2 for v in vals) / len(vals)), count=len(vals))
    return out


COVERAGE_KEYS = ('empirical', 'mean_width')


def coverage_row(report):
    """A subject's coverage block from its coverage_<t>.json report: {region: {empirical, mean_width}}."""
    return {name: {k: report['coverage'][name][k] for k in COVERAGE_KEYS} for name in report['regions']}


def aggregate_coverage(rows):
    """aggregate's mean, std and count per region over the subjects' `coverage` blocks (--coverage), for empirical and mean_width."""
    return aggregate([dict(metrics=r['coverage']) for r in rows if 'coverage' in r], COVERAGE_KEYS)


def format_lines(agg):
    """One line per region, in the style of volume_metrics.format_lines."""
    f = lambda d, spec: 'n/a' if d['mean'] is None else f"{format(d['mean'], spec)} +- {format(d['std'], spec)}"      # noqa: E731
    return [f"[cohort] {name}: PSNR {f(m['psnr'], '.4f')} dB | SSIM3D {f(m['ssim3d'], '.6f')} | MAE {f(m['mae'], '.6f')} | "
            f"subjects {m['psnr']['count']}" for name, m in agg.items()]


# ---------------------------------------------------------------------------------------------------
# one subject
# ---------------------------------------------------------------------------------------------------
def _read_subject(subject, needed, score, options):
    """(prefetch thread: no GPU work) The subject's three condition volumes as stored (volume_intake.read_nifti_raw) and, with `score`,
    the evaluation inputs as volume_prepare.read_for_evaluation reads them under `options`.  With --norm zscore every volume's moments are
    computed here too, next to the read (RawVolume.moments; their seconds in RawVolume.moments_s).  -> (raws, (gt, label or None) or
    None, seconds)."""
    from . import volume_intake as VI
    from .volume_prepare import read_for_evaluation
    t0 = time.perf_counter()
    for m in needed:
        if not subject.inputs.get(m):
            raise ValueError(f'no {m} volume given')
    raws = [VI.read_nifti_raw(subject.inputs[m]) for m in needed]
    if options.norm == 'zscore':
        for r in raws:
            t1 = time.perf_counter()
            r.moments = VI.zscore_moments(r)
            r.moments_s = time.perf_counter() - t1
    ev = None
    if score:
        if not subject.gt:
            raise ValueError('--score needs a ground-truth volume (the manifest\'s gt column)')
        ev = (read_for_evaluation(subject.gt, options), read_for_evaluation(subject.mask or None, options))
    return raws, ev, time.perf_counter() - t0


def _timed_write(path, vol, affine, header):
    from .volume import write_nifti
    t0 = time.perf_counter()
    write_nifti(path, vol, affine, header)
    return time.perf_counter() - t0


def run(args, subjects, predict=None):
    """The cohort loop -> (report dict, failures [(id, message)]).  `predict(args, plan, evaluation, conds, ref, write, calibrate,
    timing)` replaces the sampling of one subject (tests stub it); by default it is volume.predict_from_conditions on the loaded model."""
    import torch
    from . import ops
    from . import volume as V
    from . import volume_intake as VI
    from .driver import effective_prec_plan
    from .volume_prepare import IntakeOptions, evaluation_inputs, output_writer, prepare_inputs
    target = args.target_modality
    needed = V.MODALITY_ORDERS[target]
    plan = effective_prec_plan(args)
    options = IntakeOptions.from_args(args)
    norm = options.norm
    timing = dict(read=0.0, intake=0.0, sample=0.0, assemble=0.0, write=0.0, write_wait=0.0, score=0.0)
    if norm != 'percentile':                 # (a default run's report keeps the keys it had)
        timing.update(moments=0.0, read_wait=0.0)
    rows, failures, pending = [], [], collections.deque()
    t_wall = time.perf_counter()
    device = None
    if predict is None:
        torch.cuda.set_device(args.gpu_chose)
        device = torch.device(f'cuda:{args.gpu_chose}')
        gen1, gen2 = V.load_generators(args, device)
        samplers = {}

        def predict(sargs, plan, evaluation, conds, ref, write, calibrate, timing):
            return V.predict_from_conditions(sargs, plan, evaluation, gen1, gen2, device, conds, ref, on_device=True, samplers=samplers,
                                             write=write, calibrate=calibrate, timing=timing)

    def drain(keep):
        while len(pending) > keep:
            timing['write'] += pending.popleft().result()

    pool = cf.ThreadPoolExecutor(max_workers=max(1, int(args.io_threads)))
    try:
        reads = collections.deque()
        todo = iter(subjects)

        def prefetch():
            while len(reads) < QUEUE_DEPTH:
                s = next(todo, None)
                if s is None:
                    return
                reads.append((s, pool.submit(_read_subject, s, needed, args.score, options)))

        prefetch()
        calibrated = False
        with ops.prec_plan(plan):
            while reads:
                subject, fut = reads.popleft()
                prefetch()                                         # subject i+1 is read while subject i runs
                try:
                    t0 = time.perf_counter()
                    raws, ev, t_read = fut.result()
                    timing['read'] += t_read
                    if norm != 'percentile':
                        timing['read_wait'] += time.perf_counter() - t0      # the main thread waiting for the read and the moments
                        timing['moments'] += sum(r.moments_s for r in raws)
                    sargs = copy.copy(args)
                    sargs.output_dir = os.path.join(args.output_dir, subject.id)
                    gpu = device or torch.device(f'cuda:{args.gpu_chose}')
                    evaluation, resampled, found = None, [], {}
                    if ev is not None:                             # the evaluation inputs onto the grid of the prediction, checked
                        evaluation, resampled, found = evaluation_inputs(raws[0], *ev, options, gpu, names=(subject.inputs[needed[0]], subject.gt),
                                                                         wording=lambda e: f'ground truth / mask: {e}')
                    torch.manual_seed(args.seed)
                    t0 = time.perf_counter()
                    conds, ref, report = prepare_inputs(list(zip(needed, raws)), options, gpu,      # (--coregister and --bias_correct work
                                                        labels=None if device is None else subject.inputs,      # here: they need the GPU)
                                                        align=found.get('align'))
                    if device is not None:
                        conds = [VI.condition_from_raw(vol, options.half_range, args.image_size, device, name=subject.inputs[m], norm=norm)
                                 for m, vol in zip(needed, conds)]
                        torch.cuda.synchronize(device)
                    report.add_evaluation(resampled, found)
                    sargs.known_inputs = sargs.thick_inputs = sargs.lowres_inputs = None
                    if getattr(args, 'known_thick_volume', None) is not None:      # (the subject's Y: mudiff_hip.thick_volume)
                        from . import thick_volume as TV
                        sargs.known_thick_volume = subject.known if args.known_thick_volume == TV.MANIFEST else args.known_thick_volume
                        if not sargs.known_thick_volume:
                            raise ValueError(f'--known_thick_volume {TV.MANIFEST}: the manifest names no `known` file for this subject')
                        thick = TV.options_from(sargs)
                        sargs.thick_inputs = TV.on_grid(raws[0], TV.read_input(thick, options), thick, options, gpu, align=found.get('align'))
                    elif getattr(args, 'known_lowres_volume', None) is not None:   # (the subject's Y: mudiff_hip.lowres_volume)
                        from . import lowres_volume as LV
                        sargs.known_lowres_volume = subject.known if args.known_lowres_volume == LV.MANIFEST else args.known_lowres_volume
                        if not sargs.known_lowres_volume:
                            raise ValueError(f'--known_lowres_volume {LV.MANIFEST}: the manifest names no `known` file for this subject')
                        lowres = LV.options_from(sargs)
                        sargs.lowres_inputs = LV.on_grid(raws[0], LV.read_input(lowres, options), lowres, options, gpu, align=found.get('align'))
                    elif subject.known:                            # (the subject's --known_volume: mudiff_hip.known_region)
                        from . import known_region as KR
                        sargs.known_volume, sargs.known_mask = subject.known, subject.known_mask
                        known = {module: module.options_from(sargs) for module in V.known_modes() + V.constraint_modes()[-1:]}[KR]      # (each mode's own refusals;
                                                                                                            #  K's options: known_region's)
                        sargs.known_inputs = KR.on_grid(raws[0], KR.read_inputs(known, options), known, options, gpu, align=found.get('align'))
                        report.add_evaluation(list(sargs.known_inputs.resampled), {})
                    sargs.intake_report = report                   # (the [done] line names what it lists)
                    timing['intake'] += time.perf_counter() - t0

                    def write(path, vol, affine, header):
                        drain(QUEUE_DEPTH - 1)                     # subject i-1 is compressed and written while subject i runs
                        pending.append(pool.submit(_timed_write, path, vol, affine, header))

                    write = output_writer(write, raws[0], options, ref, gpu, getattr(args, 'reorient_back', False), getattr(args, 'conform_back', False))

                    t0 = time.perf_counter()
                    stage = {}
                    predict(sargs, plan, evaluation, conds, ref, write, not calibrated, stage)
                    calibrated = True
                    for k in ('sample', 'assemble'):
                        timing[k] += stage.get(k, 0.0)
                    timing['write_wait'] += stage.get('write', 0.0)      # the main thread waiting for an earlier subject's write
                    timing['score'] += max(0.0, time.perf_counter() - t0 - sum(stage.values()))
                    row = dict(id=subject.id, metrics={})
                    if evaluation is not None:
                        with open(os.path.join(sargs.output_dir, f'metrics_{target.lower()}.json')) as f:
                            row = subject_row(subject.id, json.load(f))
                        if getattr(args, 'coverage', None) is not None:
                            with open(os.path.join(sargs.output_dir, f'coverage_{target.lower()}.json')) as f:
                                row['coverage'] = coverage_row(json.load(f))
                    rows.append(row)
                except (OSError, ValueError, EOFError, zlib.error, struct.error) as e:       # (what reading a damaged file raises)
                    failures.append((subject.id, f'{type(e).__name__}: {e}'))
                    print(f'[cohort] skipped {subject.id}: {e}', file=sys.stderr)
        drain(0)
    finally:
        pool.shutdown(wait=True, cancel_futures=True)
    timing['wall'] = time.perf_counter() - t_wall
    agg = aggregate(rows)
    report = dict(target=target, **({} if norm == 'percentile' else dict(norm=norm)), subjects=rows, failed=[dict(id=i, error=e) for i, e in failures], aggregate=agg,
                  std_definition='population standard deviation over subjects (ddof = 0)', timing=timing)
    if getattr(args, 'coverage', None) is not None:      # (--coverage: mean +- std over subjects of empirical and mean_width per region)
        report['coverage'] = aggregate_coverage(rows)
    os.makedirs(args.output_dir, exist_ok=True)
    path = os.path.join(args.output_dir, f'cohort_{target.lower()}.json')
    with open(path, 'w') as f:
        json.dump(report, f, indent=1)
    for ln in format_lines(agg):
        print(ln)
    print(f'[cohort] {len(rows)} of {len(subjects)} subjects in {timing["wall"]:.1f} s; wrote {path}')
    return report, failures


def build_argparser(argv=None):
    """volume.py's parser (shared, not copied) plus the cohort's own flags."""
    from . import volume as V
    p = V.make_parser('MU-Diff cohort volume prediction (MI355X)')
    p.add_argument('--manifest', type=str, default=None, help='TSV with a header row: id, t1, t1ce, t2, flair and optionally gt, mask')
    p.add_argument('--brats_root', type=str, default=None, help='BraTS layout: <root>/<id>/<id>_{t1,t1ce,t2,flair,seg}.nii.gz')
    p.add_argument('--subjects', type=str, default=None, help='with --brats_root: a file with one subject id per line')
    p.add_argument('--score', action='store_true',
                   help='score every prediction (mudiff_hip.volume_metrics) against the subject\'s gt / mask and aggregate the cohort')
    p.add_argument('--io_threads', type=int, default=4, help='host threads that read / gunzip ahead and compress / write behind')
    args = V.finish_args(p, p.parse_args(argv))
    if (args.manifest is None) == (args.brats_root is None):
        p.error('give --manifest FILE, or --brats_root DIR with --subjects LIST')
    if args.brats_root is not None and args.subjects is None:
        p.error('--brats_root needs --subjects LIST')
    if args.io_threads < 1:
        p.error('--io_threads must be >= 1')
    for flag in ('gt_volume', 'eval_mask', 'known_volume', 'known_mask') + tuple(f'input_{m}' for m in MODALITIES):
        if getattr(args, flag) is not None:
            p.error(f'--{flag} names one subject\'s file: a cohort takes its files from the manifest or the BraTS layout')
    return args


def main(argv=None):
    args = build_argparser(argv)
    try:
        subjects = read_manifest(args.manifest) if args.manifest else brats_subjects(args.brats_root, args.subjects, args.target_modality)
    except (OSError, ValueError) as e:
        print(f'error: {e}', file=sys.stderr)
        return 2
    _, failures = run(args, subjects)
    for sid, msg in failures:
        print(f'[cohort] FAILED {sid}: {msg}', file=sys.stderr)
    return 1 if failures else 0


if __name__ == '__main__':
    sys.exit(main())
