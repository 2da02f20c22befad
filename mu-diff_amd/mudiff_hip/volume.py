"""Whole-volume prediction on MI355X.

Mirrors the reference's clinical entry point `engine/test_volume.py` - same functions, flags and outputs:
robust percentile normalisation of each input volume (:135-157), the centre +-half_range axial slices (:159-168),
bilinear resize to the model's image size (:273-274), 4-step dual-generator sampling, mapping to [0,1] (:281),
re-assembly into a volume of the original shape (:170-181) and a NIfTI written next to the inputs' geometry (:296-299).

What is different is the schedule, not the result: the reference pushes ONE slice at a time through the generators
(`for i in range(n)`, :266); here all <= 2*half_range+1 slices of the volume are uploaded once, resized by a HIP
kernel, and sampled in batches of `--batch_size` through one captured hipGraph per reverse step (sampling.GraphSampler).
Slices are independent, so the only observable difference is the order in which Gaussian draws are consumed; parity runs
inject the draws per slice (`predict_slices(..., x_inits, zs, noises)`).  --slice_coupling gives that independence up on purpose
(mudiff_hip.slice_coupling): neighbouring slices then share part of their noise, and the single-sample path draws with the keyed
generator of the ensembles instead of the torch generator.  --through_plane measures what it did (mudiff_hip.volume_through_plane).

Intake: every path reads the three condition files as stored (volume_intake.read_nifti_raw) and hands them to the one preparation
stage, volume_prepare.prepare_inputs; host_stacks then normalises with numpy, --device_intake with volume_intake.condition_from_raw.
What the stage did travels as args.intake_report to the [done] line.  Each stage's flags, defaults and checks live in its own module
(volume_prepare.STAGES lists them): make_parser, finish_args and IntakeOptions.from_args loop over that table.

NIfTI I/O: nibabel is used when importable (it is not in this image); otherwise a minimal built-in reader/writer
handles single-file NIfTI-1 (.nii / .nii.gz, little- or big-endian, scl_slope/inter applied like get_fdata()).
"""
from __future__ import annotations

import argparse
import copy
import gzip
import os
import struct

import numpy as np
import torch

MODALITY_ORDERS = {      # reference engine/test_volume.py:236-241 (same order as dataset/dataset_brats.py:29-34)
    'T1CE': ['FLAIR', 'T2', 'T1'],
    'FLAIR': ['T1CE', 'T1', 'T2'],
    'T2': ['T1CE', 'T1', 'FLAIR'],
    'T1': ['FLAIR', 'T1CE', 'T2'],
}


# ---------------------------------------------------------------------------------------------------
# host-side preprocessing (numpy in the reference too: one pass over a volume, not on the GPU hot path)
# ---------------------------------------------------------------------------------------------------
def robust_minmax_to_minus1_1(vol, mask=None, pmin=1.0, pmax=99.0):
    """Reference :135-157.  Intensities -> [-1,1] through the [pmin,pmax] percentiles of the non-zero voxels (or of
    `mask`, NaNs excluded); values outside are clipped.  No usable voxels or a flat volume -> zeros."""
    data = np.asarray(vol).astype(np.float32, copy=False)
    sel = (data != 0) if mask is None else (np.asarray(mask).astype(bool) & ~np.isnan(data))
    if not sel.any():
        return np.zeros_like(data, dtype=np.float32)
    vals = data[sel]
    lo, hi = np.percentile(vals, pmin), np.percentile(vals, pmax)
    if not (np.isfinite(lo) and np.isfinite(hi)) or hi <= lo:
        lo, hi = float(vals.min()), float(vals.max())
        if hi <= lo:
            return np.zeros_like(data, dtype=np.float32)
    return np.clip((data - lo) / (hi - lo), 0.0, 1.0) * 2.0 - 1.0


NORMS = ('percentile', 'zscore')      # --norm: 'percentile' is the reference's volume entry point, 'zscore' what its training sees


def zscore_moments_f32(data):
    """(mean, std) as np.float32 of the non-zero voxels of an fp32 [X,Y,Z] array: the reference's tools/pre_process.py:53-61 with
    numpy's own fp32 reductions over data[data != 0] (C order).  No such voxels -> (0, 1); a flat volume -> std 1."""
    vals = data[data != 0]
    if vals.size == 0:
        return np.float32(0.0), np.float32(1.0)
    mean, s = vals.mean(), vals.std()
    return np.float32(mean), np.float32(s if s != 0 else 1.0)


def zscore_to_minus1_1(vol):
    """The training normalisation: the reference's tools/pre_process.py:46-67 (z-score over the non-zero
    voxels of the whole volume) followed by dataset/dataset_brats.py:83 (clamp to +-3 sigma, divided by 3), all in fp32.  A NaN voxel
    makes both moments, and with them the whole volume, NaN."""
    data = np.asarray(vol).astype(np.float32, copy=False)
    mean, std = zscore_moments_f32(data)
    z = (data - mean) / std
    return np.clip(z, -3.0, 3.0) / np.float32(3.0)


def normalise_volume(vol, norm='percentile'):
    """--norm: robust_minmax_to_minus1_1 ('percentile', the default) or zscore_to_minus1_1 ('zscore')."""
    if norm not in NORMS:
        raise ValueError(f'norm must be one of {NORMS}, got {norm!r}')
    return zscore_to_minus1_1(vol) if norm == 'zscore' else robust_minmax_to_minus1_1(vol)


def norm_suffix(norm):
    """What a log line gains under a non-default --norm (nothing by default: the lines as they were)."""
    return '' if norm == 'percentile' else f' | norm={norm}'


def regrid_suffix(names):
    """volume_regrid.regrid_suffix, under the name it first had."""
    from .volume_regrid import regrid_suffix as suffix
    return suffix(names)


def extract_center_slices(volume, half_range):
    """Reference :159-168 -> (list of [X,Y] slices, first index, last index)."""
    z = volume.shape[2]
    c = z // 2
    s0, s1 = max(0, c - half_range), min(z - 1, c + half_range)
    return [volume[:, :, k] for k in range(s0, s1 + 1)], s0, s1


def reconstruct_volume_from_slices(predicted_slices, original_shape, start_slice, end_slice):
    """Reference :170-181: zeros everywhere except planes start_slice..end_slice."""
    vol = np.zeros(original_shape, dtype=np.float32)
    for i, sl in enumerate(predicted_slices):
        k = start_slice + i
        if k <= end_slice and k < original_shape[2]:
            vol[:, :, k] = np.asarray(sl, dtype=np.float32)
    return vol


# ---------------------------------------------------------------------------------------------------
# NIfTI-1 (single file) - used only when nibabel is absent
# ---------------------------------------------------------------------------------------------------
_NIFTI_DTYPES = {2: 'u1', 4: 'i2', 8: 'i4', 16: 'f4', 64: 'f8', 256: 'i1', 512: 'u2', 768: 'u4', 1024: 'i8', 1280: 'u8'}


class NiftiHeader:
    """The 348 raw header bytes plus the fields this pipeline needs."""

    def __init__(self, raw, endian):
        self.raw, self.endian = bytes(raw), endian

    def _get(self, fmt, off):
        return struct.unpack_from(self.endian + fmt, self.raw, off)

    @property
    def shape(self):
        dim = self._get('8h', 40)
        return tuple(int(d) for d in dim[1:1 + dim[0]])

    @property
    def affine(self):
        """sform if set, else the pixdim scaling (qform rotations are not interpreted by this minimal reader)."""
        if self._get('h', 254)[0] > 0:
            rows = [self._get('4f', 280 + 16 * r) for r in range(3)]
            return np.array(rows + [(0., 0., 0., 1.)], dtype=np.float64)
        pix = self._get('8f', 76)
        return np.diag([pix[1], pix[2], pix[3], 1.0]).astype(np.float64)

    @property
    def world_affine(self):
        """Voxel index -> world coordinate by NIfTI-1's own precedence: sform if sform_code > 0, else qform if qform_code > 0 (the
        quaternion's rotation, columns scaled by pixdim[1..3], the third also by qfac = pixdim[0], 0 read as +1), else the pixdim
        diagonal.  --regrid places volumes by this matrix (mudiff_hip.volume_regrid); `affine` stays what it was."""
        if self._get('h', 254)[0] > 0 or self._get('h', 252)[0] <= 0:
            return self.affine
        pix = self._get('8f', 76)
        b, c, d = (float(v) for v in self._get('3f', 256))
        a = float(np.sqrt(max(0.0, 1.0 - b * b - c * c - d * d)))
        rot = np.array([[a * a + b * b - c * c - d * d, 2 * (b * c - a * d), 2 * (b * d + a * c)],
                        [2 * (b * c + a * d), a * a + c * c - b * b - d * d, 2 * (c * d - a * b)],
                        [2 * (b * d - a * c), 2 * (c * d + a * b), a * a + d * d - b * b - c * c]], dtype=np.float64)
        qfac = float(pix[0]) if pix[0] != 0 else 1.0
        out = np.eye(4, dtype=np.float64)
        out[:3, :3] = rot * np.array([pix[1], pix[2], pix[3] * qfac], dtype=np.float64)
        out[:3, 3] = self._get('3f', 268)
        return out


def open_nifti1(path):
    """The built-in reader's first half (read_nifti, and volume_intake.read_nifti_raw): -> (the file's bytes, its NiftiHeader, its datatype
    code).  ValueError for what is not a single-file NIfTI-1 image of a known datatype."""
    opener = gzip.open if path.endswith('.gz') else open
    with opener(path, 'rb') as f:
        buf = f.read()
    if len(buf) < 352:
        raise ValueError(f'{path}: too short for a NIfTI-1 file')
    endian = '<' if struct.unpack_from('<i', buf, 0)[0] == 348 else '>'
    if struct.unpack_from(endian + 'i', buf, 0)[0] != 348 or buf[344:347] != b'n+1':
        raise ValueError(f'{path}: not a single-file NIfTI-1 image (sizeof_hdr / magic mismatch)')
    hdr = NiftiHeader(buf[:348], endian)
    code = hdr._get('h', 70)[0]
    if code not in _NIFTI_DTYPES:
        raise ValueError(f'{path}: unsupported NIfTI datatype code {code}')
    return buf, hdr, code


def read_nifti(path):
    """-> (float64 array scaled like nibabel's get_fdata(), affine [4,4], header)."""
    try:
        import nibabel as nib                      # noqa: F401  (preferred when present)
        img = nib.load(path)
        return img.get_fdata(), img.affine, img.header
    except ImportError:
        pass
    buf, hdr, code = open_nifti1(path)
    offset = int(hdr._get('f', 108)[0])
    slope, inter = hdr._get('2f', 112)
    shape = hdr.shape
    n = int(np.prod(shape))
    data = np.frombuffer(buf, dtype=np.dtype(hdr.endian + _NIFTI_DTYPES[code]), count=n, offset=offset).reshape(shape, order='F')
    data = data.astype(np.float64)
    if slope not in (0.0,) and np.isfinite(slope) and (slope != 1.0 or inter != 0.0):
        data = data * slope + inter
    return data, hdr.affine, hdr


def write_nifti(path, vol, affine, header=None):
    """float32 volume + the inputs' geometry -> .nii / .nii.gz (reference :296-298 via nibabel)."""
    try:
        import nibabel as nib
        nib.save(nib.Nifti1Image(vol, affine, header), path)
        return
    except ImportError:
        pass
    write_nifti1(path, np.asarray(vol, dtype=np.float32), affine, header, 16, 32)


def write_nifti1(path, vol, affine, header, code, bitpix):
    """The built-in writer behind write_nifti (float32: datatype code 16, bitpix 32) and volume_foreground.write_mask (uint8: 2, 8):
    `vol` is already of that type.  A little-endian NiftiHeader is reused, geometry fields overwritten; anything else gives a blank one."""
    reuse = isinstance(header, NiftiHeader) and header.endian == '<'
    raw = bytearray(header.raw) if reuse else bytearray(348)
    struct.pack_into('<i', raw, 0, 348)
    dim = [vol.ndim] + list(vol.shape) + [1] * (7 - vol.ndim)
    struct.pack_into('<8h', raw, 40, *dim)
    struct.pack_into('<h', raw, 70, code)         # datatype
    struct.pack_into('<h', raw, 72, bitpix)
    struct.pack_into('<f', raw, 108, 352.0)       # vox_offset
    struct.pack_into('<2f', raw, 112, 1.0, 0.0)   # scl_slope, scl_inter
    if not reuse:
        pix = [1.0] + [float(np.linalg.norm(np.asarray(affine)[:3, i])) for i in range(3)] + [1.0] * 4
        struct.pack_into('<8f', raw, 76, *pix)
    struct.pack_into('<h', raw, 254, 1)           # sform_code: scanner
    for r in range(3):
        struct.pack_into('<4f', raw, 280 + 16 * r, *[float(v) for v in np.asarray(affine)[r]])
    raw[344:348] = b'n+1\0'
    payload = bytes(raw) + b'\0\0\0\0' + vol.tobytes(order='F')
    opener = gzip.open if path.endswith('.gz') else open
    with opener(path, 'wb') as f:
        f.write(payload)


def load_and_preprocess_volume(file_path, slice_half_range, norm='percentile'):
    """Reference :183-191 -> (slices, shape, affine, header, first, last).  `norm`: --norm."""
    vol, affine, header = read_nifti(file_path)
    slices, s0, s1 = extract_center_slices(normalise_volume(vol, norm), slice_half_range)
    return slices, vol.shape, affine, header, s0, s1


def load_checkpoint(template, net, name, device):
    """Reference :193-203: strip 'module.' only where present, strict=False, eval()."""
    ckpt = torch.load(template.format(name), map_location=device, weights_only=True)
    if isinstance(ckpt, dict) and any(k.startswith('module.') for k in ckpt):
        ckpt = {(k[7:] if k.startswith('module.') else k): v for k, v in ckpt.items()}
    net.load_state_dict(ckpt, strict=False)
    net.eval()


# ---------------------------------------------------------------------------------------------------
# batched sampling of a stack of slices
# ---------------------------------------------------------------------------------------------------
def upload_conds(cond_stacks, size, device):
    """Three [n,X,Y] condition stacks -> [n,1,size,size] device tensors: one upload + one resize launch per contrast (reference:
    per slice, on the CPU).  A stack that is a device tensor already ([n,1,X,Y], mudiff_hip.volume_intake) is only resized."""
    from . import ops
    conds = []
    for st in cond_stacks:
        if torch.is_tensor(st):
            t = st.to(device)
        else:
            t = torch.from_numpy(np.ascontiguousarray(st, dtype=np.float32)).to(device)[:, None]
        if tuple(t.shape[-2:]) != (size, size):
            t = ops.resize_bilinear(t, (size, size))
        conds.append(t.contiguous())
    return conds


def calibrate_volume(args, gen1, gen2, cond_stacks, device, batch_size=32):
    """precision.calibrate_plan on the first batch predict_slices will sample (min(batch_size, n) slices: never padded), at the
    model's image size; installs the overrides on gen1 / gen2.  -> Calibration, or None for an empty volume."""
    from . import precision
    from . import sampling as S
    n = int(cond_stacks[0].shape[0])
    if n == 0:
        return None
    bs = min(int(batch_size), n)
    c1, c2, c3 = upload_conds([st[:bs] for st in cond_stacks], int(args.image_size), device)
    return precision.calibrate_plan(S.Posterior_Coefficients(args, device), gen1, c1, gen2, c2, c3, int(args.num_timesteps), args,
                                    threshold=args.calibrate_threshold)


def predict_slices(args, gen1, gen2, cond_stacks, device, batch_size=32, x_inits=None, zs=None, noises=None, seed=None,
                   use_graph=True, progress=None, sampler=None, return_device=False, coupling=None, known=None, resample=1, kspace=None,
                   thick=None, constraint=None):
    """cond_stacks: three float arrays [n,X,Y] in [-1,1] (the condition contrasts, already normalised and sliced), or three device
    tensors [n,1,S,S] (volume_intake.condition_from_raw).  -> [n,S,S] float32 numpy in [0,1], S = args.image_size; with `return_device`
    the device tensor instead (no copy to the host).

    `sampler`: a sampling.GraphSampler built for these generators (any batch size, image_size x image_size) to reuse across
    volumes - warm-up and the two hipGraph captures are then paid once per process instead of once per volume.

    x_inits [n,1,S,S] / zs (per step [n,nz]) / noises (per step [n,1,S,S]) inject the Gaussian draws per slice for
    parity runs; otherwise they are drawn on the device (seeded by `seed` when given).

    `coupling` (--slice_coupling; mudiff_hip.slice_coupling): None, 'shared' or (half_taps, R).  With one the
    draws no longer come from the torch generator: every batch is sampled through GraphSampler.sample_keyed with the keys (global slice,
    sample 0) and `seed` (required, in [0, 2^64)), so neighbouring slices share part of their noise and the result still does not depend
    on the batch size.  Injected draws together with a coupling raise ValueError.
    `known`, `kspace`, `thick` (at most one): what of the target was acquired - (known [n,1,S,S] in [-1,1], mask
    uint8 [n,1,S,S]) on the device (--known_volume), a kspace.KSpaceMeasurement (--known_kspace) or a thick.ThickMeasurement
    (--known_thick) for these n slices, with `resample` what GraphSampler.sample_keyed takes; or `constraint`, any of them as one object
    of mudiff_hip.constraints (its own `resample` counts).  The same keyed road, with the same two refusals; the batches are
    constraints.batches of the constraint's units (a slab longer than the captured batch is a ValueError naming --batch_size), and what
    the sampler returns is handed to the constraint's `record` before the [0,1] map.  A constraint that couples the whole stack
    (`lockstep`: thick_volume.BandMeasurement, section 5.29) goes through GraphSampler.sample_lockstep instead: the same keys, the whole
    state on the device, `record_volume` at the end."""
    from . import ops
    from . import sampling as S
    from .constraints import FREE, batches, of_prediction
    from .slice_coupling import check_coupling
    coupling = check_coupling(coupling)
    constraint, resample = of_prediction('predict_slices', constraint, known, kspace, thick, resample)
    keyed = coupling is not None or constraint is not FREE
    if keyed:
        what = 'a coupling' if constraint is FREE else 'a constraint (known region, k-space or thick-slice measurements)'
        if x_inits is not None or zs is not None or noises is not None:
            raise ValueError(f'predict_slices: injected x_inits / zs / noises cannot be combined with {what} (its draws are keyed)')
        if seed is None or not use_graph:
            raise ValueError(f'predict_slices: {what} needs a seed and the captured sampler (use_graph=True)')
    n = int(cond_stacks[0].shape[0])
    size = int(args.image_size)
    if n == 0:
        return torch.zeros(0, size, size, device=device) if return_device else np.zeros((0, size, size), np.float32)
    conds = upload_conds(cond_stacks, size, device)
    coef = S.Posterior_Coefficients(args, device)
    gen = None
    if seed is not None and not keyed:
        gen = torch.Generator(device=device).manual_seed(int(seed))
    T = int(args.num_timesteps)
    bs = min(int(batch_size), n)
    if sampler is not None:
        if not use_graph:
            raise ValueError('predict_slices: sampler= is a captured hipGraph; it cannot be combined with use_graph=False')
        if (sampler.H, sampler.W) != (size, size) or sampler.g1 is not gen1 or sampler.g2 is not gen2:
            raise ValueError('predict_slices: the sampler was built for other generators or another image size')
        bs = sampler.B                           # the captured batch size wins over batch_size (a short last batch is padded either way;
                                                 # seeded draws are made per slice below, so the result does not depend on it)
    elif use_graph:
        sampler = S.GraphSampler(coef, gen1, gen2, args, bs, size, size, device)
    out = torch.empty(n, size, size, device=device, dtype=torch.float32)

    def padded(t, lo, hi):      # the last batch is padded by repeating its last slice (fixed graph shape), trimmed afterwards
        t = t[lo:hi].to(device)
        return t if hi - lo == bs else torch.cat([t, t[-1:].expand(bs - (hi - lo), *t.shape[1:])], 0)

    if gen is not None and zs is None:
        # seeded run: every slice's draws come from its GLOBAL index (one pass over the generator for the whole volume), so the
        # same seed gives the same volume whatever the batch size or the reused sampler's captured shape (161 slices: 200 MB)
        if x_inits is None:
            x_inits = torch.randn(n, 1, size, size, device=device, generator=gen)
        zs = [torch.randn(n, args.nz, device=device, generator=gen) for _ in range(T)]
        noises = [torch.randn(n, 1, size, size, device=device, generator=gen) for _ in range(T)]
    if keyed and constraint.lockstep:        # the constraint couples the whole stack: every slice one step, then all constrained at once
        constraint.over(n, 'predict_slices')
        keys = torch.stack([torch.arange(n, dtype=torch.int64), torch.zeros(n, dtype=torch.int64)], 1)
        fake = sampler.sample_lockstep(conds, keys, seed, T, constraint=constraint, coupling=coupling, resample=resample)
        constraint.record_volume(fake, sampler.lockstep_x_new)
        out.copy_(ops.to_range_0_1(fake)[:, 0])
        if progress:
            progress(n, n)
        return out if return_device else out.cpu().numpy()
    if keyed:                                # row r of a batch is slice items[r]; a short batch is padded by its last slice
        constraint.over(n, 'predict_slices')
        done = 0
        for items in batches(constraint.units(0, n), bs):
            m = len(items)
            rows = items + [items[-1]] * (bs - m)
            idx = torch.as_tensor(rows, dtype=torch.int64)
            keys = torch.stack([idx, torch.zeros(bs, dtype=torch.int64)], 1)
            bound = constraint.for_rows(rows, None, m)
            idx = idx.to(device)
            fake = sampler.sample_keyed(*(c.index_select(0, idx) for c in conds), keys, seed, T, coupling=coupling, constraint=bound,
                                        resample=resample)
            constraint.record(bound, fake, sampler.thick_x_new)
            out[items[0]:items[0] + m] = ops.to_range_0_1(fake)[:m, 0]
            done += m
            if progress:
                progress(done, n)
        return out if return_device else out.cpu().numpy()
    for lo in range(0, n, bs):
        hi = min(lo + bs, n)
        c1, c2, c3 = (padded(c, lo, hi) for c in conds)
        x0 = padded(x_inits, lo, hi) if x_inits is not None else torch.randn(bs, 1, size, size, device=device)
        kw = {}
        if zs is not None:
            kw = dict(zs=[padded(z, lo, hi) for z in zs], noises=[padded(e, lo, hi) for e in noises])
        if sampler is not None:
            fake = sampler.sample(c1, c2, c3, x0, T, **kw)
        else:
            fake = S.sample_from_model(coef, gen1, c1, gen2, c2, c3, T, x0, None, args, **kw)
        out[lo:hi] = ops.to_range_0_1(fake)[:hi - lo, 0]
        if progress:
            progress(hi, n)
    return out if return_device else out.cpu().numpy()


def predict_volume(args):
    """Reference :209-300, same flags, same output file `predicted_<target>.nii.gz`.  With --num_samples the ensemble's mean goes
    there and its std next to it; the return value is then the pair of paths.  --prec_plan holds for the whole prediction.
    With --gt_volume (and --eval_mask) the written prediction is scored afterwards (mudiff_hip.volume_metrics): the lines are printed
    after the [done] line and metrics_<target>.json goes next to the prediction.  Those inputs are checked first, before any GPU or
    checkpoint work.  An input stage (volume_prepare.STAGES; each module's header says what it does) adds its report file, and what its
    *_out flag asks for, next to the prediction (volume_prepare.IntakeReport.write).  Under --reorient and --conform everything is sampled,
    scored and written on the reoriented / the conform grid; --reorient_back and --conform_back return the prediction (and its std) to the
    first input's own grid as it is written, after the scoring (volume_prepare.output_writer).  --slice_coupling couples the draws of
    neighbouring slices (predict_slices' `coupling`); --through_plane adds through_plane_<target>.json and one [through-plane] line
    after the scores (mudiff_hip.volume_through_plane).  With --num_samples, --ensemble_quantiles writes per-voxel quantile maps of the
    samples next to the mean and the std, --ensemble_center median makes the median the written and scored prediction, and --coverage
    counts how often the ground truth lies between two of the maps (mudiff_hip.ensemble, mudiff_hip.volume_coverage).  --known_volume keeps
    the acquired part of the target: it conditions the sampling and is pasted into every written map, known_<target>.json goes next to the
    prediction and the scores gain the regions known / synthesised (mudiff_hip.known_region).  With --known_kspace
    (mudiff_hip.kspace, section 5.26) or --known_thick (mudiff_hip.thick, section 5.27) that volume's measured Fourier coefficients or slab
    averages condition the sampling instead, nothing is pasted, and kspace_<target>.json or thick_<target>.json (and under
    --kspace_zero_filled / --thick_interp the baseline volume) goes next to the prediction; --known_multislice (mudiff_hip.multislice,
    section 5.28) is both at once, with multislice_<target>.json and --multislice_baseline.  --known_thick_volume (mudiff_hip.thick_volume,
    section 5.29) takes the measurement from a thick-slice file of its own geometry instead of --known_volume: the whole stack is sampled in
    lockstep, with thick_volume_<target>.json and --thick_volume_baseline.  --known_lowres_volume (mudiff_hip.lowres_volume, section 5.31) does
    the same for a file that is coarser in all three axes, with lowres_volume_<target>.json and --lowres_volume_baseline.  --known_sense
    (mudiff_hip.sense, section 5.32) measures --known_volume through several coils and pulls every step towards that measurement by a
    regularised conjugate-gradient step, with sense_<target>.json and --sense_baseline."""
    evaluation, resampled, found = _load_eval_inputs(args)
    args = copy.copy(args)                               # the run's own copy: it carries the record of what the intake did
    args.evaluation_record = (resampled, found)          # (for _predict_volume's report: IntakeReport.add_evaluation)
    args.known_inputs = _load_known_inputs(args, found)  # (--known_volume: K and M on the prediction's grid, checked, or None)
    if args.known_inputs is not None:
        args.evaluation_record = (resampled + list(args.known_inputs.resampled), found)
    from . import lowres_volume, thick_volume
    args.thick_inputs = _load_own_grid_inputs(args, found, thick_volume)       # (--known_thick_volume: Y checked against the prediction's grid, or None)
    args.lowres_inputs = _load_own_grid_inputs(args, found, lowres_volume)     # (--known_lowres_volume: likewise)
    from . import ops
    from .driver import effective_prec_plan
    plan = effective_prec_plan(args)
    with ops.prec_plan(plan):
        return _predict_volume(args, plan, evaluation)


def _needed_inputs(args):
    """[(modality, path)] of the target's three condition contrasts, in MODALITY_ORDERS order."""
    if args.target_modality not in MODALITY_ORDERS:
        raise ValueError(f'Unsupported target modality: {args.target_modality}')
    needed = MODALITY_ORDERS[args.target_modality]
    provided = {'T1CE': args.input_t1ce, 'T1': args.input_t1, 'T2': args.input_t2, 'FLAIR': args.input_flair}
    for m in needed:
        if not provided.get(m):
            raise ValueError(f'Missing required input for {m}. Provide --input_{m.lower()}')
    return [(m, provided[m]) for m in needed]


def load_eval_inputs(args):
    """--gt_volume / --eval_mask -> None, or (raw GT volume, label volume or None) once the files have been read and put on the grid the
    prediction will have and their shapes checked against it and the slab (volume_prepare.evaluation_inputs says which grid that is
    under which flags; volume_metrics.check_shapes).  A bad evaluation input raises ValueError here, so that it cannot cost a sampling
    run."""
    return _load_eval_inputs(args)[0]


def _load_eval_inputs(args):
    """load_eval_inputs -> (its result, the names of the evaluation inputs that were resampled, volume_regrid.eval_onto_grid's `found`)."""
    if args.gt_volume is None:
        if args.eval_mask is not None:
            raise ValueError('--eval_mask needs --gt_volume')
        return None, [], {}
    from . import volume_prepare as VP
    _, first = _needed_inputs(args)[0]
    options = VP.IntakeOptions.from_args(args)
    read = lambda path: VP.read_for_evaluation(path, options)      # noqa: E731
    return VP.evaluation_inputs(read(first), read(args.gt_volume), read(args.eval_mask), options, torch.device(f'cuda:{args.gpu_chose}'),
                                names=(first, args.gt_volume),
                                wording=lambda e: f'--gt_volume / --eval_mask: {e} (the prediction has the shape of {first})')


def _load_known_inputs(args, found):
    """--known_volume / --known_mask -> None, or known_region.KnownInputs: the files read and put on the grid the prediction will have
    (known_region.on_grid), before any checkpoint work.  A bad flag or shape raises ValueError here.  `found`: _load_eval_inputs' (its
    alignment, when it has one, is used)."""
    from . import known_region as KR
    known = KR.options_from(args)
    if known is None:
        return None
    from . import volume_prepare as VP
    _, first = _needed_inputs(args)[0]
    options = VP.IntakeOptions.from_args(args)
    return KR.on_grid(VP.read_for_evaluation(first, options), KR.read_inputs(known, options), known, options,
                      torch.device(f'cuda:{args.gpu_chose}'), align=found.get('align'))


def _load_own_grid_inputs(args, found, TV):
    """A measurement given as a file on a grid of its own, TV = thick_volume (--known_thick_volume) or lowres_volume
    (--known_lowres_volume) -> None, or TV's ThickInputs / LowresInputs: the file read and its geometry checked against the grid the
    prediction will have (TV.on_grid), before any checkpoint work.  A bad flag or geometry raises ValueError here."""
    options = TV.options_from(args)
    if options is None:
        return None
    from . import volume_prepare as VP
    _, first = _needed_inputs(args)[0]
    intake = VP.IntakeOptions.from_args(args)
    return TV.on_grid(VP.read_for_evaluation(first, intake), TV.read_input(options, intake), options, intake,
                      torch.device(f'cuda:{args.gpu_chose}'), align=found.get('align'))


def _score_prediction(args, evaluation, vol, std_vol, device):
    """Scores of the prediction exactly as written -> printed lines and <output_dir>/metrics_<target>.json (its path)."""
    from . import volume_metrics as VM
    gt, label = evaluation
    region = getattr(args, 'known_region', None)         # (--known_volume: the regions `known` and `synthesised` as well)
    from . import known_region as KR
    more = {} if region is None else dict(more_regions=lambda s0, s1, bit: (KR.region_bits(region, s0, s1, bit), KR.REGION_NAMES))
    rep = VM.score_arrays(vol, gt, label, std_vol, args.slice_half_range, device, norm=args.norm, **more)
    for ln in VM.format_lines(rep):
        print(ln)
    path = VM.write_json(rep, os.path.join(args.output_dir, f'metrics_{args.target_modality.lower()}.json'))
    print(f'[metrics] wrote {path}')
    return path


def load_generators(args, device):
    """The two generators of --exp on `device`, checkpoints loaded (reference :193-203)."""
    from backbones.ncsnpp_generator_adagn_feat import NCSNpp, NCSNpp_adaptive
    gen1, gen2 = NCSNpp(args).to(device), NCSNpp_adaptive(args).to(device)
    tmpl = os.path.join(args.output_path, args.exp, '{}.pth')
    load_checkpoint(tmpl, gen1, 'gen_diffusive_1', device)
    load_checkpoint(tmpl, gen2, 'gen_diffusive_2', device)
    return gen1, gen2


def _predict_volume(args, plan, evaluation=None):
    torch.manual_seed(args.seed)
    torch.cuda.set_device(args.gpu_chose)
    device = torch.device(f'cuda:{args.gpu_chose}')
    gen1, gen2 = load_generators(args, device)
    from . import volume_intake as VI
    from .volume_prepare import IntakeOptions, output_writer, prepare_inputs
    options = IntakeOptions.from_args(args)
    needed = _needed_inputs(args)
    raws = [VI.read_nifti_raw(path) for _, path in needed]
    prepared, ref, report = prepare_inputs([(m, raw) for (m, _), raw in zip(needed, raws)], options, device,
                                           labels=dict(needed) if args.device_intake else None,      # (the device path names the file)
                                           align=getattr(args, 'evaluation_record', ([], {}))[1].get('align'))      # (--gt_volume: estimated already)
    write = output_writer(write_nifti, raws[0], options, ref, device, getattr(args, 'reorient_back', False), getattr(args, 'conform_back', False))
    report.add_evaluation(*getattr(args, 'evaluation_record', ([], {})))      # the inputs first, then what predict_volume resampled
    args.intake_report = report
    if args.device_intake:
        stacks = [VI.condition_from_raw(vol, options.half_range, args.image_size, device, name=path, norm=options.norm)
                  for vol, (_, path) in zip(prepared, needed)]
    else:
        stacks = host_stacks(prepared, options)
    return predict_from_conditions(args, plan, evaluation, gen1, gen2, device, stacks, ref, on_device=args.device_intake, write=write)


def host_stacks(prepared, options):
    """The host's normalisation of volume_prepare.prepare_inputs' volumes -> one [n,X,Y] condition stack each.  An untouched file gives
    the float64 array read_nifti returns; a volume that a stage made on the device is downloaded as the fp32 it is."""
    from .volume_regrid import RegriddedVolume
    stacks = []
    for vol in prepared:
        values = vol.values_float32() if isinstance(vol, RegriddedVolume) else vol.values_float64()
        stacks.append(np.stack(extract_center_slices(normalise_volume(values, options.norm), options.half_range)[0], 0))
    return stacks


def _intake_report(args):
    """The run's volume_prepare.IntakeReport (args.intake_report; absent means empty)."""
    from .volume_prepare import IntakeReport
    return getattr(args, 'intake_report', None) or IntakeReport()


def _done_tail(args, plan):
    """What a [done] line ends in: the arithmetic plan, --norm, what the intake did, --slice_coupling and the ensemble's centre and
    quantiles, each only when it is not the default."""
    from .ensemble import done_suffix
    from .known_region import suffix as known_suffix
    from .slice_coupling import suffix
    constraint = getattr(args, 'constraint', None)
    return (('' if plan == 'auto' else f' | prec_plan={plan}') + norm_suffix(args.norm) + _intake_report(args).suffix() +
            suffix(getattr(args, 'slice_coupling', None)) + done_suffix(args) + known_suffix(getattr(args, 'known_region', None)) +
            ('' if constraint is None else constraint.done_suffix()))


class _Stages:
    """Per-stage seconds of predict_from_conditions for a caller that asks (mudiff_hip.cohort): each stage ends in a device
    synchronise.  Without a dict nothing is timed and nothing is synchronised."""

    def __init__(self, timing, device):
        self.timing, self.device = timing, device

    def run(self, name, fn):
        if self.timing is None:
            return fn()
        import time
        torch.cuda.synchronize(self.device)
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize(self.device)
        self.timing[name] = self.timing.get(name, 0.0) + time.perf_counter() - t0
        return out


def predict_from_conditions(args, plan, evaluation, gen1, gen2, device, stacks, ref, on_device=False, samplers=None, write=None,
                            calibrate=True, timing=None):
    """Everything after the intake: `stacks` are the three condition stacks (host [n,X,Y], or device [n,1,S,S] with `on_device`, which
    also keeps the prediction on the device until volume_intake.assemble has put it in file order), `ref` = (shape, affine, header, s0,
    s1).  `samplers`: a dict that keeps the captured GraphSamplers by (batch, image_size) across calls; `write`: replaces write_nifti
    (same arguments; a cohort defers it to a thread); `calibrate=False` skips --calibrate (done on an earlier subject); `timing`: a
    dict that receives the seconds of the stages sample / assemble / write."""
    shp, aff, hdr, s0, s1 = ref
    write = write or write_nifti
    stages = _Stages(timing, device)
    if tuple(shp[:2]) != (args.image_size, args.image_size) and not args.resize_back:
        # the reference fails here too, later and less clearly (numpy broadcast error at :179 when the [S,S] prediction is
        # written into an [X,Y] plane); --resize_back is this build's opt-in extension
        raise ValueError(f'in-plane size {tuple(shp[:2])} differs from --image_size {args.image_size}: the prediction cannot be '
                         'written back into the volume (pass --resize_back to resample it bilinearly)')
    if args.calibrate and calibrate:
        cal = calibrate_volume(args, gen1, gen2, stacks, device, batch_size=args.batch_size)
        if cal is not None:
            from .driver import write_calibration
            print(f'[calibrate] {cal.summary()}')
            print(f'[calibrate] wrote {write_calibration(cal, args.output_dir)}')
    region, constraint = _known_region(args, ref, device)
    if args.num_samples is not None:
        return _predict_volume_ensemble(args, gen1, gen2, stacks, device, ref, evaluation, on_device, samplers, write, stages, region, constraint)
    n = int(stacks[0].shape[0])
    sampler = _cached_sampler(args, gen1, gen2, device, samplers, min(int(args.batch_size), n)) if n else None
    pred = stages.run('sample', lambda: predict_slices(args, gen1, gen2, stacks, device, batch_size=args.batch_size, seed=args.seed,
                                                       progress=lambda d, n: print(f'[infer] processed {d}/{n} slices'), sampler=sampler,
                                                       return_device=on_device, coupling=_coupling(args), constraint=constraint))
    if on_device:
        def put_together():
            from . import ops
            from . import volume_intake as VI
            p = pred if tuple(shp[:2]) == tuple(pred.shape[1:]) else ops.resize_bilinear(pred, shp[:2])
            return VI.to_host_volume(VI.assemble(p, shp, s0, s1))
        vol_pred = stages.run('assemble', put_together)
    else:
        if tuple(shp[:2]) != tuple(pred.shape[1:]):
            from . import ops
            pred = ops.resize_bilinear(torch.from_numpy(pred).to(device), shp[:2]).cpu().numpy()
        vol_pred = reconstruct_volume_from_slices(list(pred), shp, s0, s1)
    os.makedirs(args.output_dir, exist_ok=True)
    out_path = os.path.join(args.output_dir, f'predicted_{args.target_modality.lower()}.nii.gz')
    if region is not None:
        from . import known_region as KR
        vol_pred = stages.run('assemble', lambda: KR.paste(vol_pred, region, device))      # the acquired voxels, exactly, in what is written
        KR.write_json(region, args.output_dir, args.target_modality)
    stages.run('write', lambda: write(out_path, vol_pred, aff, hdr))
    _measurement_outputs(args, write, lambda p: _assemble_map(p, shp, s0, s1, on_device), aff, hdr, evaluation, device)
    _intake_report(args).write(args.output_dir, args.target_modality, aff, hdr)
    print(f'[done] saved: {out_path} | shape={tuple(vol_pred.shape)} | slices={s0}..{s1}' + _done_tail(args, plan))
    if evaluation is not None:
        _score_prediction(args, evaluation, vol_pred, None, device)
    _through_plane(args, evaluation, vol_pred, device)
    return out_path


def known_modes():
    """The modules of the four ways a target can be partly acquired, in the order their flags are checked."""
    from . import known_region, kspace, multislice, thick
    return known_region, kspace, thick, multislice


def measurement_modes():
    """known_modes() and, after them, the mode whose measurement is a file of its own and not --known_volume measured retrospectively:
    --known_thick_volume (mudiff_hip.thick_volume)."""
    from . import thick_volume
    return known_modes() + (thick_volume,)


def sampling_modes():
    """measurement_modes() and, after them, the mode whose file is coarser than the prediction in all three axes: --known_lowres_volume
    (mudiff_hip.lowres_volume).  Every module that can put a constraint on the sampler, in the order their flags
    are checked."""
    from . import lowres_volume
    return measurement_modes() + (lowres_volume,)


def constraint_modes():
    """sampling_modes() and, after them, the mode that measures --known_volume through several coils: --known_sense (mudiff_hip.sense,
    DESIGN.md section 5.32).  The functions before this one keep the contents the tests of their modes pin; this one is what the parser,
    the refusals and the cohort visit."""
    from . import sense
    return sampling_modes() + (sense,)


def _known_region(args, ref, device):
    """--known_volume: (the run's known_region.KnownRegion, or None when K is measured in k-space or in thick slices instead: nothing
    is pasted; the one constraint that predict_slices and sample_ensemble take, or None), also left in args.known_region and
    args.constraint for the [done] line, the scores and the measurement's outputs."""
    inputs = getattr(args, 'known_inputs', None)
    args.known_region = args.constraint = None
    thick = getattr(args, 'thick_inputs', None)
    if thick is not None:                                # --known_thick_volume: the measurement itself, nothing pasted (section 5.29)
        from . import thick_volume as TV
        args.constraint = TV.measure(thick, ref, int(args.image_size), args.norm, device)
        return None, args.constraint
    lowres = getattr(args, 'lowres_inputs', None)
    if lowres is not None:                               # --known_lowres_volume: likewise, coarse in all three axes (section 5.31)
        from . import lowres_volume as LV
        args.constraint = LV.measure(lowres, ref, int(args.image_size), args.norm, device)
        return None, args.constraint
    if inputs is None:
        return None, None
    from . import known_region as KR
    region = KR.compose(inputs, ref, args.norm, device)
    args.constraint = KR.constraint_for(region, ref[3], ref[4], int(args.image_size), args, device)
    args.known_region = region if args.constraint.tag is None else None      # the known voxels themselves: pasted, and scored as regions
    return args.known_region, args.constraint


def _assemble_map(p, shp, s0, s1, on_device):
    """A device map [n,S,S] -> the host volume [X,Y,Z] the prediction's road gives it: resized back, the slab's planes put in place."""
    from . import ops
    p = p if tuple(shp[:2]) == tuple(p.shape[1:]) else ops.resize_bilinear(p.contiguous(), shp[:2])
    if on_device:
        from . import volume_intake as VI
        return VI.to_host_volume(VI.assemble(p, shp, s0, s1))
    return reconstruct_volume_from_slices(list(p.cpu().numpy()), shp, s0, s1)


def _measurement_outputs(args, write, put_together, aff, hdr, evaluation, device):
    """--known_kspace / --known_thick / --known_multislice / --known_sense: the measurement's report (kspace_<t>.json, thick_<t>.json,
    multislice_<t>.json, sense_<t>.json) next to the prediction, and under its flag its baseline (zero_filled_<t>.nii.gz,
    thick_interp_<t>.nii.gz, multislice_baseline_<t>.nii.gz, sense_baseline_<t>.nii.gz), mapped to [0,1], through the prediction's own road
    (`put_together`: a device [n,S,S] map -> the host volume as written; a baseline that is a host [X,Y,Z] array already, lowres_volume's,
    is written as it is and scored once normalised by --norm as the ground truth is); with an evaluation it is scored into metrics_<name>_<t>.json,
    and where the measurement says so --through_plane measures it into through_plane_<name>_<t>.json.  Nothing without the flags."""
    meas = getattr(args, 'constraint', None)
    if meas is None or meas.tag is None:
        return
    from . import ops
    target = args.target_modality.lower()
    print(f'[{meas.tag}] wrote {meas.write_json(args.output_dir, args.target_modality)}')
    baseline = meas.baseline()
    if baseline is None:
        return
    name, volume = baseline
    line = '[' + name.replace('_', '-') + '] '
    if isinstance(volume, np.ndarray):
        vol = volume
        scored = np.ascontiguousarray(normalise_volume(volume, args.norm), dtype=np.float32)
        scored = ops.to_range_0_1(torch.from_numpy(scored).to(device)).cpu().numpy()
    else:
        vol = scored = put_together(ops.to_range_0_1(volume))
    path = os.path.join(args.output_dir, f'{name}_{target}.nii.gz')
    write(path, vol, aff, hdr)
    print(f'[{meas.tag}] wrote {path}')
    if evaluation is not None:
        from . import volume_metrics as VM
        rep = VM.score_arrays(scored, evaluation[0], evaluation[1], None, args.slice_half_range, device, norm=args.norm)
        for ln in VM.format_lines(rep):
            print(line + ln)
        print(f"[metrics] wrote {VM.write_json(rep, os.path.join(args.output_dir, f'metrics_{name}_{target}.json'))}")
    if meas.baseline_through_plane and getattr(args, 'through_plane', False):
        from . import volume_through_plane as TP
        rep = TP.measure_arrays(scored, None if evaluation is None else evaluation[0], None, args.slice_half_range, device, norm=args.norm)
        print(line + TP.format_line(rep))
        print(f"[through-plane] wrote {TP.write_json(rep, os.path.join(args.output_dir, f'through_plane_{name}_{target}.json'))}")


def _coupling(args):
    """--slice_coupling as the samplers take it (slice_coupling.coupling_from_flag; a namespace without the flag: None)."""
    from .slice_coupling import coupling_from_flag
    return coupling_from_flag(getattr(args, 'slice_coupling', None))


def _through_plane(args, evaluation, vol, device):
    """--through_plane: the roughness of the prediction exactly as written (and of --gt_volume when given) -> one printed line and
    <output_dir>/through_plane_<target>.json (its path; None without the flag).  metrics_<t>.json is not touched."""
    if not getattr(args, 'through_plane', False):
        return None
    from . import volume_through_plane as TP
    gt = None if evaluation is None else evaluation[0]
    rep = TP.measure_arrays(vol, gt, None, args.slice_half_range, device, norm=args.norm)
    print(TP.format_line(rep))
    path = TP.write_json(rep, os.path.join(args.output_dir, f'through_plane_{args.target_modality.lower()}.json'))
    print(f'[through-plane] wrote {path}')
    return path


def _cached_sampler(args, gen1, gen2, device, samplers, batch):
    """None without a cache (the callee captures its own sampler, as ever); else the cache's GraphSampler for (batch, image_size),
    captured on first use."""
    if samplers is None:
        return None
    from . import sampling as S
    size = int(args.image_size)
    key = (int(batch), size)
    if key not in samplers:
        samplers[key] = S.GraphSampler(S.Posterior_Coefficients(args, device), gen1, gen2, args, int(batch), size, size, device)
    return samplers[key]


def _predict_volume_ensemble(args, gen1, gen2, stacks, device, ref, evaluation=None, on_device=False, samplers=None, write=None,
                             stages=None, region=None, constraint=None):
    """--num_samples: every slice sampled N times with draws keyed by (--seed, slice, sample) (mudiff_hip.ensemble); the mean and
    the std of the [0,1]-mapped samples, resized back and re-assembled like the single prediction, go to predicted_<t>.nii.gz and
    predicted_<t>_std.nii.gz.  With `evaluation` the mean is scored, the std feeding the uncertainty block.  -> (mean path, std path).
    Under --ensemble_quantiles / --ensemble_center median / --coverage (ensemble.quantile_plan) the per-voxel
    quantile maps take the same road to predicted_<t>_q<PPP>.nii.gz, the median replaces the mean as the centre, and coverage_<t>.json
    follows the scores.  `region`, `constraint` (--known_volume): _known_region's pair; every written map then carries the acquired voxels
    (the std: 0 there)."""
    from . import ensemble, ops
    from .driver import effective_prec_plan
    shp, aff, hdr, s0, s1 = ref
    size = int(args.image_size)
    conds = upload_conds(stacks, size, device)
    print(f'[infer] {conds[0].shape[0]} slices x {args.num_samples} samples')
    write = write or write_nifti
    stages = stages or _Stages(None, device)
    sampler = _cached_sampler(args, gen1, gen2, device, samplers, args.batch_size)
    qplan = ensemble.quantile_plan(args)
    res = stages.run('sample', lambda: ensemble.sample_ensemble(args, gen1, gen2, conds, args.num_samples, args.seed,
                                                                batch_size=args.batch_size, map_0_1=True, sampler=sampler,
                                                                coupling=_coupling(args), quantiles=qplan and qplan.computed,
                                                                constraint=constraint))
    mean, std = res[:2]
    qmaps = list(res[2]) if qplan is not None else []                # one [n,S,S] map per computed fraction
    os.makedirs(args.output_dir, exist_ok=True)
    if tuple(shp[:2]) != tuple(mean.shape[1:]):
        mean, std = (stages.run('assemble', lambda t=t: ops.resize_bilinear(t, shp[:2])) for t in (mean, std))
        qmaps = [stages.run('assemble', lambda t=t: ops.resize_bilinear(t.contiguous(), shp[:2])) for t in qmaps]
    if on_device:
        from . import volume_intake as VI
        vols = stages.run('assemble', lambda: [VI.to_host_volume(v) for v in VI.assemble(mean, shp, s0, s1, std)])
        qvols = [stages.run('assemble', lambda t=t: VI.to_host_volume(VI.assemble(t.contiguous(), shp, s0, s1))) for t in qmaps]
    else:
        vols = [reconstruct_volume_from_slices(list(t.cpu().numpy()), shp, s0, s1) for t in (mean, std)]
        qvols = [reconstruct_volume_from_slices(list(t.cpu().numpy()), shp, s0, s1) for t in qmaps]
    quantile_vols = {} if qplan is None else dict(zip(qplan.computed, qvols))
    if region is not None:                                           # the acquired voxels, exactly, in every map that is written; std 0 there
        from . import known_region as KR
        vols = [stages.run('assemble', lambda v=v, k=k: KR.paste(v, region, device, std=k == 1)) for k, v in enumerate(vols)]
        quantile_vols = {q: stages.run('assemble', lambda v=v: KR.paste(v, region, device)) for q, v in quantile_vols.items()}
        KR.write_json(region, args.output_dir, args.target_modality)
    if qplan is not None and qplan.center == 'median':
        vols[0] = quantile_vols[0.5]                                 # the centre: what is written, scored and measured from here on
    paths = []
    for suffix, vol in (('', vols[0]), ('_std', vols[1])) + tuple((ensemble.quantile_suffix(q), quantile_vols[q]) for q in (qplan.written if qplan else ())):
        path = os.path.join(args.output_dir, f'predicted_{args.target_modality.lower()}{suffix}.nii.gz')
        stages.run('write', lambda: write(path, vol, aff, hdr))
        paths.append(path)
    _measurement_outputs(args, write, lambda p: _assemble_map(p, shp, s0, s1, on_device), aff, hdr, evaluation, device)
    _intake_report(args).write(args.output_dir, args.target_modality, aff, hdr)
    print(f'[done] saved: {paths[0]} and {paths[1]} | shape={tuple(shp)} | slices={s0}..{s1} | {args.num_samples} samples per slice' +
          _done_tail(args, effective_prec_plan(args)))
    if evaluation is not None:
        _score_prediction(args, evaluation, vols[0], vols[1], device)
        if qplan is not None and qplan.coverage is not None:
            _coverage(args, evaluation, quantile_vols[qplan.coverage[0]], quantile_vols[qplan.coverage[1]], qplan.coverage, device)
    _through_plane(args, evaluation, vols[0], device)
    return tuple(paths[:2])


def _coverage(args, evaluation, lo_vol, hi_vol, fractions, device):
    """--coverage: how often the ground truth lies between the two quantile volumes exactly as written -> one printed line per region and
    <output_dir>/coverage_<target>.json (its path).  metrics_<t>.json is not touched."""
    from . import volume_coverage as VC
    gt, label = evaluation
    rep = VC.measure_arrays(lo_vol, hi_vol, gt, label, args.slice_half_range, device, norm=args.norm, nominal=fractions[1] - fractions[0])
    rep['quantiles'] = [float(fractions[0]), float(fractions[1])]
    for ln in VC.format_lines(rep):
        print(ln)
    path = VC.write_json(rep, os.path.join(args.output_dir, f'coverage_{args.target_modality.lower()}.json'))
    print(f'[coverage] wrote {path}')
    return path


class VolumeParser(argparse.ArgumentParser):
    """The volume pipeline's parser: an ArgumentParser whose option list is the one tests/test_volume_cli_host.py pins, and `late`, a
    second parser for the flags of the stages that came after that list was pinned (a stage's add_flags puts them there:
    volume_align).  `late`'s own list is pinned by now as well (tests/test_volume_align_host.py), so `later()` opens one more parser of
    the same kind for what came after it (slice_coupling).  parse_args hands each of them what the parsers before it did not know, into
    the same namespace, and refuses what none knows; the help lists them all."""

    def __init__(self, prog):
        super().__init__(prog)
        self.late = argparse.ArgumentParser(prog, add_help=False, usage=argparse.SUPPRESS)
        self.lates = [self.late]

    def later(self):
        """A further late parser, consulted after the ones before it."""
        self.lates.append(argparse.ArgumentParser(self.prog, add_help=False, usage=argparse.SUPPRESS))
        return self.lates[-1]

    def parse_args(self, args=None, namespace=None):
        namespace, rest = self.parse_known_args(args, namespace)
        for late in self.lates:
            namespace, rest = late.parse_known_args(rest, namespace)
        if rest:
            self.error('unrecognized arguments: ' + ' '.join(rest))
        return namespace

    def format_help(self):
        return super().format_help() + ''.join('\n' + late.format_help() for late in self.lates)


def make_parser(prog='MU-Diff volume prediction (MI355X)'):
    """The volume pipeline's parser, unparsed (mudiff_hip.cohort adds its own flags to it; finish_args checks the result)."""
    p = VolumeParser(prog)
    for m in ('t1ce', 't1', 't2', 'flair'):
        p.add_argument(f'--input_{m}', type=str, help=f'Path to {m.upper()} NIfTI')
    p.add_argument('--target_modality', type=str, required=True, choices=['T1CE', 'FLAIR', 'T2', 'T1'])
    p.add_argument('--output_dir', type=str, required=True)
    p.add_argument('--exp', type=str, required=True, help='Experiment directory name under --output_path')
    p.add_argument('--output_path', type=str, default='./results')
    p.add_argument('--slice_half_range', type=int, default=80)
    p.add_argument('--image_size', type=int, default=256)
    p.add_argument('--seed', type=int, default=1024)
    p.add_argument('--num_channels', type=int, default=1)
    p.add_argument('--num_channels_dae', type=int, default=128)
    p.add_argument('--n_mlp', type=int, default=3)
    p.add_argument('--ch_mult', nargs='+', type=int, default=[1, 2, 4])
    p.add_argument('--num_res_blocks', type=int, default=2)
    p.add_argument('--attn_resolutions', nargs='+', type=int, default=[16])
    p.add_argument('--dropout', type=float, default=0.0)
    p.add_argument('--resamp_with_conv', action='store_false', default=True)
    p.add_argument('--conditional', action='store_false', default=True)
    p.add_argument('--fir', action='store_false', default=True)
    p.add_argument('--fir_kernel', nargs='+', type=int, default=[1, 3, 3, 1])
    p.add_argument('--skip_rescale', action='store_false', default=True)
    p.add_argument('--resblock_type', type=str, default='biggan')
    p.add_argument('--progressive', type=str, default='none')
    p.add_argument('--progressive_input', type=str, default='residual')
    p.add_argument('--progressive_combine', type=str, default='sum')
    p.add_argument('--embedding_type', type=str, default='positional')
    p.add_argument('--fourier_scale', type=float, default=16.0)
    p.add_argument('--not_use_tanh', action='store_true', default=False)
    p.add_argument('--centered', action='store_false', default=True)
    p.add_argument('--nz', type=int, default=100)
    p.add_argument('--z_emb_dim', type=int, default=256)
    p.add_argument('--t_emb_dim', type=int, default=256)
    p.add_argument('--num_timesteps', type=int, default=4)
    p.add_argument('--use_geometric', action='store_true', default=False)
    p.add_argument('--beta_min', type=float, default=0.1)
    p.add_argument('--beta_max', type=float, default=20.0)
    p.add_argument('--use_bf16', action='store_true', default=False, help='accepted for compatibility; the MI355X path is fp32')
    p.add_argument('--gpu_chose', type=int, default=0)
    p.add_argument('--batch_size', type=int, default=32, help='slices per captured reverse step (MI355X build)')
    p.add_argument('--resize_back', action='store_true', help='resample the prediction to the in-plane size of the inputs')
    p.add_argument('--num_samples', type=int, default=None,
                   help='sample every slice N >= 2 times with draws keyed by --seed (mudiff_hip.ensemble): predicted_<t>.nii.gz is then '
                        'the mean of the [0,1]-mapped samples, and predicted_<t>_std.nii.gz their per-voxel standard deviation')
    p.add_argument('--gt_volume', type=str, default=None,
                   help='ground-truth NIfTI of the target contrast: score the written prediction on the GPU (PSNR / SSIM3D / MAE per '
                        'region, mudiff_hip.volume_metrics) and write metrics_<t>.json next to it')
    p.add_argument('--eval_mask', type=str, default=None,
                   help='label NIfTI (e.g. a BraTS segmentation; needs --gt_volume): adds the tumor (label != 0) and healthy regions')
    p.add_argument('--device_intake', action='store_true',
                   help='normalise, slice and re-assemble the volumes on the GPU (mudiff_hip.volume_intake): the same files, bit for '
                        'bit, without the numpy passes over each volume')
    p.add_argument('--norm', type=str, default='percentile', choices=list(NORMS),
                   help="how the input volumes (and --gt_volume) are mapped to [-1, 1]: 'percentile' = 1st / 99th percentile min-max "
                        "(the reference's volume entry point); 'zscore' = z-score over the non-zero voxels, clamped to +-3 sigma and "
                        "divided by 3 (what the reference's training and 2D test data see: use it with such a checkpoint)")
    from .volume_prepare import STAGES
    for stage in STAGES:                    # (each input stage's own flags: <module>.add_flags)
        stage.module.add_flags(p)
    from .driver import add_calibration_flags
    add_calibration_flags(p)                # (also --prec_plan)
    from . import slice_coupling
    slice_coupling.add_flags(p)             # (--slice_coupling, --through_plane: in a late parser, VolumeParser.later())
    for module in sampling_modes()[-1:] + known_modes()[1:] + constraint_modes()[-1:] + measurement_modes()[-1:] + known_modes()[:1]:
        module.add_flags(p)                 # (each mode's flags in a late parser of its own; the places of --known_volume's and
                                            #  --known_thick_volume's, the last two, are pinned, so the later modes' came before them)
    from . import ensemble
    ensemble.add_flags(p)                   # (--ensemble_quantiles, --ensemble_center, --coverage: in a further one)
    return p


def finish_args(p, args):
    """The checks that follow parsing (p.error on a bad combination) -> args."""
    from .driver import check_prec_plan_flags
    check_prec_plan_flags(p, args)
    if args.num_samples is not None and args.num_samples < 2:
        p.error(f'--num_samples must be >= 2 (got {args.num_samples})')
    if args.num_samples is not None and not 0 <= args.seed < 1 << 64:
        p.error('--num_samples needs a --seed in [0, 2^64)')
    from . import slice_coupling
    try:
        if slice_coupling.parse_flag(getattr(args, 'slice_coupling', None)) is not None and not 0 <= args.seed < 1 << 64:
            p.error('--slice_coupling needs a --seed in [0, 2^64)')
    except ValueError as e:
        p.error(str(e))
    from . import ensemble
    try:
        ensemble.quantile_plan(args)                     # (its ValueError names the flag)
    except ValueError as e:
        p.error(str(e))
    for module in constraint_modes()[:-3:-1] + measurement_modes():      # (--known_sense, then --known_lowres_volume: each refuses every mode
                                                                         #  before it by its own name)
        try:
            module.options_from(args)                    # (its ValueError names the flag)
        except ValueError as e:
            p.error(str(e))
    from . import volume_conform as VCF
    from . import volume_reorient as VO
    from .volume_prepare import STAGES
    if args.reorient_to is None and args.conform:        # not given: it follows --conform_to under --conform
        args.reorient_to = args.conform_to
    for stage in STAGES:
        try:
            stage.module.options_from(args)              # (a stage's checks: its ValueError names the flag)
        except ValueError as e:
            p.error(str(e))
    # the namespace keeps the checked spelling: upper-case codes, the default filled in, three integers, three spacings
    args.conform_to, args.reorient_to = VO.check_target(args.conform_to), VO.check_target(args.reorient_to or VO.DEFAULT_TARGET)
    args.conform_shape, args.conform_spacing = list(VCF._shape3(args.conform_shape)), list(VCF._spacing3(args.conform_spacing))
    if args.conform and args.reorient and args.conform_to != args.reorient_to:
        p.error(f'--conform_to {args.conform_to} differs from --reorient_to {args.reorient_to}: give both the same code')
    return args


def build_argparser(argv=None):
    """Flags and defaults of the reference parser (:302-357; like it, returns the PARSED namespace), plus --centered (which the
    generators read and the reference parser forgot) and this build's own: the pipeline-wide ones make_parser adds after the
    reference's (their help texts say what they do and name their modules), --calibrate / --calibrate_threshold / --prec_plan
    (mudiff_hip.driver), and the flags of every input stage, each added and checked by the stage's own module (volume_prepare.STAGES;
    DESIGN.md sections 5.12 - 5.22; --align's flags sit in VolumeParser.late), and --slice_coupling / --through_plane (mudiff_hip.slice_coupling,
    DESIGN.md section 5.23; in a further late parser), and --ensemble_quantiles / --ensemble_center / --coverage (mudiff_hip.ensemble,
    mudiff_hip.volume_coverage; in one more), and --known_volume / --known_mask / --known_drop_slices /
    --known_resample, --known_kspace with the --kspace_* flags, --known_thick with the --thick_* flags and --known_multislice with the
    --multislice_* flags (known_modes(); DESIGN.md sections 5.24a - 5.28; each in a parser of its own before that last one), and
    --known_thick_volume with the --thick_volume_* flags (measurement_modes(); section 5.29; likewise), and --known_lowres_volume with the
    --lowres_volume_* flags (sampling_modes(); section 5.31; likewise), and --known_sense with the --sense_* flags (constraint_modes();
    section 5.32; likewise)."""
    p = make_parser()
    return finish_args(p, p.parse_args(argv))


if __name__ == '__main__':
    # run the package's copy of this module: volume_intake imports it by name, and NiftiHeader must be one class for both
    from mudiff_hip import volume as _volume
    _volume.predict_volume(_volume.build_argparser())
