"""On-device NIfTI intake and re-assembly for the volume pipeline (csrc/volume_intake.hip).

The host path of mudiff_hip.volume normalises each input volume with about eight numpy passes over a float64 copy and gathers the
strided [X,Y] planes of the F-ordered volume one by one.  Here the voxels go to the device exactly as the file stores them and three
kernels do the rest:

    raw voxels --upload--> census (count, min, max, 16 exact sorted values around each percentile rank)
               --record to host--> thresholds()  (np.percentile on a surrogate array: numpy's own arithmetic, numpy's own result)
               --lo, den--> slab normalise ([n,1,X,Y], the planes s0..s1 transposed) --> ops.resize_bilinear --> the sampler

and, after sampling, assemble() writes the predicted planes back into a zero-filled volume in file order, which arrives on the host as
an F-contiguous [X,Y,Z] array (volume.write_nifti's tobytes(order='F') is then a straight copy).

Every result equals the host path's bit for bit: the census values are order statistics, the thresholds are np.percentile's own
output, and the normalisation rounds each fp32 step once like numpy.  A volume that holds NaN or inf takes the host path (with a warning).

condition_from_raw is that chain for one volume; which volumes it sees - as stored, resampled (--regrid, --coregister) or bias-corrected -
is volume_prepare.prepare_inputs' business, the same for the host path.

With norm='zscore' (--norm zscore) there is no census: the two moments come from numpy on the host
(zscore_moments, the reference's own calls on the stored array) and slab_zscore does the rest on the device, non-finite voxels included.
"""
from __future__ import annotations

import ctypes as C
import warnings

import numpy as np
import torch

from . import (NIFTI_F4, NIFTI_I2, NIFTI_I4, NIFTI_U1, NIFTI_U2, VI_MAX_RANKS, VI_WINDOW, MudiffHipError, VolumeCensusRecord, load, ptr,  # noqa: F401
               require_gpu)

DEVICE_DTYPES = {NIFTI_U1: 'u1', NIFTI_I2: 'i2', NIFTI_I4: 'i4', NIFTI_F4: 'f4', NIFTI_U2: 'u2'}      # what the kernels read directly


# ---------------------------------------------------------------------------------------------------
# reading a file without converting it
# ---------------------------------------------------------------------------------------------------
class RawVolume:
    """A volume as stored: `data` is the flat voxel array in file order (x fastest) in the file's datatype, or float32 when the file
    had to go through volume.read_nifti (`code` is then NIFTI_F4 and slope / inter are 1 / 0)."""

    def __init__(self, data, code, endian, slope, inter, shape, affine, header):
        self.data, self.code, self.endian = data, int(code), endian
        self.slope, self.inter = float(slope), float(inter)
        self.shape, self.affine, self.header = tuple(int(v) for v in shape), affine, header
        self.moments = None                  # zscore_moments(self), when a prefetch thread has computed them already

    @property
    def scaled(self):
        """volume.read_nifti's rule for applying scl_slope / scl_inter."""
        return self.slope != 0.0 and np.isfinite(self.slope) and (self.slope != 1.0 or self.inter != 0.0)

    @property
    def scaling(self):
        """(slope, inter) as the kernels take them: the file's where read_nifti applies them, else (1, 0)."""
        return (self.slope, self.inter) if self.scaled else (1.0, 0.0)

    def kernel_meta(self, stage):
        """(datatype code, shape [X,Y,Z], slope, inter) as the volume kernels take them; `stage` is what the refusal of a datatype they do
        not read calls the caller."""
        if self.code not in DEVICE_DTYPES:
            raise MudiffHipError(f'{stage}: unsupported NIfTI datatype code {self.code}')
        return (self.code, self.shape) + self.scaling

    def values_float64(self):
        """The [X,Y,Z] float64 array volume.read_nifti returns for this file (the reference conversion)."""
        data = np.asarray(self.data).reshape(self.shape, order='F').astype(np.float64)
        if self.scaled:
            data = data * self.slope + self.inter
        return data


def _via_read_nifti(path):
    from .volume import read_nifti
    vol, affine, header = read_nifti(path)
    vol = np.asarray(vol)
    data = np.ascontiguousarray(vol.astype(np.float32).reshape(-1, order='F'))
    return RawVolume(data, NIFTI_F4, '<', 1.0, 0.0, vol.shape, affine, header)


def read_nifti_raw(path):
    """volume.read_nifti's built-in reader without the float64 conversion -> RawVolume (stored array untouched, datatype code,
    endianness, slope, inter, shape, affine, header).  Big-endian files, datatypes the kernels do not read, non-3D images and
    nibabel-loaded images go through volume.read_nifti and come back as float32 (its values, rounded as the pipeline rounds them)."""
    from .volume import open_nifti1
    try:
        import nibabel  # noqa: F401
        return _via_read_nifti(path)
    except ImportError:
        pass
    buf, hdr, code = open_nifti1(path)
    shape = hdr.shape
    if hdr.endian != '<' or code not in DEVICE_DTYPES or len(shape) != 3:
        return _via_read_nifti(path)
    offset = int(hdr._get('f', 108)[0])
    slope, inter = hdr._get('2f', 112)
    n = int(np.prod(shape))
    data = np.frombuffer(buf, dtype=np.dtype('<' + DEVICE_DTYPES[code]), count=n, offset=offset)
    return RawVolume(data, code, hdr.endian, slope, inter, shape, hdr.affine, hdr)


def write_report_json(kind, payload, output_dir, target):
    """<kind>_<target>.json next to the prediction (every stage's write_reports).  -> its path."""
    import json
    import os
    os.makedirs(output_dir, exist_ok=True)
    path = os.path.join(output_dir, f'{kind}_{target.lower()}.json')
    with open(path, 'w') as f:
        json.dump(payload, f, indent=1)
    return path


# ---------------------------------------------------------------------------------------------------
# census -> thresholds
# ---------------------------------------------------------------------------------------------------
class CensusRecord:
    """Host copy of a mud_volume_census_record: n, n_nonfinite, min, max (np.float32) and per requested fraction the window
    (first_rank, np.float32 values)."""

    def __init__(self, n, n_nonfinite, vmin, vmax, windows):
        self.n, self.n_nonfinite = int(n), int(n_nonfinite)
        self.min, self.max = np.float32(vmin), np.float32(vmax)
        self.windows = [(int(a), np.asarray(w, np.float32)) for a, w in windows]

    @classmethod
    def from_bytes(cls, raw, nq):
        rec = VolumeCensusRecord.from_buffer_copy(raw)
        wins = [(rec.first_rank[i], np.array(rec.window[i][:rec.count[i]], np.float32)) for i in range(nq)]
        return cls(rec.n, rec.n_nonfinite, rec.min, rec.max, wins)

    @classmethod
    def from_sorted(cls, s, fractions):
        """The record the device produces for selected values whose np.sort is `s` (tests, and the definition of the windows)."""
        s = np.asarray(s, np.float32)
        n = int(s.size)
        wins = []
        for q in fractions:
            if n == 0:
                wins.append((0, np.zeros(0, np.float32)))
                continue
            r = int(np.floor(float(n - 1) * float(q)))
            a, b = max(0, r - 8), min(n - 1, r + 7)
            wins.append((a, s[a:b + 1].copy()))
        nonfinite = int((~np.isfinite(s)).sum())
        return cls(n, nonfinite, s[0] if n else 0.0, s[-1] if n else 0.0, wins)


def census(dev_raw, code, shape, slope=1.0, inter=0.0, fractions=(0.01, 0.99)):
    """mud_volume_census on a flat device array of the stored voxels -> device uint8 tensor holding the record (no synchronisation;
    CensusRecord.from_bytes(t.cpu().numpy().tobytes(), len(fractions)) reads it)."""
    require_gpu(dev_raw)
    X, Y, Z = (int(v) for v in shape)
    nq = len(fractions)
    rec = torch.empty(C.sizeof(VolumeCensusRecord), device=dev_raw.device, dtype=torch.uint8)
    nbytes = load().mud_volume_census_ws_bytes()
    ws = torch.empty(nbytes, device=dev_raw.device, dtype=torch.uint8)
    q = (C.c_double * max(nq, 1))(*[float(v) for v in fractions])
    from . import ops
    ops._launch('volume_census', dev_raw.device, load().mud_volume_census, ptr(dev_raw), int(code), X, Y, Z, float(slope), float(inter), q, nq,
                ptr(rec), ptr(ws), nbytes, ops.STREAM, nbytes=5.0 * dev_raw.numel() * dev_raw.element_size())
    return rec


def thresholds(record, pmin=1.0, pmax=99.0):
    """(lo, den, degenerate) of volume.robust_minmax_to_minus1_1 from a CensusRecord whose windows were taken at the fractions
    (pmin / 100, pmax / 100): the volume's normalised value is clip((v - lo) / den, 0, 1) * 2 - 1, or zeros when `degenerate`.

    np.percentile is called on a sorted surrogate of length n that holds the exact minimum below the windows, the exact window values
    inside them and the exact maximum above: numpy's result depends only on n, q and the sorted values at the ranks it picks, which lie
    inside the windows, so this is its result on the data whatever arithmetic the installed numpy uses.  The fallback chain
    (percentiles non-finite or hi <= lo -> min / max; flat -> zeros) is the host function's, with its fp32 rounding of hi - lo."""
    n = record.n
    if n == 0:
        return np.float32(0), np.float32(1), True
    if record.n_nonfinite:
        raise ValueError('thresholds: the volume holds non-finite voxels (use the host path)')
    (a0, w0), (a1, w1) = record.windows[:2]
    s = np.empty(n, np.float32)
    s[:a0] = record.min
    s[a0:a0 + w0.size] = w0
    if a1 > a0 + w0.size:
        s[a0 + w0.size:a1] = w0[-1]
    s[a1:a1 + w1.size] = w1
    s[a1 + w1.size:] = record.max
    lo, hi = np.percentile(s, pmin), np.percentile(s, pmax)
    if not (isinstance(lo, np.float32) and isinstance(hi, np.float32)):
        raise ValueError('thresholds: this numpy does not return float32 percentiles of float32 data (use the host path)')
    if not (np.isfinite(lo) and np.isfinite(hi)) or hi <= lo:
        lo, hi = float(record.min), float(record.max)
        if hi <= lo:
            return np.float32(0), np.float32(1), True
        return np.float32(lo), np.float32(hi - lo), False        # the host divides by the python float hi - lo, cast to fp32
    return lo, np.float32(hi - lo), False


def slab_range(z, half_range):
    c = int(z) // 2
    return max(0, c - int(half_range)), min(int(z) - 1, c + int(half_range))


def slab_normalise(dev_raw, code, shape, slope, inter, lo, den, degenerate, s0, s1):
    """mud_volume_slab_normalise -> device fp32 [s1 - s0 + 1, 1, X, Y]."""
    require_gpu(dev_raw)
    X, Y, Z = (int(v) for v in shape)
    if not 0 <= s0 <= s1 < Z:
        raise MudiffHipError(f'slab_normalise: the slab {s0}..{s1} is not inside the {Z} planes')
    out = torch.empty(s1 - s0 + 1, 1, X, Y, device=dev_raw.device, dtype=torch.float32)
    from . import ops
    ops._launch('volume_slab_normalise', dev_raw.device, load().mud_volume_slab_normalise, ptr(dev_raw), int(code), X, Y, Z, float(slope),
                float(inter), float(lo), float(den), int(bool(degenerate)), int(s0), int(s1), ptr(out), ops.STREAM)
    return out


def zscore_moments(raw):
    """(mean, std) as np.float32 of a RawVolume's non-zero voxels: volume.zscore_moments_f32 (numpy's fp32 reductions, the calls the
    reference makes) on the fp32 values the host path sees, read_nifti(...).astype(float32).  Host work, about 0.1 s for
    240 x 240 x 155 int16 voxels; a cohort does it on the prefetch thread."""
    from .volume import zscore_moments_f32
    stored = np.ascontiguousarray(np.asarray(raw.data).reshape(raw.shape, order='F'))      # C order first, in the small stored dtype:
    if raw.scaled:                                                                         # the gather below then reads memory in order
        data = (stored.astype(np.float64) * raw.slope + raw.inter).astype(np.float32)
    else:
        data = stored.astype(np.float32)          # = float32(float64(stored)): one rounding either way
    return zscore_moments_f32(data)


def slab_zscore(dev_raw, code, shape, slope, inter, mean, std, s0, s1):
    """mud_volume_slab_zscore -> device fp32 [s1 - s0 + 1, 1, X, Y]: clamp((v - mean) / std, -3, 3) / 3 of the planes s0..s1."""
    require_gpu(dev_raw)
    X, Y, Z = (int(v) for v in shape)
    if not 0 <= s0 <= s1 < Z:
        raise MudiffHipError(f'slab_zscore: the slab {s0}..{s1} is not inside the {Z} planes')
    out = torch.empty(s1 - s0 + 1, 1, X, Y, device=dev_raw.device, dtype=torch.float32)
    from . import ops
    ops._launch('volume_slab_zscore', dev_raw.device, load().mud_volume_slab_zscore, ptr(dev_raw), int(code), X, Y, Z, float(slope),
                float(inter), float(mean), float(std), int(s0), int(s1), ptr(out), ops.STREAM)
    return out


def assemble(planes, shape, s0, s1, planes2=None):
    """Device fp32 planes [n, X, Y] (n = s1 - s0 + 1; optionally a second stack) -> device fp32 volume(s) [Z, Y, X]: zeros with the
    planes at s0..s1 (volume.reconstruct_volume_from_slices, in file order).  -> tensor, or a pair with `planes2`."""
    require_gpu(planes, planes2)
    X, Y, Z = (int(v) for v in shape)
    n = s1 - s0 + 1
    for t in (planes,) + (() if planes2 is None else (planes2,)):
        if t.dtype != torch.float32 or tuple(t.shape) != (n, X, Y):
            raise MudiffHipError(f'assemble: need fp32 planes [{n}, {X}, {Y}], got {t.dtype} {tuple(t.shape)}')
    planes = planes.contiguous()
    planes2 = None if planes2 is None else planes2.contiguous()
    vol = torch.empty(Z, Y, X, device=planes.device, dtype=torch.float32)
    vol2 = None if planes2 is None else torch.empty_like(vol)
    from . import ops
    ops._launch('volume_assemble', planes.device, load().mud_volume_assemble, ptr(planes), ptr(planes2), X, Y, Z, int(s0), int(s1), ptr(vol),
                ptr(vol2), ops.STREAM)
    return vol if planes2 is None else (vol, vol2)


def to_host_volume(vol_zyx):
    """Device [Z, Y, X] volume -> F-contiguous host [X, Y, Z] array (one D2H copy; the transpose is a view)."""
    return vol_zyx.cpu().numpy().transpose(2, 1, 0)


# ---------------------------------------------------------------------------------------------------
# the intake of one condition volume (a subject's three: volume_prepare.prepare_inputs, then condition_from_raw on each)
# ---------------------------------------------------------------------------------------------------
def upload(raw, device):
    """RawVolume -> flat device tensor of the stored voxels (uint16 travels as int16 bits: the kernels reinterpret by datatype code).
    A volume that --regrid resampled is on the device already (volume_regrid.RegriddedVolume.dev)."""
    dev = getattr(raw, 'dev', None)
    if dev is not None:
        return dev.reshape(-1).to(device)
    a = np.asarray(raw.data)
    if a.dtype == np.dtype('<u2'):
        a = a.view(np.int16)
    if not a.flags.writeable:                 # (frombuffer views are read-only; torch wants to be told nothing is written)
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            t = torch.from_numpy(a)
    else:
        t = torch.from_numpy(a)
    return t.to(device)


def _host_condition(raw, s0, s1, device):
    """The host path for one volume (non-finite voxels): robust_minmax_to_minus1_1 + the slab's planes, uploaded."""
    from .volume import robust_minmax_to_minus1_1
    norm = robust_minmax_to_minus1_1(raw.values_float64())
    planes = np.ascontiguousarray(np.moveaxis(norm[:, :, s0:s1 + 1], 2, 0), dtype=np.float32)
    return torch.from_numpy(planes).to(device)[:, None]


def condition_from_raw(raw, half_range, image_size, device, pmin=1.0, pmax=99.0, name='volume', norm='percentile'):
    """One RawVolume -> its condition tensor [n, 1, S, S] on the device: upload, census, thresholds, slab normalise, resize; with
    norm='zscore': upload, slab z-score with the host's moments (raw.moments when set, else computed here), resize."""
    from .volume import NORMS
    if norm not in NORMS:
        raise ValueError(f'norm must be one of {NORMS}, got {norm!r}')
    if len(raw.shape) != 3:
        raise ValueError(f'{name}: expected a 3D volume, got shape {raw.shape}')
    s0, s1 = slab_range(raw.shape[2], half_range)
    dev_raw = upload(raw, device)
    slope, inter = raw.scaling
    if norm == 'zscore':
        mean, std = raw.moments if raw.moments is not None else zscore_moments(raw)
        return _resized(slab_zscore(dev_raw, raw.code, raw.shape, slope, inter, mean, std, s0, s1), image_size)
    rec_dev = census(dev_raw, raw.code, raw.shape, slope, inter, (pmin / 100.0, pmax / 100.0))
    rec = CensusRecord.from_bytes(rec_dev.cpu().numpy().tobytes(), 2)
    try:
        lo, den, degenerate = thresholds(rec, pmin, pmax)
        t = slab_normalise(dev_raw, raw.code, raw.shape, slope, inter, lo, den, degenerate, s0, s1)
    except ValueError as e:
        print(f'[intake] warning: {name}: {e}; normalised on the host')
        t = _host_condition(raw, s0, s1, device)
    return _resized(t, image_size)


def _resized(t, image_size):
    from . import ops
    size = int(image_size)
    if tuple(t.shape[-2:]) != (size, size):
        t = ops.resize_bilinear(t, (size, size))
    return t.contiguous()
