"""N4-style bias-field correction of the inputs (--bias_correct; csrc/volume_bias.hip).

Coil-sensitivity shading is a smooth multiplicative ramp across the head.  With --bias_correct every input is divided by an estimate of
it after --regrid / --coregister have put it on the first input's grid and before it is normalised:

    stored voxels --mud_volume_bias_log--> u = log(v) at every shrink-th voxel
    per level (2^l spans per axis), at most `iters` times:
        mud_volume_bias_corrected (c = u - F, min, max, largest change) --> mud_volume_bias_hist --counts--> sharpen() on the host
        --table--> mud_volume_bias_fit (integer sums of the B-spline fit of c - table(c)) --delta / omega--> the level's lattice
    mud_volume_bias_apply: every voxel / exp(F) --> fp32 [Z,Y,X], a volume like a regridded one

The histogram sharpening is N3's (a Wiener deconvolution of the log-intensity histogram by a Gaussian), the fit N4's multilevel
B-spline approximation.  All per-voxel work is the device's; the host sees `bins` counts and two lattices of at most 19^3 integers per
iteration.  The sums are integers: two runs give the same bits.
"""
from __future__ import annotations

import os

import numpy as np
import torch

from . import MudiffHipError
from .volume_intake import DEVICE_DTYPES, upload, write_report_json
from .volume_regrid import RegriddedVolume

MAX_LEVELS, MAX_BINS, MAX_K = 5, 1024, 44
DEFAULTS = dict(shrink=4, levels=4, iters=50, tol=1e-3, bins=200, fwhm=0.15, wiener=0.01)


# ---------------------------------------------------------------------------------------------------
# the host's share: histogram sharpening, the fixed-point scale, the loop
# ---------------------------------------------------------------------------------------------------
def bin_centres(lo, hi, bins):
    return float(lo) + (np.arange(int(bins), dtype=np.float64) + 0.5) * ((float(hi) - float(lo)) / int(bins))


def sharpen(hist, lo, hi, fwhm=0.15, wiener=0.01):
    """N3's sharpening of a histogram of log intensities (`hist[b]` counts in [lo + b w, lo + (b + 1) w), w = (hi - lo) / bins) -> the
    table E[b]: the expected true log intensity of a sample observed at the centre of bin b, fp64 [bins].  The histogram is padded to
    the power of two 2^(ceil(log2 bins) + 1), deconvolved by a Gaussian of FWHM `fwhm` log units with the Wiener filter conj(G) /
    (|G|^2 + wiener), clipped at 0 (U), and E = (G * (U centre)) / (G * U).  Where the denominator vanishes (below 1e-10 of its
    largest value: what an FFT leaves of a zero) the table holds the bin centre; an empty histogram and a flat image (hi <= lo: every
    sample in one bin) return the bin centres.  E is a mean of padded bin centres and is clamped to their range, so that
    |c - E| <= 3 (hi - lo) for every c in [lo, hi] (choose_k relies on it)."""
    h = np.asarray(hist, np.float64).reshape(-1)
    bins = h.size
    lo, hi = float(lo), float(hi)
    centres = bin_centres(lo, hi, bins)
    if bins < 2 or not hi > lo or not h.sum() > 0 or not np.isfinite(h).all():
        return centres
    width = (hi - lo) / bins
    padded = 1 << (int(np.ceil(np.log2(bins))) + 1)
    off = (padded - bins) // 2
    v = np.zeros(padded, np.float64)
    v[off:off + bins] = h
    pc = lo + (np.arange(padded, dtype=np.float64) - off + 0.5) * width
    sf = float(fwhm) / width                                    # the FWHM in bins
    i = np.arange(padded, dtype=np.float64)
    i = np.minimum(i, padded - i)                               # wrap-around distance
    g = 2.0 * np.sqrt(np.log(2.0) / np.pi) / sf * np.exp(-(i * i) * (4.0 * np.log(2.0) / (sf * sf)))
    G = np.fft.fft(g)
    U = np.fft.ifft(np.fft.fft(v) * (np.conj(G) / (np.abs(G) ** 2 + float(wiener)))).real
    U = np.maximum(U, 0.0)
    num = np.fft.ifft(np.fft.fft(U * pc) * G).real
    den = np.fft.ifft(np.fft.fft(U) * G).real
    ok = den > 1e-10 * max(float(den.max()), 0.0)
    E = np.where(ok, num / np.where(ok, den, 1.0), pc)
    return np.clip(E, pc[0], pc[-1])[off:off + bins]


def choose_k(n_samples, lo, hi):
    """The fixed-point scale 2^k of the fit's integer sums.  A sample adds llrint(w^3 r / S2 * 2^k) to delta and llrint(w^2 * 2^k) to
    omega of a control point.  w^3 / S2 <= ((2/3)^3 / (265/576))^3 < 0.27 and w^2 < 1 (the cubic B-spline's largest weight is 2/3, its
    smallest sum of squares 265/576 per axis, at t = 1/2), |r| <= 3 (hi - lo) (sharpen), so each term is below max(hi - lo, 1) * 2^k in magnitude,
    half a unit of rounding included; with n samples |sum| < 2^ceil(log2 n) * 2^ceil(log2 max(hi - lo, 1)) * 2^k, which stays below
    2^62 for k = 62 - ceil(log2 n) - ceil(log2 max(hi - lo, 1)).  Capped at 44: beyond that the products' own fp64 rounding shows."""
    n = max(int(n_samples), 1)
    span = max(float(hi) - float(lo), 1.0) if (lo is not None and hi is not None) else 1.0
    k = 62 - int(np.ceil(np.log2(n))) - int(np.ceil(np.log2(span)))
    return int(min(max(k, 0), MAX_K))


def new_lattices(levels):
    return [np.zeros((n + 3,) * 3, np.float64) for n in (1 << l for l in range(int(levels)))]


def loop(engine, levels=4, iters=50, tol=1e-3, bins=200, fwhm=0.15, wiener=0.01):
    """The estimation loop over an engine (DeviceEngine here, the numpy restatement in the tests): per level at most `iters` times
    corrected -> histogram -> sharpen -> fit; a level ends early when, after one of its fits, the corrected log image moved by less than
    `tol` anywhere.  -> (lattices [fp64 [m][m][m] per level], iterations per level, the last dmax)."""
    lattices = new_lattices(levels)
    iterations, dmax = [], 0.0
    for level in range(int(levels)):
        done = 0
        while True:
            lo, hi, dmax = engine.corrected(lattices)
            if lo is None or (done and dmax < tol) or done >= int(iters):
                break
            scale = float(bins) / (hi - lo) if hi > lo else 0.0
            scale = scale if np.isfinite(scale) else 0.0
            table = sharpen(engine.hist(lo, scale, bins), lo, hi if scale > 0 else lo, fwhm, wiener)
            delta, omega = engine.fit(level, table, lo, scale, choose_k(engine.n_samples, lo, hi))
            d, w = np.asarray(delta).astype(np.float64), np.asarray(omega).astype(np.float64)
            lattices[level] = lattices[level] + np.where(w != 0, d / np.where(w != 0, w, 1.0), 0.0).reshape(lattices[level].shape)
            done += 1
        iterations.append(done)
    return lattices, iterations, float(dmax)


# ---------------------------------------------------------------------------------------------------
# the device's share
# ---------------------------------------------------------------------------------------------------
def _key_to_float(key):
    """The order-preserving uint32 key of an fp32 (sign bit flipped for positives, all bits for negatives) -> python float."""
    key = int(key) & 0xFFFFFFFF
    bits = key ^ 0x80000000 if key & 0x80000000 else key ^ 0xFFFFFFFF
    return float(np.array([bits], np.uint32).view(np.float32)[0])


def flat_lattices(lattices, device):
    """The lattices of levels 0.. as one device fp64 array, level after level, each [cz][cy][cx]."""
    return torch.from_numpy(np.concatenate([np.asarray(L, np.float64).reshape(-1) for L in lattices])).to(device)


class DeviceEngine:
    """The four kernels around one uploaded volume: `dev` the flat device array of the stored voxels, meta = (datatype code, shape
    [X,Y,Z], slope, inter) with slope / inter 1 / 0 for an unscaled file."""

    def __init__(self, dev, meta, shrink):
        from . import ops
        code, shape, slope, inter = meta
        if int(code) not in DEVICE_DTYPES:
            raise MudiffHipError(f'bias correction: unsupported NIfTI datatype code {code}')
        self.dev, self.meta, self.shrink = dev, (int(code), tuple(int(v) for v in shape), float(slope), float(inter)), int(shrink)
        self.shape = self.meta[1]
        self.u = ops.volume_bias_log(dev, *self.meta, self.shrink)
        self.c = [self.u.clone(), torch.empty_like(self.u)]           # previous / new corrected log image
        self.n_samples = int(self.u.numel())

    def corrected(self, lattices):
        from . import ops
        stats = ops.volume_bias_corrected(self.u, self.c[0], self.c[1], flat_lattices(lattices, self.dev.device), len(lattices), self.shape,
                                          self.shrink)
        self.c.reverse()                                              # c[0]: the current corrected log image
        dbits, kmax, kmin = (int(v) for v in stats.cpu().numpy().view(np.uint64))
        if kmin > 0xFFFFFFFF:                                         # no finite sample
            return None, None, 0.0
        return _key_to_float(kmin), _key_to_float(kmax), float(np.array([dbits], np.uint64).view(np.float64)[0])

    def hist(self, lo, scale, bins):
        from . import ops
        return ops.volume_bias_hist(self.c[0], lo, scale, bins).cpu().numpy().view(np.uint32).astype(np.int64)

    def fit(self, level, table, lo, scale, k):
        from . import ops
        sums = ops.volume_bias_fit(self.c[0], torch.from_numpy(np.ascontiguousarray(table, np.float64)).to(self.dev.device), lo, scale,
                                   level, self.shape, self.shrink, k).cpu().numpy()
        return sums[0], sums[1]

    def apply(self, lattices, field=False):
        from . import ops
        return ops.volume_bias_apply(self.dev, *self.meta, flat_lattices(lattices, self.dev.device), len(lattices), field)


class BiasCorrectedVolume(RegriddedVolume):
    """A RawVolume whose voxels live on the device (fp32 [Z,Y,X], the geometry of the volume it was made from), as a regridded one."""


def check_options(shrink, levels, iters, tol, bins, fwhm, wiener):
    """ValueError (with the flag's name) for a value the estimation cannot run with."""
    if int(shrink) < 1:
        raise ValueError(f'--bias_shrink must be >= 1 (got {shrink})')
    if not 1 <= int(levels) <= MAX_LEVELS:
        raise ValueError(f'--bias_levels must be in [1, {MAX_LEVELS}] (got {levels})')
    if int(iters) < 1:
        raise ValueError(f'--bias_iters must be >= 1 (got {iters})')
    if not (np.isfinite(tol) and tol >= 0):
        raise ValueError(f'--bias_tol must be finite and not negative (got {tol})')
    if not 2 <= int(bins) <= MAX_BINS:
        raise ValueError(f'--bias_bins must be in [2, {MAX_BINS}] (got {bins})')
    if not (np.isfinite(fwhm) and fwhm > 0):
        raise ValueError(f'--bias_fwhm must be finite and positive (got {fwhm})')
    if not (np.isfinite(wiener) and wiener > 0):
        raise ValueError(f'--bias_wiener must be finite and positive (got {wiener})')


def correct(raw, device, shrink=4, levels=4, iters=50, tol=1e-3, bins=200, fwhm=0.15, wiener=0.01, field=False):
    """A RawVolume (its voxels on the host, or on the device already: a regridded one) -> (BiasCorrectedVolume, report).  report:
    iterations (per level), dmax (the last one), field_min / field_mean / field_max (the log field F over the masked sample points;
    None without any), samples, masked, and the options.  With `field` the volume also carries `.field`: exp(F) at every voxel as an
    F-ordered fp32 [X,Y,Z] host array."""
    if len(raw.shape) != 3:
        raise ValueError(f'bias correction: expected a 3D volume, got shape {tuple(raw.shape)}')
    check_options(shrink, levels, iters, tol, bins, fwhm, wiener)
    eng = DeviceEngine(upload(raw, device), raw.kernel_meta('bias correction'), shrink)
    lattices, iterations, dmax = loop(eng, levels, iters, tol, bins, fwhm, wiener)
    eng.corrected(lattices)
    u, c = eng.u.cpu().numpy().astype(np.float64), eng.c[0].cpu().numpy().astype(np.float64)
    f = (u - c)[np.isfinite(c)]
    report = dict(iterations=[int(v) for v in iterations], dmax=float(dmax),
                  field_min=float(f.min()) if f.size else None, field_mean=float(f.mean()) if f.size else None,
                  field_max=float(f.max()) if f.size else None, samples=int(u.size), masked=int(f.size), shrink=int(shrink),
                  levels=int(levels), iters=int(iters), tol=float(tol), bins=int(bins), fwhm=float(fwhm), wiener=float(wiener))
    out = BiasCorrectedVolume(eng.apply(lattices), raw.shape, raw.affine, raw.header)
    out.lattices = lattices
    if field:
        out.field = eng.apply(lattices, field=True).cpu().numpy().transpose(2, 1, 0)
    return out, report


# ---------------------------------------------------------------------------------------------------
# the pipeline's side
# ---------------------------------------------------------------------------------------------------
def add_flags(p):
    p.add_argument('--bias_correct', action='store_true',
                   help='divide every input by an estimate of its coil-shading (bias) field before it is normalised: an N4-style '
                        'correction on the GPU (histogram sharpening + multilevel B-spline fit of the log image: '
                        'mudiff_hip.volume_bias), after --regrid / --coregister; bias_<t>.json next to the prediction holds what was '
                        'found.  --gt_volume / --eval_mask are not corrected')
    p.add_argument('--bias_shrink', type=int, default=DEFAULTS['shrink'], help='the field is estimated from every N-th voxel per axis')
    p.add_argument('--bias_levels', type=int, default=DEFAULTS['levels'], help='B-spline levels: level l has 2^l spans per axis (1 to 5)')
    p.add_argument('--bias_iters', type=int, default=DEFAULTS['iters'], help='most iterations per level')
    p.add_argument('--bias_tol', type=float, default=DEFAULTS['tol'], help='a level ends when no sample of the corrected log image moved by more')
    p.add_argument('--bias_bins', type=int, default=DEFAULTS['bins'], help='bins of the log-intensity histogram (2 to 1024)')
    p.add_argument('--bias_fwhm', type=float, default=DEFAULTS['fwhm'], help='FWHM, in log units, of the Gaussian the histogram is deconvolved by')
    p.add_argument('--bias_wiener', type=float, default=DEFAULTS['wiener'], help='noise term of the Wiener deconvolution filter')
    p.add_argument('--bias_field_out', action='store_true',
                   help='with --bias_correct: also write bias_field_<name>_<t>.nii.gz, exp(field) of each input on the output grid')


def options_from(args):
    """A namespace's --bias_* flags (any may be missing) -> IntakeOptions' `bias`: the keyword arguments of correct, or None without
    --bias_correct.  ValueError, naming the flag, for a value check_options refuses and for --bias_field_out on its own."""
    kw = {k: type(v)(getattr(args, 'bias_' + k, v)) for k, v in DEFAULTS.items()}
    check_options(**kw)
    on, field = bool(getattr(args, 'bias_correct', False)), bool(getattr(args, 'bias_field_out', False))
    if field and not on:
        raise ValueError('--bias_field_out needs --bias_correct')
    return dict(bias=dict(kw, field=field) if on else None)


def bias_suffix(reports):
    """What a [done] line gains under --bias_correct (nothing otherwise): ` | bias=<name>,<name>,...`."""
    if not reports:
        return ''
    return ' | bias=' + ','.join(str(r[0]) for r in reports)


def write_reports(reports, output_dir, target, affine=None, header=None):
    """bias_<t>.json next to the prediction: {input name: report}; with --bias_field_out also bias_field_<name>_<t>.nii.gz, exp(F) on
    the output grid.  -> the json's path."""
    path = write_report_json('bias', {r[0]: r[1] for r in reports}, output_dir, target)
    for r in reports:
        if len(r) > 2 and r[2] is not None:
            from .volume import write_nifti
            write_nifti(os.path.join(output_dir, f'bias_field_{str(r[0]).lower()}_{target.lower()}.nii.gz'), r[2],
                        np.eye(4) if affine is None else affine, header)
    return path
