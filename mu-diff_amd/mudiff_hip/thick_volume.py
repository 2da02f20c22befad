"""Sample a target given as a thick-slice volume of its own geometry (--known_thick_volume; csrc/band.hip: mud_band_constrain,
mud_band_measure; GraphSampler.sample_lockstep).

--known_thick (mudiff_hip.thick) measures a thin target retrospectively.  The user that module names as the most common one has no thin
target: there is a real 2D multi-slice scan Y of the target - 5 mm slices with a slice spacing and an origin of their own, contiguous,
overlapping or with gaps - next to 3D conditioning contrasts at 1 mm, and through-plane super-resolution is wanted:

    Y --volume_prepare.read_for_evaluation (--reorient applies)--> geometry against the prediction's grid --> A [m, n]
      --norm, resize--> y [m,S,S] --> sampler (every step: x <- x - A^T (A A^T)^-1 (A (x - s eta) - a y)) --> prediction

Geometry.  Y must share the prediction grid's in-plane geometry: the same first two shape entries, in-plane affine columns and origin
equal within 1e-3 mm, the slice axis parallel within 1e-3 rad.  Anything else is refused: resampling or registering a thick volume
in-plane is out of scope.  From the two affines thick slice j has its centre c_j in thin-slice index units, and it is T / thin_dz thin
slices wide (--thick_volume_thickness_mm T; default Y's own slice spacing: contiguous slices; larger: overlap; smaller: a gap).  Thin
slice i covers [i - 1/2, i + 1/2], and row j of A is
    box    the overlap length of [c_j - T/2, c_j + T/2] with each thin slice,
    gauss  a Gaussian of FWHM = T, cut at c_j +- T, integrated over each thin slice (erf differences),
normalised to sum 1: fp64 numpy, a function of the flags and the two affines alone (--thick_volume_profile).

A thick slice is measured when its support lies wholly inside the sampled range, it is finite on every pixel and --thick_volume_drop
does not name it; the others leave A, and thin slices under no measured row are sampled freely.  Thick slices that cut thin slices in
fractions, or overlap, share thin slices: G = A A^T is a banded SPD matrix and the projection is a banded Cholesky solve along z per
pixel (ops.band_constrain).  ops.band_tables refuses more than 256 measured thick or 512 thin slices, 32 thin slices per thick one, a
bandwidth above 8 and cond(G) > 1e4 (coincident or nearly dependent slices).

The constraint couples the whole stack, so no batch can keep what it couples together (`lockstep`): the samplers advance every (slice,
sample) of the prediction one reverse step and then constrain them all in one launch (GraphSampler.sample_lockstep).  The state of
the whole prediction lives on the device, 2 N n S^2 x 4 bytes for N samples; sample_ensemble refuses up front, naming --num_samples,
when that does not fit.

Y is normalised by --norm from its own non-zero voxels, as K is.  For 'percentile' that is an affine map, which commutes with the slice
average; the zscore clamp at 3 sigma does not (the average of clamped thin voxels is not the clamped average), so under --norm zscore
y is only approximately A k for the k the model was trained on: the effect on trained weights is unmeasured.  Y is resized to S x S like
the conditions.

There is no final paste.  thick_volume_<t>.json lists the geometry, T, the profile, cond(G), the bandwidth and per thick slice its
centre, whether it was measured and |A x - y| / |y| of the sampler's result (the largest over an ensemble's samples; ops.band_measure).
--thick_volume_baseline also writes and scores thick_volume_interp_<t>.nii.gz, piecewise linear in z through (c_j, y_j).  A cohort
takes each subject's Y from the manifest's `known` column under `--known_thick_volume manifest`.

Out of scope: in-plane resampling or registration of Y; multi-coil or in-plane-undersampled thick volumes; a profile per slice; the
uncaptured (use_graph=False) path; the 2D driver.  A Y that is coarser in-plane as well goes to --known_lowres_volume
(mudiff_hip.lowres_volume, section 5.31), which measures it on its own grid in all three axes.
"""
from __future__ import annotations

import collections
import math

import numpy as np
import torch

from .constraints import Constraint, level_tables, need_keyed_seed, relative_residual

PROFILES = ('box', 'gauss')
MANIFEST = 'manifest'
TOL_MM, TOL_RAD = 1e-3, 1e-3
_OTHERS = ('known_volume', 'known_kspace', 'known_thick', 'known_multislice', 'known_mask', 'known_drop_slices')


def add_flags(p):
    p = p.later() if hasattr(p, 'later') else p          # volume.VolumeParser: the lists of the parsers before this one are pinned
    p.add_argument('--known_thick_volume', type=str, default=None, metavar='Y',
                   help='the target contrast as a thick-slice NIfTI with a slice spacing and origin of its own (same in-plane grid as the '
                        'prediction): every thick slice is a weighted average of thin slices and the sampler re-imposes those averages '
                        'after every reverse step - through-plane super-resolution (mudiff_hip.thick_volume, DESIGN.md section 5.29); '
                        f"'{MANIFEST}' in a cohort: the manifest's `known` column")
    p.add_argument('--thick_volume_thickness_mm', type=float, default=None, metavar='T',
                   help='with --known_thick_volume: the slice thickness in mm (default: Y\'s slice spacing = contiguous slices; larger: '
                        'overlap; smaller: a gap)')
    p.add_argument('--thick_volume_profile', type=str, default=None, choices=list(PROFILES),
                   help='with --known_thick_volume: the slice profile, box (the default) or gauss (FWHM = T, cut at +-T)')
    p.add_argument('--thick_volume_drop', type=str, nargs='+', default=None, metavar='A:B',
                   help='with --known_thick_volume: thick slices A..B (inclusive, indices of Y) that were not acquired')
    p.add_argument('--thick_volume_baseline', action='store_true',
                   help='with --known_thick_volume: also write thick_volume_interp_<t>.nii.gz, the thick slices interpolated linearly '
                        'along z (what one would have without the model; scored too under --gt_volume)')


def _drop_ranges(values):
    out = []
    for v in values or ():
        parts = str(v).split(':')
        try:
            a, b = (int(x) for x in parts) if len(parts) == 2 else (None, None)
        except ValueError:
            a = b = None
        if a is None or a < 0 or b < a:
            raise ValueError(f'--thick_volume_drop takes ranges A:B of thick slices with 0 <= A <= B, got {v!r}')
        out.append((a, b))
    return out


def options_from(args):
    """A namespace's --known_thick_volume / --thick_volume_* flags (any may be missing) -> None without --known_thick_volume, else
    dict(volume, thickness, profile, drop [(a, b)], baseline, resample).  ValueError, naming the flag, for a dependent flag without
    --known_thick_volume, for --known_thick_volume together with --known_volume or a flag that rests on it, `manifest` outside a cohort,
    a bad value and a seed outside [0, 2^64)."""
    volume = getattr(args, 'known_thick_volume', None)
    T, profile, drop = (getattr(args, f, None) for f in ('thick_volume_thickness_mm', 'thick_volume_profile', 'thick_volume_drop'))
    baseline = bool(getattr(args, 'thick_volume_baseline', False))
    if volume is None:
        for flag, given in (('--thick_volume_thickness_mm', T is not None), ('--thick_volume_profile', profile is not None),
                            ('--thick_volume_drop', drop is not None), ('--thick_volume_baseline', baseline)):
            if given:
                raise ValueError(f'{flag} needs --known_thick_volume')
        return None
    for other in _OTHERS:
        if getattr(args, other, None) is not None:
            raise ValueError(f'--known_thick_volume cannot be combined with --{other}: Y is the measurement itself, on its own grid '
                             '(--known_volume and the modes on it measure a thin target retrospectively)')
    cohort = getattr(args, 'manifest', None) is not None or getattr(args, 'brats_root', None) is not None
    if volume == MANIFEST and not cohort:
        raise ValueError(f"--known_thick_volume {MANIFEST} needs a cohort (--manifest): it takes each subject's file from the `known` column")
    if T is not None and not (math.isfinite(T) and T > 0):
        raise ValueError(f'--thick_volume_thickness_mm must be a positive number of millimetres, got {T}')
    profile = 'box' if profile is None else profile
    if profile not in PROFILES:
        raise ValueError(f'--thick_volume_profile must be one of {PROFILES}, got {profile!r}')
    resample = getattr(args, 'known_resample', 1)
    resample = 1 if resample is None else resample
    if int(resample) != resample or resample < 1:
        raise ValueError(f'--known_resample must be an integer >= 1, got {resample}')
    need_keyed_seed(args, '--known_thick_volume')
    return dict(volume=volume, thickness=None if T is None else float(T), profile=profile, drop=_drop_ranges(drop), baseline=baseline,
                resample=int(resample))


# ---------------------------------------------------------------------------------------------------
# geometry and weights: numpy fp64, functions of the flags and the two affines alone
# ---------------------------------------------------------------------------------------------------
def slice_geometry(grid_shape, grid_affine, y_shape, y_affine):
    """The prediction grid and Y as (shape, world affine) -> dict(c0, step: thick slice j is centred at thin index c0 + j * step;
    thin_dz, thick_dz in mm; m).  ValueError, naming in-plane resampling as out of scope, unless Y shares the grid's in-plane geometry
    (see the module's header)."""
    a, b = np.asarray(grid_affine, np.float64), np.asarray(y_affine, np.float64)
    out_of_scope = ' (resampling or registering a thick volume in-plane is out of scope: bring Y onto the inputs\' in-plane grid first)'
    if len(y_shape) != 3:
        raise ValueError(f'--known_thick_volume: expected a 3D volume, got shape {tuple(y_shape)}')
    if tuple(int(v) for v in y_shape[:2]) != tuple(int(v) for v in grid_shape[:2]):
        raise ValueError(f'--known_thick_volume: in-plane shape {tuple(y_shape[:2])} differs from the prediction grid\'s '
                         f'{tuple(grid_shape[:2])}' + out_of_scope)
    dz, dy = float(np.linalg.norm(a[:3, 2])), float(np.linalg.norm(b[:3, 2]))
    if not (dz > 0 and dy > 0):
        raise ValueError('--known_thick_volume: an affine has a slice axis of length 0')
    axis = a[:3, 2] / dz
    cosine = float(np.dot(b[:3, 2] / dy, axis))
    sine = float(np.linalg.norm(np.cross(b[:3, 2] / dy, axis)))
    if cosine <= 0 or math.atan2(sine, cosine) > TOL_RAD:
        raise ValueError(f'--known_thick_volume: its slice axis is not parallel to the prediction grid\'s (angle {math.atan2(sine, cosine):.4g} rad)' +
                         out_of_scope)
    for k in (0, 1):
        if float(np.abs(a[:3, k] - b[:3, k]).max()) > TOL_MM:
            raise ValueError(f'--known_thick_volume: in-plane affine column {k} differs from the prediction grid\'s by more than {TOL_MM} mm' +
                             out_of_scope)
    d = b[:3, 3] - a[:3, 3]
    along = float(np.dot(d, axis))
    if float(np.abs(d - along * axis).max()) > TOL_MM:
        raise ValueError(f'--known_thick_volume: its origin is shifted in-plane against the prediction grid\'s by more than {TOL_MM} mm' +
                         out_of_scope)
    return dict(c0=along / dz, step=dy * cosine / dz, thin_dz=dz, thick_dz=dy, m=int(y_shape[2]))


def support(c, width, profile):
    """[lo, hi] in thin-slice index units of the thick slice centred at c, `width` thin slices thick."""
    half = width / 2.0 if profile == 'box' else width
    return c - half, c + half


def weight_rows(n, centres, width, profile='box'):
    """fp64 [len(centres), n]: row j holds the weights of the thick slice centred at thin index centres[j] over thin slices 0..n-1
    (thin slice i covers [i - 1/2, i + 1/2]); each row sums to 1 (0 where nothing overlaps)."""
    c = np.asarray(centres, np.float64).reshape(-1, 1)
    lo_i = np.arange(n, dtype=np.float64).reshape(1, -1) - 0.5
    hi_i = lo_i + 1.0
    if profile == 'box':
        A = np.clip(np.minimum(hi_i, c + width / 2.0) - np.maximum(lo_i, c - width / 2.0), 0.0, None)
    elif profile == 'gauss':
        k = 2.0 * math.sqrt(math.log(2.0)) / width                    # 1 / (sigma sqrt 2), sigma = width / (2 sqrt(2 ln 2))
        p, q = np.maximum(lo_i, c - width), np.minimum(hi_i, c + width)
        erf = np.vectorize(math.erf)
        A = np.where(q > p, 0.5 * (erf((q - c) * k) - erf((p - c) * k)), 0.0)
    else:
        raise ValueError(f'weight_rows: profile must be one of {PROFILES}, got {profile!r}')
    s = A.sum(1, keepdims=True)
    return np.where(s > 0, A / np.where(s > 0, s, 1.0), 0.0)


# ---------------------------------------------------------------------------------------------------
# the measurement of one prediction
# ---------------------------------------------------------------------------------------------------
class BandMeasurement(Constraint):
    """What the samplers take for one prediction of n thin slices (local index i = slice s0 + i): `y` fp32 [m,S,S] on the device, the
    measured thick slices; `A` fp64 [m, n], their rows over the local thin slices; `tables`: ops.band_tables(A) (None when nothing was
    measured: the prediction is then sampled freely, still in lockstep); `report`: thick_volume_<t>.json without the residuals;
    `resample`: --known_resample; `centres` [m]: the measured slices' centres in local index units (for the baseline)."""
    lockstep = True
    tag, baseline_through_plane = 'thick_volume', True

    def __init__(self, y, A, resample=1, report=None, options=None, centres=None):
        from . import ops
        A = np.asarray(A, np.float64)
        self.y, self.A, self.resample = y, A, int(resample)
        self.m, self.n = int(A.shape[0]), int(A.shape[1])
        if tuple(y.shape[:1]) != (self.m,):
            raise ValueError(f'BandMeasurement: y holds {y.shape[0]} thick slices, A {self.m}')
        self.tables = ops.band_tables(A) if self.m else None
        self.report = dict(report or {})
        self.options = dict(options or {})
        self.centres = None if centres is None else np.asarray(centres, np.float64)
        dev = y.device
        self.y_norm = torch.linalg.vector_norm(y.flatten(1), dim=1) if self.m else torch.zeros(0, device=dev)
        self.residual = torch.zeros(self.m, device=dev, dtype=torch.float32)
        self.x_new_norm = torch.zeros(self.n, device=dev, dtype=torch.float32)
        self._work = None

    def chunk_end(self, s0, s1):
        return self.n                                # the whole stack is one chunk

    def check_volume(self, sampler, rows):
        if rows % self.n:
            raise ValueError(f'GraphSampler.sample_lockstep: {rows} rows are not whole stacks of {self.n} slices')
        want = (self.m, sampler.H, sampler.W)
        if self.y.dtype != torch.float32 or tuple(self.y.shape) != want:
            raise ValueError(f'GraphSampler.sample_lockstep: thick volume y must be fp32 {want}, got {self.y.dtype} {tuple(self.y.shape)}')
        self._y = self.y.to(sampler.x.device).contiguous()
        need = (rows // self.n) * self.m * sampler.H * sampler.W
        if self.m and (self._work is None or self._work.numel() != need or self._work.device != sampler.x.device):
            self._work = torch.empty(need, device=sampler.x.device, dtype=torch.float32)

    def apply_volume(self, sampler, x_new, x, keys_dev, seed, step, clean):
        from . import ops
        if not self.m:
            x.copy_(x_new)
            return
        ops.band_constrain_into(x, x_new, self._y, self.tables, self._work, keys_dev, seed, step, ops.KIND_BAND, sampler.t_rows, 0,
                                *level_tables(sampler), clean=clean)

    def record_volume(self, x, x_new=None):
        """x [sets * n,1,S,S]: what the sampler returned (in [-1,1], before any map): keeps, per thick slice, the largest
        |A x - y| / |y| over the sets, and per thin slice the largest |x_new| of what the last constraint was given: with |y|, what the
        residual's rounding scales with."""
        from . import ops
        if not self.m:
            return
        sets = x.shape[0] // self.n
        xs = x.reshape(sets, self.n, -1)
        d = ops.band_measure(xs.contiguous(), self.tables) - self.y.reshape(1, self.m, -1)
        self.residual = torch.maximum(self.residual, relative_residual(d, self.y_norm).amax(0))
        xn = xs if x_new is None else x_new.reshape(sets, self.n, -1)
        self.x_new_norm = torch.maximum(self.x_new_norm, torch.linalg.vector_norm(xn, dim=2).amax(0))

    def interpolated(self):
        return interpolate(self.y, self.centres, self.n)

    def baseline(self):
        return ('thick_volume_interp', self.interpolated()) if self.options.get('baseline') else None

    def finish(self):
        """The report with the residuals put in (None for a thick slice that was not measured)."""
        res, yn = self.residual.cpu().tolist(), self.y_norm.cpu().tolist()
        rep, g = dict(self.report), 0
        rep['slices'] = [dict(s) for s in rep.get('slices', [dict(measured=True) for _ in res])]
        for s in rep['slices']:
            s['residual'], s['y_norm'] = (res[g], yn[g]) if s['measured'] else (None, None)
            g += 1 if s['measured'] else 0
        rep['max_residual'] = max(res, default=None)
        rep['x_new_norm'] = self.x_new_norm.cpu().tolist()
        return rep

    def done_suffix(self):
        r = self.report
        if 'T' not in r:
            return ''
        return (f" | thick_volume={r['T']:g}mm/{r['thin_dz']:g}mm {r['profile']} ({r['measured_slices']}/{len(r['slices'])} slices, "
                f"bw {r['bandwidth']})")


def interpolate(y, centres, n):
    """y fp32 [m,S,S], one image per measured thick slice centred at local index centres[j] (ascending) -> [n,S,S] in [-1,1] terms:
    piecewise linear along z through (c_j, y_j), constant beyond the first and the last centre.  Without a measured slice: -1."""
    m, S = y.shape[0], y.shape[-1]
    if m == 0:
        return torch.full((n, S, S), -1.0, device=y.device)
    c = np.asarray(centres, np.float64)
    z = np.arange(n, dtype=np.float64)
    hi = np.clip(np.searchsorted(c, z, side='right'), 1, max(m - 1, 1))
    lo = hi - 1
    hi = np.minimum(hi, m - 1)
    span = np.where(hi > lo, c[hi] - c[lo], 1.0)
    f = np.clip((z - c[lo]) / span, 0.0, 1.0)
    f = torch.from_numpy(f.astype(np.float32)).to(y.device)[:, None, None]
    ya = y.index_select(0, torch.from_numpy(lo).to(y.device))
    yb = y.index_select(0, torch.from_numpy(hi).to(y.device))
    return ((1.0 - f) * ya + f * yb).contiguous()


ThickInputs = collections.namedtuple('ThickInputs', 'values geometry grid_shape options')
ThickInputs.__doc__ = """Y checked against the prediction's grid: `values` [X,Y,m] float (as read, reoriented under --reorient), `geometry`:
slice_geometry's dict, `grid_shape` of the prediction, `options`: options_from's dict."""


def read_input(options, intake_options):
    """(host work only) Y as volume_prepare.read_for_evaluation reads it."""
    from .volume_prepare import read_for_evaluation
    return read_for_evaluation(options['volume'], intake_options)


def on_grid(first, y_file, options, intake_options, device, align=None):
    """Y (read_input's) against the grid the prediction will have (volume_prepare.evaluation_grid: `first` is the first input as
    read_for_evaluation reads it, or its RawVolume) -> ThickInputs.  Y is reoriented by its own affine under --reorient and never
    resampled: slice_geometry's ValueError when it does not share the grid's in-plane geometry."""
    shape, grid_world, values, y_world = own_grid_volume(first, y_file, intake_options, device, align)
    return ThickInputs(values, slice_geometry(shape, grid_world, values.shape, y_world), shape, options)


def own_grid_volume(first, y_file, intake_options, device, align=None):
    """What on_grid (and lowres_volume.on_grid) compares: -> (the prediction grid's shape and world affine, Y's values [X,Y,Z] float as
    read - reoriented under --reorient, never resampled - and Y's world affine)."""
    from . import volume_prepare as VP
    from . import volume_regrid as VR
    grid, Y, _, y_affine, _, _ = VP.evaluation_grid(first, y_file, None, intake_options, device, align)
    if hasattr(Y, 'header'):                                   # a RawVolume (as stored, or reoriented and about to be resampled)
        y_world, values = VR.world_affine_of(Y.affine, Y.header), Y.values_float64()
    elif intake_options.reorient is None and not hasattr(y_file, 'header'):
        y_world, values = VR.world_affine_of(y_file[1], y_file[2]), np.asarray(Y)
    else:
        y_world, values = np.asarray(y_affine, np.float64), np.asarray(Y)
    return tuple(int(v) for v in grid[0]), VR.world_affine_of(grid[1], grid[2]), values, y_world


def measure(inputs, ref, size, norm, device):
    """ThickInputs and the prediction's ref = (shape, affine, header, s0, s1) -> BandMeasurement for the thin slices s0..s1 on the S x S
    sampler grid."""
    from . import ops
    from .volume import normalise_volume
    shp, s0, s1 = tuple(int(v) for v in ref[0]), int(ref[3]), int(ref[4])
    if inputs.grid_shape != shp:
        raise ValueError(f'--known_thick_volume: checked against the grid {inputs.grid_shape}, the prediction is on {shp}')
    geo, opt, S = inputs.geometry, inputs.options, int(size)
    n, m_all = s1 - s0 + 1, geo['m']
    T = geo['thick_dz'] if opt['thickness'] is None else opt['thickness']
    width = T / geo['thin_dz']
    finite = np.isfinite(inputs.values)
    values = inputs.values if finite.all() else np.where(finite, inputs.values, 0.0)
    ynorm = np.ascontiguousarray(normalise_volume(values, norm), dtype=np.float32)
    whole = finite.reshape(-1, m_all).all(0)
    dropped = np.zeros(m_all, bool)
    for a, b in opt['drop']:
        dropped[a:b + 1] = True
    centres = geo['c0'] + geo['step'] * np.arange(m_all, dtype=np.float64)          # in thin-slice indices of the volume
    slices, keep = [], []
    for j in range(m_all):
        lo, hi = support(centres[j], width, opt['profile'])
        inside = lo >= s0 - 0.5 - 1e-9 and hi <= s1 + 0.5 + 1e-9
        measured = bool(inside and whole[j] and not dropped[j])
        slices.append(dict(centre=float(centres[j]), measured=measured))
        if measured:
            keep.append(j)
    local = centres[keep] - s0
    A = weight_rows(n, local, width, opt['profile'])
    planes = torch.from_numpy(np.ascontiguousarray(np.moveaxis(ynorm[:, :, keep], 2, 0))).to(device)[:, None]
    if keep and tuple(planes.shape[-2:]) != (S, S):
        planes = ops.resize_bilinear(planes.contiguous(), (S, S))
    y = planes[:, 0].contiguous() if keep else torch.zeros(0, S, S, device=device, dtype=torch.float32)
    meas = BandMeasurement(y, A, opt['resample'], None, opt, local)
    tab = meas.tables
    meas.report = dict(T=float(T), thin_dz=geo['thin_dz'], thick_dz=geo['thick_dz'], c0=geo['c0'], step=geo['step'], width=float(width),
                       profile=opt['profile'], image_size=S, slab=[s0, s1], thin_slices=n, thick_slices=m_all, measured_slices=len(keep),
                       cond=None if tab is None else tab.cond, bandwidth=None if tab is None else tab.bw, slices=slices,
                       drop=[list(r) for r in opt['drop']], resample=opt['resample'])
    return meas
