"""Sample a target given as a low-resolution volume of its own geometry (--known_lowres_volume; csrc/lowres.hip: mud_lowres_constrain,
mud_lowres_measure; GraphSampler.sample_lockstep).

--known_thick_volume (mudiff_hip.thick_volume) takes a scan that is coarser than the conditioning contrasts along z only.  The commonest
real case is coarser in all three axes: a fast 2 x 2 x 5 mm FLAIR or a scout next to 1 mm 3D T1 / T2.  Interpolating such a Y onto the
fine grid and passing it as --known_volume would impose interpolated voxels as if they were acquired; here every coarse voxel is what it
is, a weighted average of fine voxels, and the sampler re-imposes those averages after every reverse step:

    Y --volume_prepare.read_for_evaluation (--reorient applies)--> geometry of each axis against the prediction's grid
      --> A_z [m_z, n], A_y [m_y, S], A_x [m_x, S];  --norm--> y [m_z, m_y, m_x]
      --> sampler (every step: x <- x - A^T (A A^T)^-1 (A (x - s eta) - a y),  A = A_z (x) A_y (x) A_x) --> prediction

Geometry (voxel_geometry).  Y is 3D, and each of its axes is parallel to the same axis of the prediction grid within 1e-3 rad and points
the same way; shape, voxel size and origin are free.  Anything else is refused: registering Y, or resampling an oblique Y, is out of
scope.  From the two world affines coarse voxel j of an axis has its centre at fine index c0 + j * step, and it is E / (fine voxel size)
fine voxels wide (--lowres_volume_extent_mm EX EY EZ; default Y's own voxel size: contiguous voxels; larger: overlap; smaller: a gap).
The rows of an axis are thick_volume.weight_rows' (--lowres_volume_profile box | gauss, per axis as there), normalised to sum 1.

The sampler grid.  The sampler works on S x S images, the bilinear resize (align_corners=False) of an X x Y plane; volume axis 0 is the
image's row axis (volume.host_stacks).  Under that resize fine index c of an axis of X voxels sits at sampler pixel (c + 1/2) S / X - 1/2
and a width w becomes w S / X, so A_y and A_x are built over the S sampler pixels from the mapped centres and widths.  Y's own values
are never resampled.

Which coarse voxels are measured.  The measured set is a product J_z x J_y x J_x, so that A stays a Kronecker product.  A coarse index of
an axis is kept when its support lies wholly inside the sampled range of that axis: the slab s0..s1 along z, [-1/2, S - 1/2] in-plane.
A coarse z slice is also dropped when --lowres_volume_drop names it or when it holds a non-finite voxel inside J_y x J_x.  Pixels under
no measured coarse voxel are sampled freely.  A A^T = G_z (x) G_y (x) G_x, each factor banded, and the projection is one banded Cholesky
solve per axis (ops.lowres_constrain); ops.lowres_tables keeps ops.band_tables' limits per axis and refuses cond(G_z) cond(G_y) cond(G_x)
> 1e4.  The constraint couples the whole stack (`lockstep`), as thick_volume's does; its memory rule is that module's.

Y is normalised by --norm from its own non-zero voxels, as K is.  Two caveats.  For 'percentile' the map is affine between the 1st and
99th percentile, which commutes with the voxel average, but the clip beyond them does not: the average of clipped fine voxels is not the
clipped average, and the percentiles of a coarse volume are not those of the fine one (partial-volume voxels pull them inwards).  The
zscore clamp at 3 sigma does not commute either, so under --norm zscore y is only approximately A k for the k the model was trained on.
The effect of either on trained weights is unmeasured.

There is no final paste.  lowres_volume_<t>.json lists the three axes' c0 / step / width, the extents, the profile, cond and bandwidth
per axis and their product, and per coarse slice whether it was measured and |A x - y| / |y| of the sampler's result (the largest over
an ensemble's samples; ops.lowres_measure).  --lowres_volume_baseline also writes and scores lowres_volume_interp_<t>.nii.gz: Y resampled
onto the prediction's grid (mudiff_hip.volume_regrid, --regrid_interp), what one has without the model.  A cohort takes each subject's Y
from the manifest's `known` column under `--known_lowres_volume manifest`.

Limits.  box and gauss are voxel-footprint models of a magnitude image stored at a coarse voxel size; they are not the sinc point spread
of a truncated k-space (--known_kspace with a centre mask is the tool for that, on an equal grid).  Out of scope: an oblique or
unregistered Y; multi-coil data; a profile per slice; the uncaptured (use_graph=False) path; the 2D driver.
"""
from __future__ import annotations

import collections
import math

import numpy as np
import torch

from .constraints import Constraint, level_tables, need_keyed_seed, relative_residual
from .thick_volume import MANIFEST, PROFILES, TOL_RAD, own_grid_volume, support, weight_rows

_OTHERS = ('known_volume', 'known_kspace', 'known_thick', 'known_multislice', 'known_mask', 'known_drop_slices', 'known_thick_volume')
AXES = ('x', 'y', 'z')                                   # the volume's axes: x = image rows, y = image columns, z = slices


def add_flags(p):
    p = p.later() if hasattr(p, 'later') else p          # volume.VolumeParser: the lists of the parsers before this one are pinned
    p.add_argument('--known_lowres_volume', type=str, default=None, metavar='Y',
                   help='the target contrast as a NIfTI that is coarser than the prediction in all three axes, with a voxel size and origin '
                        'of its own (axes parallel to the prediction\'s): every coarse voxel is a weighted average of fine voxels and the '
                        'sampler re-imposes those averages after every reverse step - super-resolution in all three axes '
                        f"(mudiff_hip.lowres_volume, DESIGN.md section 5.31); '{MANIFEST}' in a cohort: the manifest's `known` column")
    p.add_argument('--lowres_volume_extent_mm', type=float, nargs=3, default=None, metavar=('EX', 'EY', 'EZ'),
                   help='with --known_lowres_volume: the extent of a coarse voxel in mm per axis (default: Y\'s voxel size = contiguous '
                        'voxels; larger: overlap; smaller: a gap)')
    p.add_argument('--lowres_volume_profile', type=str, default=None, choices=list(PROFILES),
                   help='with --known_lowres_volume: the voxel profile along every axis, box (the default) or gauss (FWHM = the extent, cut at '
                        '+- the extent)')
    p.add_argument('--lowres_volume_drop', type=str, nargs='+', default=None, metavar='A:B',
                   help='with --known_lowres_volume: coarse slices A..B along z (inclusive, indices of Y) that were not acquired')
    p.add_argument('--lowres_volume_baseline', action='store_true',
                   help='with --known_lowres_volume: also write lowres_volume_interp_<t>.nii.gz, Y resampled onto the prediction\'s grid '
                        '(--regrid_interp; what one would have without the model; scored too under --gt_volume)')


def _drop_ranges(values):
    out = []
    for v in values or ():
        parts = str(v).split(':')
        try:
            a, b = (int(x) for x in parts) if len(parts) == 2 else (None, None)
        except ValueError:
            a = b = None
        if a is None or a < 0 or b < a:
            raise ValueError(f'--lowres_volume_drop takes ranges A:B of coarse slices with 0 <= A <= B, got {v!r}')
        out.append((a, b))
    return out


def options_from(args):
    """A namespace's --known_lowres_volume / --lowres_volume_* flags (any may be missing) -> None without --known_lowres_volume, else
    dict(volume, extent (3 or None), profile, drop [(a, b)], baseline, resample).  ValueError, naming the flag, for a dependent flag
    without --known_lowres_volume, for --known_lowres_volume together with any other known-target flag, `manifest` outside a cohort, a bad
    value and a seed outside [0, 2^64)."""
    volume = getattr(args, 'known_lowres_volume', None)
    extent, profile, drop = (getattr(args, f, None) for f in ('lowres_volume_extent_mm', 'lowres_volume_profile', 'lowres_volume_drop'))
    baseline = bool(getattr(args, 'lowres_volume_baseline', False))
    if volume is None:
        for flag, given in (('--lowres_volume_extent_mm', extent is not None), ('--lowres_volume_profile', profile is not None),
                            ('--lowres_volume_drop', drop is not None), ('--lowres_volume_baseline', baseline)):
            if given:
                raise ValueError(f'{flag} needs --known_lowres_volume')
        return None
    for other in _OTHERS:
        if getattr(args, other, None) is not None:
            raise ValueError(f'--known_lowres_volume cannot be combined with --{other}: Y is the measurement itself, on its own grid in all '
                             'three axes (give one known-target mode)')
    cohort = getattr(args, 'manifest', None) is not None or getattr(args, 'brats_root', None) is not None
    if volume == MANIFEST and not cohort:
        raise ValueError(f"--known_lowres_volume {MANIFEST} needs a cohort (--manifest): it takes each subject's file from the `known` column")
    if extent is not None:
        extent = [float(v) for v in extent]
        if len(extent) != 3 or not all(math.isfinite(v) and v > 0 for v in extent):
            raise ValueError(f'--lowres_volume_extent_mm takes three positive numbers of millimetres, got {extent}')
    profile = 'box' if profile is None else profile
    if profile not in PROFILES:
        raise ValueError(f'--lowres_volume_profile must be one of {PROFILES}, got {profile!r}')
    resample = getattr(args, 'known_resample', 1)
    resample = 1 if resample is None else resample
    if int(resample) != resample or resample < 1:
        raise ValueError(f'--known_resample must be an integer >= 1, got {resample}')
    need_keyed_seed(args, '--known_lowres_volume')
    return dict(volume=volume, extent=extent, profile=profile, drop=_drop_ranges(drop), baseline=baseline, resample=int(resample))


# ---------------------------------------------------------------------------------------------------
# geometry and weights: numpy fp64, functions of the flags and the two affines alone
# ---------------------------------------------------------------------------------------------------
def voxel_geometry(grid_shape, grid_affine, y_shape, y_affine):
    """The prediction grid and Y as (shape, world affine) -> dict(c0, step: coarse voxel j of axis k is centred at fine index c0[k] +
    j * step[k]; fine_mm, coarse_mm: the voxel sizes; m: Y's shape), each a list over the volume's three axes.  ValueError, naming
    registration and oblique resampling as out of scope, unless every axis of Y is parallel to the same axis of the grid and points the
    same way (see the module's header)."""
    a, b = np.asarray(grid_affine, np.float64), np.asarray(y_affine, np.float64)
    out_of_scope = ' (registering Y, or resampling an oblique Y, is out of scope: bring its axes onto the inputs\' first)'
    if len(y_shape) != 3 or len(grid_shape) != 3:
        raise ValueError(f'--known_lowres_volume: expected a 3D volume, got shape {tuple(y_shape)}')
    fine = [float(np.linalg.norm(a[:3, k])) for k in range(3)]
    coarse = [float(np.linalg.norm(b[:3, k])) for k in range(3)]
    if not all(v > 0 and math.isfinite(v) for v in fine + coarse):
        raise ValueError('--known_lowres_volume: an affine has an axis of length 0')
    for k in range(3):
        u, v = a[:3, k] / fine[k], b[:3, k] / coarse[k]
        cosine, sine = float(np.dot(u, v)), float(np.linalg.norm(np.cross(u, v)))
        if cosine <= 0 or math.atan2(sine, cosine) > TOL_RAD:
            raise ValueError(f'--known_lowres_volume: its {AXES[k]} axis is not parallel to the prediction grid\'s (angle '
                             f'{math.atan2(sine, cosine):.4g} rad)' + out_of_scope)
    to_fine = np.linalg.inv(a[:3, :3])                   # world displacement -> fine voxel index units
    c0 = to_fine @ (b[:3, 3] - a[:3, 3])
    step = np.diag(to_fine @ b[:3, :3])
    return dict(c0=[float(v) for v in c0], step=[float(v) for v in step], fine_mm=fine, coarse_mm=coarse, m=[int(v) for v in y_shape])


def to_sampler(c, width, step, size, extent):
    """Centres, a width and a step in fine-voxel index units of an axis of `extent` voxels -> the same in pixels of the sampler's axis
    of `size`, the bilinear resize with align_corners=False: c -> (c + 1/2) size / extent - 1/2, lengths scale by size / extent."""
    k = float(size) / float(extent)
    return (np.asarray(c, np.float64) + 0.5) * k - 0.5, float(width) * k, float(step) * k


def kept(centres, width, profile, lo, hi):
    """bool [len(centres)]: the coarse voxels whose support lies wholly inside [lo, hi]."""
    out = np.zeros(len(centres), bool)
    for j, c in enumerate(centres):
        a, b = support(float(c), width, profile)
        out[j] = a >= lo - 1e-9 and b <= hi + 1e-9
    return out


# ---------------------------------------------------------------------------------------------------
# the measurement of one prediction
# ---------------------------------------------------------------------------------------------------
class LowresMeasurement(Constraint):
    """What the samplers take for one prediction of n thin slices on S x S: `y` fp32 [m_z, m_y, m_x] on the device, the measured coarse
    voxels; `A` = (A_z [m_z, n], A_y [m_y, S], A_x [m_x, S]) fp64; `tables`: ops.lowres_tables(*A) (None when nothing was measured: the
    prediction is then sampled freely, still in lockstep); `report`: lowres_volume_<t>.json without the residuals; `resample`:
    --known_resample; `interp`: a callable -> the baseline volume (host [X,Y,Z]) or None."""
    lockstep = True
    tag, baseline_through_plane = 'lowres_volume', True

    def __init__(self, y, A, resample=1, report=None, options=None, interp=None):
        from . import ops
        self.A = tuple(np.asarray(M, np.float64) for M in A)
        self.y, self.resample = y, int(resample)
        self.shape = tuple(int(M.shape[0]) for M in self.A)
        self.n, self.H, self.W = (int(M.shape[1]) for M in self.A)
        if tuple(y.shape) != self.shape:
            raise ValueError(f'LowresMeasurement: y is {tuple(y.shape)}, the matrices name {self.shape} coarse voxels')
        self.measured = all(self.shape)
        self.tables = ops.lowres_tables(*self.A) if self.measured else None
        self.report = dict(report or {})
        self.options = dict(options or {})
        self._interp = interp
        dev = y.device
        mz = self.shape[0] if self.measured else 0
        self.y_norm = torch.linalg.vector_norm(y.reshape(mz, -1), dim=1) if mz else torch.zeros(0, device=dev)
        self.residual = torch.zeros(mz, device=dev, dtype=torch.float32)
        self.x_new_norm = torch.zeros(self.n, device=dev, dtype=torch.float32)
        self._work = None

    @property
    def m(self):
        """The workspace per sample in rows of H x W floats (ensemble.lockstep_bytes)."""
        if not self.measured:
            return 0
        mz, my, mx = self.shape
        return -(-(self.n + mz) * my * mx // (self.H * self.W))

    def chunk_end(self, s0, s1):
        return self.n                                # the whole stack is one chunk

    def check_volume(self, sampler, rows):
        from . import ops
        if rows % self.n:
            raise ValueError(f'GraphSampler.sample_lockstep: {rows} rows are not whole stacks of {self.n} slices')
        if (sampler.H, sampler.W) != (self.H, self.W):
            raise ValueError(f'GraphSampler.sample_lockstep: the low-resolution volume was measured for {self.H} x {self.W} images, the '
                             f'sampler makes {sampler.H} x {sampler.W}')
        if self.y.dtype != torch.float32:
            raise ValueError(f'GraphSampler.sample_lockstep: low-resolution volume y must be fp32, got {self.y.dtype}')
        self._y = self.y.to(sampler.x.device).contiguous()
        if self.measured:
            need = ops.lowres_ws_floats(rows // self.n, self.tables)
            if self._work is None or self._work.numel() != need or self._work.device != sampler.x.device:
                self._work = torch.empty(need, device=sampler.x.device, dtype=torch.float32)

    def apply_volume(self, sampler, x_new, x, keys_dev, seed, step, clean):
        from . import ops
        if not self.measured:
            x.copy_(x_new)
            return
        ops.lowres_constrain_into(x, x_new, self._y, self.tables, self._work, keys_dev, seed, step, ops.KIND_LOWRES, sampler.t_rows, 0,
                                  *level_tables(sampler), clean=clean)

    def record_volume(self, x, x_new=None):
        """x [sets * n,1,S,S]: what the sampler returned (in [-1,1], before any map): keeps, per coarse slice, the largest
        |A x - y| / |y| over the sets, and per thin slice the largest |x_new| of what the last constraint was given."""
        from . import ops
        if not self.measured:
            return
        sets = x.shape[0] // self.n
        xs = x.reshape(sets, self.n, self.H, self.W)
        d = ops.lowres_measure(xs.contiguous(), self.tables) - self.y[None]
        self.residual = torch.maximum(self.residual, relative_residual(d.reshape(sets, self.shape[0], -1), self.y_norm).amax(0))
        xn = xs if x_new is None else x_new.reshape(sets, self.n, self.H, self.W)
        self.x_new_norm = torch.maximum(self.x_new_norm, torch.linalg.vector_norm(xn.reshape(sets, self.n, -1), dim=2).amax(0))

    def baseline(self):
        if not self.options.get('baseline') or self._interp is None:
            return None
        return 'lowres_volume_interp', self._interp()

    def finish(self):
        """The report with the residuals put in (None for a coarse slice that was not measured)."""
        res, yn = self.residual.cpu().tolist(), self.y_norm.cpu().tolist()
        rep, g = dict(self.report), 0
        rep['slices'] = [dict(s) for s in rep.get('slices', [dict(measured=True) for _ in res])]
        for s in rep['slices']:
            s['residual'], s['y_norm'] = (res[g], yn[g]) if s['measured'] and g < len(res) else (None, None)
            g += 1 if s['measured'] else 0
        rep['max_residual'] = max(res, default=None)
        rep['x_new_norm'] = self.x_new_norm.cpu().tolist()
        return rep

    def done_suffix(self):
        r = self.report
        if 'extent_mm' not in r:
            return ''
        mm = lambda v: 'x'.join(f'{float(e):g}' for e in v)      # noqa: E731
        bw = '/'.join('-' if r['axes'][k]['bandwidth'] is None else str(r['axes'][k]['bandwidth']) for k in ('z', 'y', 'x'))
        return (f" | lowres_volume={mm(r['extent_mm'])}mm on {mm(r['fine_mm'])}mm {r['profile']} ({r['measured_slices']}/{len(r['slices'])} slices, "
                f"bw {bw})")


LowresInputs = collections.namedtuple('LowresInputs', 'values geometry grid_shape options y_world grid_world interp')
LowresInputs.__doc__ = """Y checked against the prediction's grid: `values` [m_x,m_y,m_z] float (as read, reoriented under --reorient),
`geometry`: voxel_geometry's dict, `grid_shape` of the prediction, `options`: options_from's dict, the two world affines and
--regrid_interp (for the baseline)."""


def read_input(options, intake_options):
    """(host work only) Y as volume_prepare.read_for_evaluation reads it."""
    from .volume_prepare import read_for_evaluation
    return read_for_evaluation(options['volume'], intake_options)


def on_grid(first, y_file, options, intake_options, device, align=None):
    """Y (read_input's) against the grid the prediction will have (volume_prepare.evaluation_grid: `first` is the first input as
    read_for_evaluation reads it, or its RawVolume) -> LowresInputs.  Y is reoriented by its own affine under --reorient and never
    resampled: voxel_geometry's ValueError when an axis of it is not parallel to the grid's."""
    shape, grid_world, values, y_world = own_grid_volume(first, y_file, intake_options, device, align)
    geometry = voxel_geometry(shape, grid_world, values.shape, y_world)
    return LowresInputs(values, geometry, shape, options, np.asarray(y_world, np.float64), np.asarray(grid_world, np.float64),
                        getattr(intake_options, 'interp', 'linear'))


def interpolated(inputs, device):
    """Y resampled onto the prediction's grid (volume_regrid.regrid, inputs.interp) -> host fp32 [X,Y,Z], in Y's own units."""
    from . import volume_regrid as VR
    flat = torch.from_numpy(np.ascontiguousarray(np.asarray(inputs.values, np.float32).reshape(-1, order='F'))).to(device)
    M = VR.grid_matrix(inputs.y_world, inputs.grid_world)
    out = VR.regrid(flat, 16, inputs.values.shape, 1.0, 0.0, M, inputs.grid_shape, inputs.interp or 'linear')      # 16: NIFTI_F4
    return np.ascontiguousarray(out.cpu().numpy().transpose(2, 1, 0))


def measure(inputs, ref, size, norm, device):
    """LowresInputs and the prediction's ref = (shape, affine, header, s0, s1) -> LowresMeasurement for the thin slices s0..s1 on the
    S x S sampler grid."""
    from .volume import normalise_volume
    shp, s0, s1 = tuple(int(v) for v in ref[0]), int(ref[3]), int(ref[4])
    if inputs.grid_shape != shp:
        raise ValueError(f'--known_lowres_volume: checked against the grid {inputs.grid_shape}, the prediction is on {shp}')
    geo, opt, S = inputs.geometry, inputs.options, int(size)
    n, profile = s1 - s0 + 1, opt['profile']
    extent = list(geo['coarse_mm']) if opt['extent'] is None else list(opt['extent'])
    fine_c, fine_w = [], []                              # per volume axis, in fine-voxel index units of the volume
    for k in range(3):
        fine_c.append(geo['c0'][k] + geo['step'][k] * np.arange(geo['m'][k], dtype=np.float64))
        fine_w.append(extent[k] / geo['fine_mm'][k])
    # z: local thin-slice indices of the slab; in-plane: sampler pixels
    cz, wz, stz = fine_c[2] - s0, fine_w[2], geo['step'][2]
    (cx, wx, stx), (cy, wy, sty) = (to_sampler(fine_c[k], fine_w[k], geo['step'][k], S, shp[k]) for k in (0, 1))
    keep_x, keep_y = kept(cx, wx, profile, -0.5, S - 0.5), kept(cy, wy, profile, -0.5, S - 0.5)
    inside_z = kept(cz, wz, profile, -0.5, n - 0.5)
    finite = np.isfinite(inputs.values)
    values = inputs.values if finite.all() else np.where(finite, inputs.values, 0.0)
    whole = finite[keep_x][:, keep_y].reshape(-1, geo['m'][2]).all(0) if keep_x.any() and keep_y.any() else np.ones(geo['m'][2], bool)
    dropped = np.zeros(geo['m'][2], bool)
    for a, b in opt['drop']:
        dropped[a:b + 1] = True
    keep_z = inside_z & whole & ~dropped
    slices = [dict(centre=float(fine_c[2][j]), measured=bool(keep_z[j])) for j in range(geo['m'][2])]
    if not (keep_x.any() and keep_y.any() and keep_z.any()):
        keep_x, keep_y, keep_z = (np.zeros_like(v) for v in (keep_x, keep_y, keep_z))      # nothing is measured: sampled freely
        slices = [dict(s, measured=False) for s in slices]
    A = (weight_rows(n, cz[keep_z], wz, profile), weight_rows(S, cx[keep_x], wx, profile), weight_rows(S, cy[keep_y], wy, profile))
    ynorm = np.asarray(normalise_volume(values, norm), dtype=np.float32)
    y = np.ascontiguousarray(np.moveaxis(ynorm[keep_x][:, keep_y][:, :, keep_z], 2, 0))      # [m_z, m_x (image rows), m_y (image columns)]
    meas = LowresMeasurement(torch.from_numpy(y).to(device), A, opt['resample'], None, opt, lambda: interpolated(inputs, device))
    tabs = meas.tables
    axis = lambda name, k, c0, step, width, keep, tab: dict(                               # noqa: E731
        volume_axis=AXES[k], c0=float(c0), step=float(step), width=float(width), coarse=int(geo['m'][k]), measured=int(keep.sum()),
        first=int(np.flatnonzero(keep)[0]) if keep.any() else None, cond=None if tab is None else tab.cond,
        bandwidth=None if tab is None else tab.bw)
    meas.report = dict(
        extent_mm=[float(v) for v in extent], fine_mm=list(geo['fine_mm']), coarse_mm=list(geo['coarse_mm']), profile=profile, image_size=S,
        slab=[s0, s1], thin_slices=n, geometry=dict(c0=list(geo['c0']), step=list(geo['step'])),
        axes=dict(z=axis('z', 2, cz[0] if len(cz) else 0.0, stz, wz, keep_z, None if tabs is None else tabs.z),
                  y=axis('y', 0, cx[0] if len(cx) else 0.0, stx, wx, keep_x, None if tabs is None else tabs.y),
                  x=axis('x', 1, cy[0] if len(cy) else 0.0, sty, wy, keep_y, None if tabs is None else tabs.x)),
        cond=None if tabs is None else tabs.cond, measured_slices=int(keep_z.sum()), slices=slices, drop=[list(r) for r in opt['drop']],
        resample=opt['resample'])
    return meas
