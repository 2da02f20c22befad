"""Inputs stored in another orientation than the training data (--reorient; csrc/volume_reorient.hip: mud_volume_reorient; DESIGN.md
section 5.20).

The volume pipeline takes the first input's storage grid as it is: the slab runs along the third storage axis and the generators see
each plane with the first storage axis as rows.  The checkpoints were trained on BraTS files read without reorientation (the
reference's tools/pre_process.py: get_fdata() and vol[:, :, z]), and BraTS stores its voxels Left-Posterior-Superior.  A volume stored
otherwise - RAS by another converter, or a sagittal or coronal acquisition - would reach the generators mirrored or as non-axial planes.
With --reorient every input is first brought to the target orientation (default 'LPS'; --reorient_to for a checkpoint trained
otherwise) by a permutation and flips of its storage axes, and its affine is changed to match, so that every voxel keeps its world
position exactly:

    world affine --axcodes--> 'RAS' --plan(shape, affine, 'LPS')--> perm, flip, new shape, new affine
    stored voxels --upload--> mud_volume_reorient(perm, flip) --> the same stored values (datatype and scaling kept) in the new order

No interpolation: this is exact, and the numpy restatement (tests/volume_reorient_ref.py) is a transpose and slices.  A permutation
cannot make tilted slices axial: an oblique acquisition keeps its tilt (obliquity_deg reports it, the pipeline warns above
OBLIQUE_WARN_DEG); de-obliquing by resampling is out of scope here.

Definitions (numpy only, no device): axcodes, obliquity_deg, plan / ReorientPlan, apply_host, reoriented_header, reorient_suffix,
write_reports.  On the device: reorient -> ReorientedVolume.
"""
from __future__ import annotations

import itertools
import struct

import numpy as np

from .volume_intake import DEVICE_DTYPES, RawVolume, upload, write_report_json

POSITIVE, NEGATIVE = 'RAS', 'LPI'                        # NIfTI world is RAS+: the letter of world axis w by the sign along it
TARGETS = tuple(''.join(POSITIVE[w] if s else NEGATIVE[w] for w, s in zip(order, signs))
                for order in itertools.permutations(range(3)) for signs in itertools.product((True, False), repeat=3))      # the 48 codes
DEFAULT_TARGET = 'LPS'                                   # BraTS's storage order, which the reference reads unreoriented
OBLIQUE_WARN_DEG = 10.0                                  # an untuned default, not a measured bar: above it the pipeline prints a warning


def check_target(code):
    """-> the code in upper case; ValueError unless it holds one letter of each of R/L, A/P, S/I."""
    c = str(code).upper()
    if c not in TARGETS:
        raise ValueError(f"--reorient_to must hold one letter of each of R/L, A/P, S/I (such as 'LPS' or 'RAS'), got {code!r}")
    return c


def _assignment(world_affine):
    """-> (world axis of every voxel axis, sign of every voxel axis (+1 / -1), |cos| of every voxel axis to its world axis, the 3 x 3
    matrix of cosines [world, voxel])."""
    a = np.asarray(world_affine, np.float64)
    if a.shape not in ((3, 3), (4, 4)) or not np.isfinite(a).all():
        raise ValueError(f'affine: need a finite 3 x 3 or 4 x 4 affine, got {a.tolist() if a.size <= 16 else a.shape}')
    lin = a[:3, :3]
    norms = np.sqrt((lin * lin).sum(0))
    scale = np.abs(lin).max()
    if scale == 0 or (norms == 0).any() or abs(np.linalg.det(lin / scale)) < 1e-12:      # (volume_regrid.grid_matrix's test)
        raise ValueError('the affine is singular')
    cos = lin / norms
    left = np.abs(cos)
    world, sign = [0, 0, 0], [1, 1, 1]
    for _ in range(3):
        w, v = divmod(int(np.argmax(left)), 3)          # the largest entry; the first in (world, voxel) order among equals
        world[v], sign[v] = w, -1 if cos[w, v] < 0 else 1
        left[w, :] = -1.0
        left[:, v] = -1.0
    return tuple(world), tuple(sign), cos


def axcodes(world_affine):
    """The orientation code of a voxel -> world matrix (the 3 x 3 part of volume_regrid.world_affine_of(...), or the 4 x 4 itself), one
    letter per voxel axis: the world direction it runs towards, 'R'/'L', 'A'/'P', 'S'/'I'.  The columns are normalised to unit length and
    every voxel axis is assigned a world axis greedily on |cos|: the largest entry, its row and column struck, and again; ties go to the
    lowest (world, voxel) index.  ValueError for a singular or non-finite affine."""
    world, sign, _ = _assignment(world_affine)
    return ''.join((POSITIVE if s > 0 else NEGATIVE)[w] for w, s in zip(world, sign))


def obliquity_deg(world_affine):
    """The largest angle, in degrees, between a voxel axis and the world axis axcodes assigned it to (0 for an axis-aligned grid)."""
    world, _, cos = _assignment(world_affine)
    worst = 0.0
    for v, w in enumerate(world):
        off = float(np.sqrt(sum(cos[u, v] ** 2 for u in range(3) if u != w)))
        worst = max(worst, float(np.degrees(np.arctan2(off, abs(float(cos[w, v]))))))
    return worst


class ReorientPlan:
    """dst[i0, i1, i2] = src[j] with j[perm[o]] = S[perm[o]] - 1 - i_o if flip[o] else i_o.  `shape`: the destination's; `affine` =
    source affine @ `matrix`, where `matrix` is the 4 x 4 integer matrix that takes a destination index to its source index, so that every
    voxel keeps its world position; `identity`: nothing moves; `source` / `target`: the orientation codes; `src_shape`, `src_affine`: what
    the plan was made for."""

    def __init__(self, perm, flip, src_shape, src_affine, source, target, affine=None):
        self.perm, self.flip = tuple(int(p) for p in perm), tuple(bool(f) for f in flip)
        self.src_shape = tuple(int(v) for v in src_shape)
        self.src_affine = np.array(src_affine, np.float64)
        self.source, self.target = source, target
        self.shape = tuple(self.src_shape[p] for p in self.perm)
        m = np.zeros((4, 4), np.float64)
        for o, (p, f) in enumerate(zip(self.perm, self.flip)):
            m[p, o] = -1.0 if f else 1.0
            m[p, 3] = self.src_shape[p] - 1 if f else 0.0
        m[3, 3] = 1.0
        self.matrix = m
        self.affine = self.src_affine @ m if affine is None else np.array(affine, np.float64)
        self.identity = self.perm == (0, 1, 2) and not any(self.flip)

    def inverse(self):
        """The plan that undoes this one: applied to this plan's result it gives the source back, with the source's own affine."""
        perm, flip = [0, 0, 0], [False, False, False]
        for o, (p, f) in enumerate(zip(self.perm, self.flip)):
            perm[p], flip[p] = o, f
        return ReorientPlan(perm, flip, self.shape, self.affine, self.target, self.source, affine=self.src_affine)

    def entry(self):
        """What reorient_<t>.json holds for one input."""
        return {'from': self.source, 'to': self.target, 'perm': list(self.perm), 'flip': [bool(f) for f in self.flip],
                'shape_from': list(self.src_shape), 'shape_to': list(self.shape), 'obliquity_deg': obliquity_deg(self.src_affine),
                'moved': not self.identity}


def plan(shape, world_affine, target=DEFAULT_TARGET):
    """The permutation and flips that bring a volume of `shape` whose voxel -> world matrix is `world_affine` (4 x 4) to the orientation
    `target` (any of the 48 codes).  ValueError for a volume that is not 3D, a bad code, a singular or non-finite affine."""
    target = check_target(target)
    if len(shape) != 3:
        raise ValueError(f'reorient: expected a 3D volume, got shape {tuple(shape)}')
    a = np.asarray(world_affine, np.float64)
    if a.shape != (4, 4):
        raise ValueError(f'reorient: need a 4 x 4 affine, got {a.shape}')
    world, sign, _ = _assignment(a)
    perm, flip = [], []
    for letter in target:
        w = (POSITIVE.index(letter) if letter in POSITIVE else NEGATIVE.index(letter))
        v = world.index(w)                                # the source voxel axis that runs along this world axis
        perm.append(v)
        flip.append((sign[v] > 0) != (letter in POSITIVE))
    return ReorientPlan(perm, flip, shape, a, axcodes(a), target)


def apply_host(vol, p):
    """A host [X, Y, Z] array permuted and flipped by a plan: a numpy view (transpose + slices), no copy."""
    out = np.asarray(vol).transpose(p.perm)
    return out[tuple(slice(None, None, -1) if f else slice(None) for f in p.flip)]


def reoriented_header(header, p):
    """The header that describes a volume after plan `p`.  The built-in NiftiHeader: a copy of the 348 bytes with dim[1..3] and
    pixdim[1..3] permuted, the sform rows set to p.affine, sform_code = max(old, 1) and qform_code = 0 (no stale quaternion survives);
    everything else, datatype and scl_slope / scl_inter included, is kept.  A nibabel header goes through its own setters; None stays None."""
    from .volume import NiftiHeader
    if header is None:
        return None
    if isinstance(header, NiftiHeader):
        e = header.endian
        raw = bytearray(header.raw)
        dim, pix = list(header._get('8h', 40)), list(header._get('8f', 76))
        dim[1:4] = [int(v) for v in p.shape]
        pix[1:4] = [pix[1 + q] for q in p.perm]
        struct.pack_into(e + '8h', raw, 40, *dim)
        struct.pack_into(e + '8f', raw, 76, *pix)
        struct.pack_into(e + 'h', raw, 252, 0)
        struct.pack_into(e + 'h', raw, 254, max(int(header._get('h', 254)[0]), 1))
        for r in range(3):
            struct.pack_into(e + '4f', raw, 280 + 16 * r, *[float(v) for v in p.affine[r]])
        return NiftiHeader(bytes(raw), e)
    h = header.copy()                                     # nibabel
    zooms = list(h.get_zooms())
    zooms[:3] = [zooms[q] for q in p.perm]
    h.set_data_shape(tuple(p.shape) + tuple(h.get_data_shape()[3:]))
    h.set_zooms(zooms)
    h.set_sform(p.affine, code=max(int(h['sform_code']), 1))
    h.set_qform(None, code=0)
    return h


class ReorientedVolume(RawVolume):
    """A RawVolume whose stored voxels live on the device in their new order (`dev`: flat, the representation volume_intake.upload hands
    on as it is: uint16 as int16 bits), with the datatype code, endianness and scaling of the volume it was made from and the shape, affine
    and header of the plan.  `data` (the flat host array in the stored dtype) is downloaded on first use and kept."""

    def __init__(self, dev, raw, p):
        self._host = None
        super().__init__(None, raw.code, raw.endian, raw.slope, raw.inter, p.shape, p.affine, reoriented_header(raw.header, p))
        self.dev = dev

    @property
    def data(self):
        if self._host is None:
            host = self.dev.reshape(-1).cpu().numpy()
            kind = DEVICE_DTYPES.get(self.code)
            self._host = host if kind is None else host.view(np.dtype('<' + kind))
        return self._host

    @data.setter
    def data(self, value):
        self._host = value


def reorient(raw, device, target=DEFAULT_TARGET):
    """A RawVolume -> (the same volume stored in the orientation `target`, its report entry).  A volume that is stored that way already
    is returned itself and nothing is launched; otherwise the stored voxels are uploaded as they are and permuted on the device
    (ops.volume_reorient): a ReorientedVolume.  The volume's place in the world is volume_regrid.world_affine_of(raw.affine, raw.header)."""
    from .volume_regrid import world_affine_of
    p = plan(raw.shape, world_affine_of(raw.affine, raw.header), target)
    if p.identity:
        return raw, p.entry()
    from . import ops
    dev = upload(raw, device)
    return ReorientedVolume(ops.volume_reorient(dev, dev.element_size(), raw.shape, p), raw, p), p.entry()


# ---------------------------------------------------------------------------------------------------
# the pipeline's side
# ---------------------------------------------------------------------------------------------------
def add_flags(p):
    p.add_argument('--reorient', action='store_true',
                   help='bring every input (and --gt_volume / --eval_mask), each by its own affine, to the storage orientation the '
                        'checkpoints were trained on before anything else sees it: a permutation and flips of the storage axes on the GPU '
                        '(mudiff_hip.volume_reorient), exact, datatype and scaling kept, the affine changed to match.  The slab is then '
                        'cut along the third axis of that orientation and everything is written on the reoriented grid; '
                        'reorient_<t>.json next to the prediction holds what was done.  A permutation cannot make tilted slices axial: an '
                        'input whose axes are tilted by more than 10 degrees (an untuned default, not a measured bar) gets a warning, and '
                        'de-obliquing by resampling is not done')
    p.add_argument('--reorient_to', type=str, default=None, metavar='CODE',
                   help="the target orientation of --reorient, one letter of each of R/L, A/P, S/I: the direction every storage axis runs "
                        "towards.  'LPS' is how BraTS stores its volumes, which the reference reads without reorienting; a checkpoint "
                        'trained on data stored otherwise needs its own code.  Default: LPS, or under --conform what --conform_to says')
    p.add_argument('--reorient_back', action='store_true',
                   help="with --reorient: write predicted_<t>.nii.gz (and predicted_<t>_std.nii.gz) in the first input's own storage order, "
                        'with its original affine and header (scored first, on the reoriented grid)')


def options_from(args):
    """A namespace's --reorient flags (any may be missing) -> IntakeOptions' `reorient`: dict(target=the code of --reorient_to, LPS
    when there is none), or None without --reorient.  ValueError for a bad code and for --reorient_back on its own."""
    target = check_target(getattr(args, 'reorient_to', None) or DEFAULT_TARGET)
    on = bool(getattr(args, 'reorient', False))
    if getattr(args, 'reorient_back', False) and not on:
        raise ValueError('--reorient_back needs --reorient')
    return dict(reorient=dict(target=target) if on else None)


def reference_of(raw, target=DEFAULT_TARGET):
    """(shape, affine, header) of a volume once reoriented, and the plan: the geometry a prediction from it has.  No voxel is moved."""
    from .volume_regrid import world_affine_of
    p = plan(raw.shape, world_affine_of(raw.affine, raw.header), target)
    return (p.shape, p.affine, reoriented_header(raw.header, p)), p


def eval_inputs(gt_raw, label_raw, device, target, as_arrays):
    """--gt_volume / --eval_mask under --reorient: each RawVolume reoriented by its own affine to `target`.  -> (gt, label or None, the
    ground truth's new affine); with `as_arrays` the two are [X, Y, Z] float64 arrays as volume.read_nifti returns them (the path without
    --regrid), else RawVolumes (--regrid resamples them next)."""
    gt = reorient(gt_raw, device, target)[0]
    label = None if label_raw is None else reorient(label_raw, device, target)[0]
    affine = gt.affine
    if as_arrays:
        gt, label = gt.values_float64(), None if label is None else label.values_float64()
    return gt, label, affine


def write_back(write, first_raw, target=DEFAULT_TARGET):
    """--reorient_back: wraps a `write(path, vol, affine, header)` callable (volume.write_nifti, or a cohort's deferred writer) so that
    the volume it is given on the reoriented grid is written in the first input's own storage order with that input's original affine and
    header.  The volume is a host array about to be serialised at that point: the inverse permutation is a numpy transpose / flip view,
    applied once, and write_nifti's tobytes(order='F') does the only copy; a device launch would buy nothing there."""
    from .volume_regrid import world_affine_of
    back = plan(first_raw.shape, world_affine_of(first_raw.affine, first_raw.header), target).inverse()

    def wrapped(path, vol, affine, header):
        return write(path, apply_host(vol, back), first_raw.affine, first_raw.header)
    return wrapped


def warn_oblique(name, entry):
    if entry['obliquity_deg'] > OBLIQUE_WARN_DEG:
        print(f"[reorient] warning: {name}: the voxel axes are tilted by {entry['obliquity_deg']:.1f} degrees against the world axes; a "
              'permutation cannot make tilted slices axial (de-obliquing by resampling is not done here)')


def reorient_suffix(entries):
    """What a [done] line gains under --reorient (nothing otherwise): ` | reorient=T1:RAS>LPS,T2:same,...`."""
    if not entries:
        return ''
    return ' | reorient=' + ','.join(f"{name}:{e['from']}>{e['to']}" if e['moved'] else f'{name}:same' for name, e in entries)


def write_reports(entries, output_dir, target):
    """reorient_<t>.json next to the prediction: {input name: entry}.  -> its path."""
    return write_report_json('reorient', {name: e for name, e in entries}, output_dir, target)
