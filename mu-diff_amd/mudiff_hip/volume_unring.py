"""Removal of truncation (Gibbs) ringing from the inputs (--unring; csrc/volume_unring.hip; DESIGN.md section 5.30 holds the definition).

A finite k-space window lays ripples next to every sharp edge of an image; the generators were never trained on them and copy them from
the conditioning contrasts into the synthesised one.  With --unring every input is corrected on its own grid, where the ripples still sit
on the sampling lattice, by the local sub-voxel-shift method (Kellner et al. 2016, what MRtrix's mrdegibbs runs): per image line a bank of
2 N + 1 sub-voxel shifts, per voxel the shift of the smallest local total variation, re-interpolated to the voxel's centre:

    host, once per size: the tables - twiddles and direction kernels of the filter (fp64), D_s of the shift bank (fp64, rounded to fp32)
    stored voxels --mud_volume_unring_filter--> Ix, Iy (fp32 [Z,Y,X]): the slices split by Gx = cy / (cx + cy), Ix + Iy = I
    mud_volume_unring_lines along axes[0] on Ix, in place; along axes[1] on Iy, added to it
    --> fp32 [Z,Y,X], a volume like a regridded one, with the source's own geometry; two uint64 counters per pass for the report

All per-voxel work is the device's; every sum runs in a fixed order and the counters are integers: two runs give the same bits.

Limits: the data must not be zero-filled or partial-Fourier (the ripples of an interpolated image do not sit on its lattice); only the
two axes of --unring_axes are corrected, a 3D acquisition's third axis is not; the lines are treated as circular; the defaults are
MRtrix's and untuned here; the benefit on trained weights is unmeasured.
"""
from __future__ import annotations

import functools

import numpy as np

from .volume_intake import upload, write_report_json
from .volume_regrid import RegriddedVolume

MAX_SHIFTS, MAX_WINDOW, MAX_LINE = 32, 8, 512
DEFAULTS = dict(axes=(0, 1), shifts=20, window=(1, 3))


class UnringedVolume(RegriddedVolume):
    """A RawVolume whose voxels live on the device (fp32 [Z,Y,X]) with the shape, affine and header of the volume it was made from."""


def check_options(axes=(0, 1), shifts=20, window=(1, 3)):
    """ValueError (with the flag's name) for a value the kernels cannot run with."""
    axes = tuple(axes)
    if len(axes) != 2 or any(int(a) != a or not 0 <= a <= 2 for a in axes) or axes[0] == axes[1]:
        raise ValueError(f'--unring_axes takes two distinct storage axes out of 0, 1, 2 (got {list(axes)})')
    if int(shifts) != shifts or not 1 <= shifts <= MAX_SHIFTS:
        raise ValueError(f'--unring_shifts must be in [1, {MAX_SHIFTS}] (got {shifts})')
    window = tuple(window)
    if len(window) != 2 or any(int(w) != w for w in window) or not 1 <= window[0] <= window[1] <= MAX_WINDOW:
        raise ValueError(f'--unring_window takes A B with 1 <= A <= B <= {MAX_WINDOW} (got {list(window)})')


def check_shape(shape, name, axes=(0, 1), shifts=20, window=(1, 3)):
    """ValueError, naming the input and the flag, for in-plane axes the kernels do not take: shorter than 2 B + 2 or longer than 512."""
    for axis in axes:
        n = int(shape[axis])
        if n < 2 * window[1] + 2:
            raise ValueError(f'{name}: axis {axis} has {n} voxels, fewer than the 2 B + 2 = {2 * window[1] + 2} that --unring_window {window[0]} '
                             f'{window[1]} needs (--unring_axes {axes[0]} {axes[1]})')
        if n > MAX_LINE:
            raise ValueError(f'{name}: axis {axis} has {n} voxels, more than the {MAX_LINE} --unring takes (--unring_axes {axes[0]} {axes[1]})')


# ---------------------------------------------------------------------------------------------------
# the tables (fp64 -> fp32), built once per size
# ---------------------------------------------------------------------------------------------------
def shift_values(shifts):
    """s_j, j = 0 .. 2 N: 0, +1/K .. +N/K, -1/K .. -N/K with K = 2 N + 1."""
    N, K = int(shifts), 2 * int(shifts) + 1
    return np.array([0.0] + [j / K for j in range(1, N + 1)] + [-(j - N) / K for j in range(N + 1, 2 * N + 1)])


@functools.lru_cache(maxsize=16)
def shift_table(n, shifts):
    """fp32 [2 N + 1, n]: D_s[r], the circulant that samples a band-limited line of n voxels at l + s.  The sum of the definition in
    closed form, t = r + s: sin(pi t) / (n sin(pi t / n)) for odd n, times cos(pi t / n) for even n (whose bin n/2 carries cos(pi s)); the
    unit impulse for s = 0."""
    r = np.arange(n, dtype=np.float64)
    D = np.zeros((2 * shifts + 1, n))
    D[0, 0] = 1.0
    for j, s in enumerate(shift_values(shifts)):
        if j == 0:
            continue
        t = (r + s) / n
        top = np.where(np.arange(n) % 2 == 0, 1.0, -1.0) * np.sin(np.pi * s)          # sin(pi (r + s))
        D[j] = top * (np.cos(np.pi * t) if n % 2 == 0 else 1.0) / (n * np.sin(np.pi * t))
    return D.astype(np.float32)


@functools.lru_cache(maxsize=16)
def filter_tables(nx, ny):
    """-> (twiddle fp64 [nx, 2] = (cos, -sin)(2 pi m / nx); kernel fp64 [nx // 2 + 1, ny]: row kx = the inverse transform along ky of
    Gx(kx, ky) = cy / (cx + cy), c = 1 + cos(2 pi k / n), with 1/2 at the one bin where 2 kx = nx and 2 ky = ny (picked by index))."""
    m = np.arange(nx, dtype=np.float64)
    twiddle = np.stack([np.cos(2 * np.pi * m / nx), -np.sin(2 * np.pi * m / nx)], axis=1)
    nk = nx // 2 + 1
    cx = 1.0 + np.cos(2 * np.pi * np.arange(nk) / nx)[:, None]
    cy = 1.0 + np.cos(2 * np.pi * np.arange(ny) / ny)[None, :]
    den = cx + cy
    corner = nx % 2 == 0 and ny % 2 == 0
    if corner:
        den[nx // 2, ny // 2] = 1.0
    G = cy / den
    if corner:
        G[nx // 2, ny // 2] = 0.5
    return twiddle, np.ascontiguousarray(np.fft.ifft(G, axis=1).real)


def unring(raw, device, axes=(0, 1), shifts=20, window=(1, 3), name='the input', maps=False):
    """A RawVolume (its voxels on the host, or on the device already) -> (UnringedVolume, report).  report: the options, `n` (the length
    of the two axes), `nonfinite` (stored voxels read as 0) and per axis `moved` (the share of voxels whose chosen shift is not 0) and
    `mean_abs_shift` (in voxels, over all voxels).  With maps=True the report also holds `jmaps`, the two int8 [Z,Y,X] device maps of the
    chosen shifts (tests).  ValueError, naming `name` and the flag, for an axis the kernels do not take - before any launch."""
    import torch
    from . import ops
    if len(raw.shape) != 3:
        raise ValueError(f'unring: expected a 3D volume, got shape {tuple(raw.shape)}')
    check_options(axes, shifts, window)
    axes, shifts, window = tuple(int(a) for a in axes), int(shifts), tuple(int(w) for w in window)
    check_shape(raw.shape, name, axes, shifts, window)
    dev, meta = upload(raw, device), raw.kernel_meta('unring')
    nx, ny = raw.shape[axes[0]], raw.shape[axes[1]]
    on_device = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev.device)      # noqa: E731
    ix, iy, nonfinite = ops.volume_unring_filter(dev, *meta, axes, *(on_device(t) for t in filter_tables(nx, ny)))
    normal = 3 - axes[0] - axes[1]
    _, jx, cx = ops.volume_unring_lines(ix, raw.shape, axes[0], normal, shifts, window, on_device(shift_table(nx, shifts)), jmap=maps)
    out, jy, cy = ops.volume_unring_lines(iy, raw.shape, axes[1], normal, shifts, window, on_device(shift_table(ny, shifts)), out=ix,
                                          accumulate=True, jmap=maps)
    counts = torch.stack([cx, cy]).cpu().numpy()
    voxels, K = float(np.prod(raw.shape)), 2 * shifts + 1
    report = dict(axes=list(axes), shifts=shifts, window=list(window), n=[int(nx), int(ny)],
                  nonfinite=int(nonfinite.cpu().numpy().view(np.uint32)[0]), moved=[float(c[0]) / voxels for c in counts],
                  mean_abs_shift=[float(c[1]) / K / voxels for c in counts])
    if maps:
        report['jmaps'], report['counters'] = (jx, jy), [[int(c[0]), int(c[1])] for c in counts]
    return UnringedVolume(out, raw.shape, raw.affine, raw.header), report


# ---------------------------------------------------------------------------------------------------
# the pipeline's side
# ---------------------------------------------------------------------------------------------------
def add_flags(p):
    p = p.later() if hasattr(p, 'later') else p          # volume.VolumeParser: the lists of the parsers before this one are pinned
    p.add_argument('--unring', action='store_true',
                   help='remove truncation (Gibbs) ringing from every input on its own grid, after --denoise and before --foreground, by '
                        'local sub-voxel shifts (Kellner et al. 2016, on the GPU: mudiff_hip.volume_unring); unring_<t>.json next to the '
                        'prediction holds what moved.  Not for zero-filled or partial-Fourier data; --gt_volume / --eval_mask are not unringed')
    p.add_argument('--unring_axes', type=int, nargs=2, default=list(DEFAULTS['axes']), metavar=('A', 'B'),
                   help='the two storage axes of the acquired slices (default 0 1: axial slices of a volume stored x, y, z)')
    p.add_argument('--unring_shifts', type=int, default=DEFAULTS['shifts'], help='N: 2 N + 1 shifts within half a voxel are tried (1 to 32)')
    p.add_argument('--unring_window', type=int, nargs=2, default=list(DEFAULTS['window']), metavar=('A', 'B'),
                   help='the total variation is taken over the voxels A to B away, on either side (1 <= A <= B <= 8)')


def options_from(args):
    """A namespace's --unring_* flags (any may be missing) -> IntakeOptions' `unring`: the keyword arguments of unring, or None without
    --unring.  ValueError, naming the flag, for a value check_options refuses."""
    get = lambda k: getattr(args, 'unring_' + k, DEFAULTS[k])      # noqa: E731
    kw = dict(axes=tuple(get('axes')), shifts=get('shifts'), window=tuple(get('window')))
    check_options(**kw)
    return dict(unring=kw if getattr(args, 'unring', False) else None)


def unring_suffix(reports):
    """What a [done] line gains under --unring (nothing otherwise): ` | unring=<name>,<name>,...`."""
    if not reports:
        return ''
    return ' | unring=' + ','.join(str(r[0]) for r in reports)


def write_reports(reports, output_dir, target):
    """unring_<t>.json next to the prediction: {input name: report}.  -> its path."""
    return write_report_json('unring', {r[0]: r[1] for r in reports}, output_dir, target)
