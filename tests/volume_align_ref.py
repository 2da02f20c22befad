"""Host reference for the --align tests (numpy only, fp64): what mud_volume_mirror_moments must compute (include/mudiff_hip.h), by
volume_coreg_ref's overlap, trilinear and bin rules, and the analytic "head" whose planted mid-sagittal plane the recovery tests find."""
import numpy as np

import volume_coreg_ref as K

SHAPE, SPACING = (48, 44, 40), (1.5, 1.5, 2.0)
POSES = ((7.0, -5.0, 3.0), (-12.0, 9.0, -4.5), (0.0, 0.0, 0.0))      # (yaw deg, roll deg, offset mm): two tilted heads and the untilted one
SEARCH = dict(max_deg=20.0, max_mm=12.0, step_deg=5.0, step_mm=4.0, final_deg=0.35, final_mm=0.25, strides=(2, 1))
BINS = 32


def moments(vol, M, stride, lo, scale, bins, details=False):
    """vol: fp32 [X,Y,Z] (the values the pipeline sees); M: voxel index -> the voxel coordinate of its mirror image -> int64 [6]: n, sum a,
    sum b, sum a^2, sum b^2, sum a b of the bin indices a (the voxel) and b (the trilinear value at M x) over the overlap, from
    volume_coreg_ref.joint_hist of the volume with itself.  With `details` also joint_hist's dict (for n_edge)."""
    hist, info = K.joint_hist(vol, vol, M, stride, (lo, scale, lo, scale), bins, details=True)
    i = np.arange(bins, dtype=np.int64)
    ra, rb = hist.sum(1), hist.sum(0)
    out = np.array([hist.sum(), (ra * i).sum(), (rb * i).sum(), (ra * i * i).sum(), (rb * i * i).sum(), (hist * np.outer(i, i)).sum()], np.int64)
    return (out, info) if details else out


def moments_of(vol, mats, stride, lo, scale, bins):
    """[K, 3, 4] matrices -> int64 [K, 6]."""
    return np.stack([moments(vol, M, stride, lo, scale, bins) for M in np.asarray(mats, np.float64).reshape(-1, 3, 4)])


def bin_range(vol, bins):
    """(lo, scale) of mudiff_hip.volume_align.estimate for a value array: `bins` equal bins between the finite minimum and maximum."""
    lo, scale, _, _ = K.ranges_of(vol, vol, bins)
    return lo, scale


# ---------------------------------------------------------------------------------------------------
# the analytic head
# ---------------------------------------------------------------------------------------------------
def affine(shape=SHAPE, spacing=SPACING, oblique=True):
    """A voxel -> world matrix: the spacing, turned by Rz(3 deg) . Rx(-2 deg) when oblique, the grid centre at world (5, -8, 12)."""
    lin = np.diag(np.asarray(spacing, np.float64))
    if oblique:
        cz, sz, cx, sx = np.cos(np.deg2rad(3.0)), np.sin(np.deg2rad(3.0)), np.cos(np.deg2rad(-2.0)), np.sin(np.deg2rad(-2.0))
        lin = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1.0]]) @ np.array([[1.0, 0, 0], [0, cx, -sx], [0, sx, cx]]) @ lin
    a = np.eye(4)
    a[:3, :3] = lin
    a[:3, 3] = np.array([5.0, -8.0, 12.0]) - lin @ ((np.asarray(shape, np.float64) - 1.0) / 2.0)
    return a


def phantom(pose, shape=SHAPE, A=None, lesion=True, dtype=np.int16, scale=1.0):
    """A head that is symmetric about the plane n . (p - c) = t of `pose` = (yaw, roll, t) (mudiff_hip.volume_align's definitions; c: the
    world position of the grid centre), sampled on the grid of A: a bright shell, tissue with an even texture and a pair of dark
    "ventricles", in the coordinates q = R^T (p - c - t n) in which the plane is q_x = 0; plus, with `lesion`, one bright blob on one
    side only.  The head is about 44 x 55 x 63 mm, times `scale`.  -> the stored [X,Y,Z] array (Fortran order)."""
    from mudiff_hip import volume_align as VA
    A = affine(shape) if A is None else np.asarray(A, np.float64)
    yaw, roll, t = pose
    R = VA.rotation(yaw, roll)
    c = A[:3, :3] @ ((np.asarray(shape, np.float64) - 1.0) / 2.0) + A[:3, 3]
    g = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing='ij')
    p = np.stack([A[a, 0] * g[0] + A[a, 1] * g[1] + A[a, 2] * g[2] + A[a, 3] for a in range(3)], -1)
    q = (p - c - t * R[:, 0]) @ R                         # rows: R^T (p - c - t n)
    x, y, z = q[..., 0] / scale, q[..., 1] / scale, q[..., 2] / scale
    e = np.sqrt((x / 21.0) ** 2 + (y / 26.0) ** 2 + (z / 30.0) ** 2)
    inside = 1.0 / (1.0 + np.exp((e - 0.80) / 0.05))
    v = 900.0 * np.exp(-((e - 0.95) / 0.10) ** 2)
    v = v + inside * (420.0 + 140.0 * np.cos(0.33 * x) * np.cos(0.21 * y + 0.5) + 90.0 * np.sin(0.27 * z) * np.cos(0.19 * x)
                      + 60.0 * np.cos(0.5 * np.abs(x) + 0.4 * y - 0.3 * z))
    for sx in (-1.0, 1.0):                               # the pair of ventricles
        v = v - inside * 260.0 * np.exp(-(((x - 7.0 * sx) / 4.0) ** 2 + ((y - 2.0) / 9.0) ** 2 + ((z - 4.0) / 5.0) ** 2))
    if lesion:
        v = v + inside * 300.0 * np.exp(-(((x - 11.0) / 4.0) ** 2 + ((y + 9.0) / 4.5) ** 2 + ((z - 6.0) / 4.0) ** 2))
    return np.asfortranarray(np.rint(v).astype(dtype))


def host_cost(vol, A, centre, lo, scale, bins):
    """The cost callable of mudiff_hip.volume_align.search over the numpy moments: (candidates [K, 3], stride) -> int64 [K, 6]."""
    from mudiff_hip import volume_align as VA
    vol = np.asarray(vol, np.float32)
    return lambda cand, stride: moments_of(vol, VA.mirror_matrices(cand, A, centre), stride, lo, scale, bins)


def flip_correlation(vol):
    """Pearson r of a [X,Y,Z] volume with its own flip along the first axis (fp64)."""
    a = np.asarray(vol, np.float64)
    b = a[::-1]
    a, b = a - a.mean(), b - b.mean()
    return float((a * b).sum() / np.sqrt((a * a).sum() * (b * b).sum()))
