"""Host reference for the --regrid tests (numpy only, fp64): what mud_volume_regrid must compute (include/mudiff_hip.h), and the grids
the tests resample between."""
import numpy as np

SRC_SHAPE, REF_SHAPE = (70, 23, 17), (75, 18, 20)        # x crosses a wave and a 256-thread workgroup; nothing is a multiple of 64
EXACT_CASES = ('identity', 'shift', 'flip', 'dyadic')     # every product and sum of these is exact in fp64


def _affine(lin, offset):
    a = np.eye(4)
    a[:3, :3] = lin
    a[:3, 3] = offset
    return a


def oblique_linear():
    """Rz(0.3) . Rx(-0.17) . diag(1.1, 0.9, 1.3)."""
    c, s = np.cos(0.3), np.sin(0.3)
    rz = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]])
    c, s = np.cos(-0.17), np.sin(-0.17)
    rx = np.array([[1.0, 0, 0], [0, c, -s], [0, s, c]])
    return rz @ rx @ np.diag([1.1, 0.9, 1.3])


def case(name, src_shape=SRC_SHAPE, ref_shape=REF_SHAPE):
    """-> (source shape, source affine, reference shape, reference affine)."""
    src_shape, ref_shape = tuple(src_shape), tuple(ref_shape)
    if name == 'identity':
        return src_shape, np.eye(4), src_shape, np.eye(4)
    if name == 'shift':
        return src_shape, np.eye(4), ref_shape, _affine(np.eye(3), (3.0, -2.0, 1.0))
    if name == 'flip':                                    # x and y reversed: reference voxel (i, j, k) is source voxel (SX-1-i, SY-1-j, k)
        return src_shape, np.eye(4), ref_shape, _affine(np.diag([-1.0, -1.0, 1.0]), (src_shape[0] - 1.0, src_shape[1] - 1.0, 0.0))
    if name == 'dyadic':
        return src_shape, _affine(np.diag([1.0, 2.0, 1.0]), (0, 0, 0)), ref_shape, _affine(np.diag([2.0, 1.0, 0.5]), (1.0, -1.0, 0.5))
    if name == 'oblique':                                 # both grid centres at world 0, the reference 1 mm isotropic
        lin = oblique_linear()
        cs, cr = (np.array(src_shape) - 1) / 2.0, (np.array(ref_shape) - 1) / 2.0
        return src_shape, _affine(lin, -lin @ cs), ref_shape, _affine(np.eye(3), -cr)
    if name == 'outside':                                 # the reference wholly outside the source's field of view
        return src_shape, np.eye(4), ref_shape, _affine(np.eye(3), (1000.0, 0.0, 0.0))
    raise ValueError(name)


def matrix(src_affine, ref_affine):
    return np.linalg.solve(np.asarray(src_affine, np.float64), np.asarray(ref_affine, np.float64))


def coordinates(M, out_shape):
    """p = M (i, j, k, 1) in fp64 for every voxel of the reference grid -> three [X,Y,Z] arrays."""
    M = np.asarray(M, np.float64)
    i, j, k = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in out_shape], indexing='ij')
    return [((M[a, 0] * i + M[a, 1] * j) + M[a, 2] * k) + M[a, 3] for a in range(3)]


def trilinear(src, M, out_shape):
    """src: fp32 [SX,SY,SZ] (the values the pipeline sees) -> fp32 [X,Y,Z]: the fp64 sum over the 8 neighbours of value * weight,
    rounded once; a neighbour outside the grid counts as 0, one of weight exactly 0 is not read."""
    src = np.asarray(src, np.float32)
    p = coordinates(M, out_shape)
    f = [np.floor(v) for v in p]
    w = [v - fv for v, fv in zip(p, f)]
    acc = np.zeros(tuple(out_shape), np.float64)
    with np.errstate(invalid='ignore'):
        for dz in (0, 1):
            for dy in (0, 1):
                for dx in (0, 1):
                    idx = [fv + d for fv, d in zip(f, (dx, dy, dz))]
                    wgt = ((w[0] if dx else 1.0 - w[0]) * (w[1] if dy else 1.0 - w[1])) * (w[2] if dz else 1.0 - w[2])
                    use = wgt != 0
                    for a in range(3):
                        use &= (idx[a] >= 0) & (idx[a] < src.shape[a])
                    ii = [np.clip(np.nan_to_num(idx[a]), 0, src.shape[a] - 1).astype(np.int64) for a in range(3)]
                    v = src[ii[0], ii[1], ii[2]].astype(np.float64)
                    acc = acc + np.where(use, np.where(use, v, 0.0) * wgt, 0.0)
    return acc.astype(np.float32)


def nearest(src, M, out_shape):
    """The value at floor(p + 0.5) per axis, 0 outside the source -> fp32 [X,Y,Z]."""
    src = np.asarray(src, np.float32)
    q = [np.floor(v + 0.5) for v in coordinates(M, out_shape)]
    inside = np.ones(tuple(out_shape), bool)
    for a in range(3):
        inside &= (q[a] >= 0) & (q[a] < src.shape[a])
    ii = [np.clip(np.nan_to_num(q[a]), 0, src.shape[a] - 1).astype(np.int64) for a in range(3)]
    return np.where(inside, src[ii[0], ii[1], ii[2]], np.float32(0)).astype(np.float32)


def near_half_integer(M, out_shape, eps=1e-9):
    """Voxels whose coordinate is within eps of a half-integer on some axis: there floor(p + 0.5) may fall either way."""
    out = np.zeros(tuple(out_shape), bool)
    for v in coordinates(M, out_shape):
        out |= np.abs((v - np.floor(v)) - 0.5) <= eps
    return out
