"""Host reference for the device intake tests (numpy only): what the kernels of csrc/volume_intake.hip must reproduce bit for bit,
stated with np.sort and the numpy expressions of mudiff_hip.volume, plus the synthetic volumes and NIfTI files the tests use."""
import gzip
import struct

import numpy as np

CODES = {'u1': 2, 'i2': 4, 'i4': 8, 'f4': 16, 'u2': 512}


def is_scaled(slope, inter):
    """volume.read_nifti's rule."""
    slope, inter = float(np.float32(slope)), float(np.float32(inter))
    return slope != 0.0 and np.isfinite(slope) and (slope != 1.0 or inter != 0.0)


def values_float32(raw, slope=1.0, inter=0.0):
    """The fp32 value of every stored voxel: read_nifti's float64 conversion and scaling, then robust_minmax's astype(float32)."""
    d = np.asarray(raw).astype(np.float64)
    if is_scaled(slope, inter):
        d = d * float(np.float32(slope)) + float(np.float32(inter))
    return d.astype(np.float32)


def sorted_selected(values):
    """np.sort of the voxels with value != 0 (the mask=None selection of robust_minmax_to_minus1_1)."""
    v = np.asarray(values, np.float32).reshape(-1)
    return np.sort(v[v != 0])


def window(s, q):
    """(first rank, exact sorted values) at the ranks [r - 8, r + 7] clipped to [0, n), r = floor((n - 1) q) in fp64."""
    n = int(s.size)
    if n == 0:
        return 0, np.zeros(0, np.float32)
    r = int(np.floor(float(n - 1) * float(q)))
    a, b = max(0, r - 8), min(n - 1, r + 7)
    return a, s[a:b + 1]


def normalise(values, lo, hi_minus_lo):
    """The numpy expression of volume.robust_minmax_to_minus1_1's last line on fp32 values."""
    data = np.asarray(values, np.float32)
    return np.clip((data - np.float32(lo)) / np.float32(hi_minus_lo), 0.0, 1.0) * 2.0 - 1.0


def slab_range(z, half_range):
    c = z // 2
    return max(0, c - half_range), min(z - 1, c + half_range)


def stack_planes(vol_xyz, s0, s1):
    """[X,Y,Z] -> [n,X,Y]: extract_center_slices + np.stack."""
    return np.stack([vol_xyz[:, :, k] for k in range(s0, s1 + 1)], 0)


def synthetic(shape, kind, dtype, seed=0):
    """An [X,Y,Z] volume of `dtype` (F-ordered, like a file's): 'ties' integer intensities inside an ellipsoid (thousands of voxels per
    level), 'single' one non-zero voxel, 'zeros' all zero, 'noise' distinct values of both signs where the dtype has them."""
    rng = np.random.default_rng(seed)
    dt = np.dtype(dtype)
    X, Y, Z = shape
    if kind == 'zeros':
        v = np.zeros(shape)
    elif kind == 'single':
        v = np.zeros(shape)
        v[X // 3, Y // 2, Z // 2] = 77
    elif kind == 'ties':
        x, y, z = np.meshgrid(np.linspace(-1, 1, X), np.linspace(-1, 1, Y), np.linspace(-1, 1, Z), indexing='ij')
        inside = (x / 0.8) ** 2 + (y / 0.7) ** 2 + (z / 0.75) ** 2 < 1
        top = 200 if dt.itemsize == 1 else 1500
        v = np.where(inside, rng.integers(1, top, shape), 0)
    elif kind == 'noise':
        if dt.kind == 'f':
            v = rng.standard_normal(shape) * 1000 * (rng.random(shape) > 0.3)
        else:
            info = np.iinfo(dt)
            v = rng.integers(max(info.min, -30000), min(info.max, 30000), shape) * (rng.random(shape) > 0.3)
    else:
        raise ValueError(kind)
    return np.asfortranarray(v.astype(dt))


def write_nifti_typed(path, vol, endian='<', slope=0.0, inter=0.0, affine=None):
    """A single-file NIfTI-1 of `vol` ([X,Y,Z], any of the supported dtypes plus f8 / i1) stored in its own datatype and byte order."""
    vol = np.asarray(vol)
    codes = dict(CODES, f8=64, i1=256)
    code = codes[vol.dtype.kind + str(vol.dtype.itemsize)]
    affine = np.eye(4) if affine is None else np.asarray(affine)
    raw = bytearray(348)
    struct.pack_into(endian + 'i', raw, 0, 348)
    struct.pack_into(endian + '8h', raw, 40, 3, *vol.shape, 1, 1, 1, 1)
    struct.pack_into(endian + 'h', raw, 70, code)
    struct.pack_into(endian + 'h', raw, 72, 8 * vol.dtype.itemsize)
    struct.pack_into(endian + '8f', raw, 76, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0)
    struct.pack_into(endian + 'f', raw, 108, 352.0)
    struct.pack_into(endian + '2f', raw, 112, slope, inter)
    struct.pack_into(endian + 'h', raw, 254, 1)
    for r in range(3):
        struct.pack_into(endian + '4f', raw, 280 + 16 * r, *[float(v) for v in affine[r]])
    raw[344:348] = b'n+1\0'
    payload = bytes(raw) + b'\0\0\0\0' + vol.astype(vol.dtype.newbyteorder(endian)).tobytes(order='F')
    opener = gzip.open if str(path).endswith('.gz') else open
    with opener(str(path), 'wb') as f:
        f.write(payload)
    return str(path)
