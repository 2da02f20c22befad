"""Host reference for the --reorient tests (numpy only): the definition of DESIGN.md section 5.20 restated independently of
mudiff_hip.volume_reorient - the permutation as a transpose plus slices, the orientation code by brute force over all 48 signed
permutations - and the fixtures both test files share."""
import itertools

import numpy as np

POSITIVE, NEGATIVE = 'RAS', 'LPI'
CODES = tuple(''.join(POSITIVE[w] if s > 0 else NEGATIVE[w] for w, s in zip(order, signs))
              for order in itertools.permutations(range(3)) for signs in itertools.product((1, -1), repeat=3))
BRATS = np.array([[-1., 0, 0, 0], [0, -1, 0, 239], [0, 0, 1, 0], [0, 0, 0, 1]])


def apply(vol, perm, flip):
    """dst[i0, i1, i2] = src[j], j[perm[o]] = S[perm[o]] - 1 - i_o if flip[o] else i_o -> a C-contiguous copy."""
    out = np.transpose(np.asarray(vol), perm)
    for o, f in enumerate(flip):
        if f:
            out = np.flip(out, o)
    return np.ascontiguousarray(out)


def axcodes(affine):
    """The code whose signed permutation has the largest sum of cosines with the normalised columns (ties: the first in CODES order)."""
    lin = np.asarray(affine, np.float64)[:3, :3]
    cos = lin / np.sqrt((lin * lin).sum(0))
    best, best_score = None, -np.inf
    for order in itertools.permutations(range(3)):                 # order[v]: the world axis of voxel axis v
        for signs in itertools.product((1, -1), repeat=3):
            score = sum(signs[v] * cos[order[v], v] for v in range(3))
            if score > best_score + 1e-12:
                best, best_score = ''.join((POSITIVE if signs[v] > 0 else NEGATIVE)[order[v]] for v in range(3)), score
    return best


def affine_of(code, shape, spacing=(1.0, 1.0, 1.0), origin=(0.0, 0.0, 0.0)):
    """An axis-aligned affine whose voxel axes run as `code` says, `spacing` millimetres apart (per voxel axis); `origin`: the world
    position of voxel (0, 0, 0)."""
    a = np.zeros((4, 4))
    for v, letter in enumerate(code):
        w = POSITIVE.index(letter) if letter in POSITIVE else NEGATIVE.index(letter)
        a[w, v] = spacing[v] if letter in POSITIVE else -spacing[v]
    a[:3, 3] = origin
    a[3, 3] = 1.0
    return a


def rotation(axis, degrees):
    """The 4 x 4 rotation about world axis `axis` (0, 1, 2)."""
    t = np.radians(degrees)
    c, s = np.cos(t), np.sin(t)
    r = np.eye(4)
    i, j = [(1, 2), (2, 0), (0, 1)][axis]
    r[i, i], r[i, j], r[j, i], r[j, j] = c, -s, s, c
    return r


def stored_as(vol_lps, lps_affine, code):
    """A volume given in LPS storage -> (the same voxels stored in the orientation `code`, the affine that keeps every voxel where it
    was): the inverse of what --reorient does, by this file's own arithmetic."""
    perm, flip, t = [], [], np.zeros((4, 4))
    for o, letter in enumerate(code):
        w = POSITIVE.index(letter) if letter in POSITIVE else NEGATIVE.index(letter)
        perm.append(w)                                            # LPS storage: voxel axis w runs along world axis w
        flip.append((letter in POSITIVE) != (w == 2))             # ... towards L, P, S
        t[w, o] = -1.0 if flip[-1] else 1.0
        t[w, 3] = vol_lps.shape[w] - 1 if flip[-1] else 0.0
    t[3, 3] = 1.0
    return np.asfortranarray(apply(vol_lps, perm, flip)), np.asarray(lps_affine, np.float64) @ t


def labelled(shape, width):
    """A volume in which a misplaced voxel cannot match: the linear index (x fastest) modulo the width's range plus a non-periodic hash
    of it, as an unsigned integer of `width` bytes, [X, Y, Z] F-ordered."""
    n = int(np.prod(shape))
    i = np.arange(n, dtype=np.uint64)
    h = (i * np.uint64(0x9E3779B97F4A7C15)) ^ (i >> np.uint64(7)) ^ ((i * i) << np.uint64(17))
    v = i + (h >> np.uint64(11))
    dt = np.dtype(f'<u{width}')
    return (v & np.uint64(np.iinfo(dt).max)).astype(dt).reshape(shape, order='F')
