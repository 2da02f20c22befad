"""Host reference for the --foreground tests (numpy only): the definition of DESIGN.md section 5.16 that the kernels of
csrc/volume_foreground.hip mirror - candidates, histogram, Otsu, raw mask, opening, largest component, hole filling, output, report - the
adversarial masks of the labelling tests and the phantom of the recovery tests.  Volumes are [X,Y,Z] arrays as everywhere in the tests;
a linear index has x fastest: i = x + X * (y + Y * z).  Everything except the Otsu scan is integer work, so the device must equal this
restatement bit for bit."""
import numpy as np

PHANTOM_SHAPE = (37, 29, 23)
# what this restatement gives on the phantom (256 bins, no opening): the Otsu bin, the Dice of the raw mask, of
# the largest component and of the filled mask against the true ellipsoid, and the ventricle voxels the filling brought back
RECORDED = dict(bin=87, dice_raw=0.9906, dice_largest=0.9940, dice_filled=1.0, ventricle=81)
DICE_SLACK = 0.005


# ---- the definition ---------------------------------------------------------------------------------------------------------------------
def candidates(values):
    v = np.asarray(values, np.float32)
    return np.isfinite(v) & (v != 0)


def bin_of(values, lo, scale, bins):
    """vc_bin: clamp(floor((double(v) - lo) * scale), 0, bins - 1), the subtraction and the product rounded separately."""
    with np.errstate(invalid='ignore', over='ignore'):
        d = np.floor((np.asarray(values, np.float32).astype(np.float64) - float(lo)) * float(scale))
        d = np.where(d > 0.0, d, 0.0)              # (a NaN goes to 0, as in the kernel; it is never a candidate)
        d = np.where(d < bins - 1.0, d, bins - 1.0)
    return d.astype(np.int64)


def otsu(counts):
    """Brute force, in fp64 and in index order -> the first k in [0, bins - 2] with the largest s_k, None with fewer than two non-empty bins."""
    c = [int(v) for v in counts]
    if sum(1 for v in c if v) < 2:
        return None
    n, mt = sum(c), float(sum(i * v for i, v in enumerate(c)))
    best, best_s = None, -1.0
    for k in range(len(c) - 1):
        a, m0 = sum(c[:k + 1]), sum(i * v for i, v in enumerate(c[:k + 1]))
        b = n - a
        if a == 0 or b == 0:
            continue
        d = float(m0) / float(a) - (mt - float(m0)) / float(b)
        s = float(a) * float(b) * (d * d)
        if s > best_s:
            best, best_s = k, s
    return best


def _shifted(mask, axis, step, fill):
    out = np.full(mask.shape, fill, bool)
    src = [slice(None)] * 3
    dst = [slice(None)] * 3
    if step > 0:
        src[axis], dst[axis] = slice(0, -1), slice(1, None)
    else:
        src[axis], dst[axis] = slice(1, None), slice(0, -1)
    out[tuple(dst)] = mask[tuple(src)]
    return out


def erode(mask):
    """On iff the voxel and its six face neighbours are on; a neighbour outside the volume counts as on."""
    m = np.asarray(mask, bool)
    out = m.copy()
    for axis in range(3):
        for step in (1, -1):
            out &= _shifted(m, axis, step, True)
    return out


def dilate(mask):
    """On iff the voxel or one of its six face neighbours is on; a neighbour outside the volume counts as off."""
    m = np.asarray(mask, bool)
    out = m.copy()
    for axis in range(3):
        for step in (1, -1):
            out |= _shifted(m, axis, step, False)
    return out


def label(mask, value=1):
    """The 6-connected components of the voxels where (mask != 0) == (value != 0) -> int32 [X,Y,Z]: the smallest linear index (x fastest)
    of each voxel's component, -1 elsewhere.  A sequential union-find over the face-neighbour pairs."""
    member = (np.asarray(mask) != 0) == (value != 0)
    X, Y, Z = member.shape
    flat = member.reshape(-1, order='F')
    index = np.arange(flat.size, dtype=np.int64).reshape(member.shape, order='F')
    parent = list(range(flat.size))

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i

    for a, b in ((np.s_[1:, :, :], np.s_[:-1, :, :]), (np.s_[:, 1:, :], np.s_[:, :-1, :]), (np.s_[:, :, 1:], np.s_[:, :, :-1])):
        both = member[a] & member[b]
        for i, j in zip(index[a][both].tolist(), index[b][both].tolist()):
            ri, rj = find(i), find(j)
            if ri != rj:
                parent[max(ri, rj)] = min(ri, rj)      # the smaller index is the root: the root is the component's smallest index
    roots = np.array([find(i) for i in range(flat.size)], np.int64)
    return np.where(flat, roots, -1).astype(np.int32).reshape(member.shape, order='F')


def census(labels):
    """-> (counts int64 [n] by root, face bool [n] by root, winner root or None, number of components): the census of the components; the
    winner is the largest, the smallest root on a tie."""
    lab = np.asarray(labels)
    flat = lab.reshape(-1, order='F')
    n = flat.size
    counts = np.bincount(flat[flat >= 0], minlength=n).astype(np.int64)
    border = np.zeros(lab.shape, bool)
    border[0], border[-1], border[:, 0], border[:, -1], border[:, :, 0], border[:, :, -1] = (True,) * 6
    face = np.zeros(n, bool)
    face[flat[(flat >= 0) & border.reshape(-1, order='F')]] = True
    roots = np.flatnonzero(counts)
    winner = int(roots[np.argmax(counts[roots])]) if roots.size else None      # (argmax: the first, i.e. the smallest root, of the largest)
    return counts, face, winner, int(roots.size)


def largest(mask):
    """-> (the largest component of the mask as bool, the number of components)."""
    lab = label(mask, 1)
    _, _, winner, components = census(lab)
    return (lab == winner) if components else np.zeros(lab.shape, bool), components


def fill_holes(mask):
    """The mask plus every component of its complement that has no voxel on a face of the volume."""
    lab = label(mask, 0)
    _, face, _, _ = census(lab)
    flat = lab.reshape(-1, order='F')
    hole = (flat >= 0) & ~face[np.where(flat >= 0, flat, 0)]
    return np.asarray(mask, bool) | hole.reshape(lab.shape, order='F')


def foreground(values, bins=256, open=0, keep_holes=False):      # noqa: A002
    """fp32 values [X,Y,Z] -> (output fp32 [X,Y,Z] or None for an input that is left untouched, mask bool or None, report, stages): the
    whole definition.  stages: the raw mask and the largest component, for the recovery figures."""
    v = np.asarray(values, np.float32)
    cand = candidates(v)
    report = dict(threshold=None, bin=None, bins=int(bins), lo=None, hi=None, candidates=int(cand.sum()), components=0, kept=0, filled=0,
                  removed=0, open=int(open), keep_holes=bool(keep_holes))
    if not cand.any():
        return None, None, report, {}
    lo, hi = float(v[cand].min()), float(v[cand].max())
    report['lo'], report['hi'] = lo, hi
    if hi == lo:
        return None, None, report, {}
    scale = bins / (hi - lo)
    b = bin_of(v, lo, scale, bins)
    k = otsu(np.bincount(b[cand], minlength=bins))
    if k is None:
        return None, None, report, {}
    report['bin'], report['threshold'] = k, lo + (k + 1) / scale
    raw = cand & (b > k)
    mask = raw
    for _ in range(open):
        mask = erode(mask)
    for _ in range(open):
        mask = dilate(mask)
    kept, report['components'] = largest(mask)
    final = kept if keep_holes else fill_holes(kept)
    report['filled'] = int(final.sum() - kept.sum())
    report['kept'] = int(final.sum())
    report['removed'] = int((cand & ~final).sum())
    out = np.where(final, v, np.float32(0.0)).astype(np.float32)
    out[final] = v[final]                          # (the bits as they are, a NaN's included)
    return out, final, report, dict(raw=raw, largest=kept)


# ---- the masks of the labelling tests -----------------------------------------------------------------------------------------------------
def serpentine(shape):
    """A one-voxel-wide path through every second row of every second plane: one component, the longest chains a labelling can meet."""
    X, Y, Z = shape
    m = np.zeros(shape, np.uint8)
    x = y = 0
    dirx = diry = 1
    for z in range(0, Z, 2):
        while True:
            m[:, y, z] = 1
            x = X - 1 if dirx > 0 else 0
            dirx = -dirx
            if not 0 <= y + 2 * diry < Y:
                break
            m[x, y + diry, z] = 1
            y += 2 * diry
        diry = -diry
        if z + 2 < Z:
            m[x, y, z + 1] = 1
    return m


def label_masks(shape, seed=3):
    """{name: uint8 [X,Y,Z]}: all on, all off, a single voxel, the checkerboard (every voxel its own component), the serpentine, a comb
    whose teeth (along z) join only in the last plane, random masks at three densities."""
    X, Y, Z = shape
    x, y, z = np.meshgrid(np.arange(X), np.arange(Y), np.arange(Z), indexing='ij')
    rng = np.random.default_rng(seed + X)
    single = np.zeros(shape, np.uint8)
    single[X // 2, Y // 2, Z // 2] = 1
    masks = {'on': np.ones(shape, np.uint8), 'off': np.zeros(shape, np.uint8), 'single': single,
             'checker': ((x + y + z) % 2 == 0).astype(np.uint8), 'serpentine': serpentine(shape),
             'comb': (((x % 2 == 0) & (y % 2 == 0)) | (z == Z - 1)).astype(np.uint8)}
    for density in (0.3, 0.5, 0.7):
        masks[f'random{density}'] = (rng.random(shape) < density).astype(np.uint8)
    return masks


def canonical(labelled):
    """scipy.ndimage.label's output (1 .. N, 0 for background) -> the smallest linear index of each component, -1 for background."""
    lab = np.asarray(labelled)
    flat = lab.reshape(-1, order='F').astype(np.int64)
    first = np.full(int(flat.max()) + 1, flat.size, np.int64)
    np.minimum.at(first, flat, np.arange(flat.size, dtype=np.int64))
    return np.where(flat > 0, first[flat], -1).astype(np.int32).reshape(lab.shape, order='F')


# ---- the phantom of the recovery tests ----------------------------------------------------------------------------------------------------
def phantom(shape=PHANTOM_SHAPE, seed=5, sigma=20.0):
    """-> (noisy fp32 [X,Y,Z], the true head (ellipsoid) bool, the ventricle bool, the detached block bool).  An ellipsoid of semi-axes
    0.40 X, 0.40 Y, 0.42 Z about the centre (s - 1) / 2 holding 500 + 200 cos(x / 5) sin(y / 4), a dark sphere of radius 0.12 Z (value
    15) in its middle, a detached block of 700 in the corner x < 4, y < 4, z < 3, and Rician noise of sigma 20 everywhere."""
    X, Y, Z = shape
    x, y, z = np.meshgrid(np.arange(X, dtype=np.float64), np.arange(Y, dtype=np.float64), np.arange(Z, dtype=np.float64), indexing='ij')
    cx, cy, cz = (X - 1) / 2, (Y - 1) / 2, (Z - 1) / 2
    head = ((x - cx) / (0.40 * X)) ** 2 + ((y - cy) / (0.40 * Y)) ** 2 + ((z - cz) / (0.42 * Z)) ** 2 <= 1.0
    ventricle = (x - cx) ** 2 + (y - cy) ** 2 + (z - cz) ** 2 <= (0.12 * Z) ** 2
    block = (x < 4) & (y < 4) & (z < 3)
    clean = np.where(head, 500.0 + 200.0 * np.cos(x / 5.0) * np.sin(y / 4.0), 0.0)
    clean[ventricle] = 15.0
    clean[block] = 700.0
    rng = np.random.default_rng(seed)
    n1, n2 = rng.normal(0.0, sigma, shape), rng.normal(0.0, sigma, shape)
    return np.sqrt((clean + n1) ** 2 + n2 ** 2).astype(np.float32), head, ventricle, block


def dice(a, b):
    a, b = np.asarray(a, bool), np.asarray(b, bool)
    return 2.0 * float((a & b).sum()) / float(a.sum() + b.sum())
