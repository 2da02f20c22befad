"""Host reference for the --brain_extract tests (numpy only): the definition of DESIGN.md section 5.18 that csrc/volume_brain.hip and
mudiff_hip.volume_brain mirror - the exact squared Euclidean distance transform by brute force, the morphological brain mask built from it
and from volume_foreground_ref's Otsu, labelling and hole filling - and the head phantom of the recovery tests.  Volumes are [X,Y,Z] arrays
as everywhere in the tests.  Every fp64 operation is one IEEE operation in a stated order, so the device must equal this bit for bit."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import volume_foreground_ref as F

PHANTOM_SHAPE = (48, 40, 36)
PHANTOM_RADII = dict(erode_mm=2.5, dilate_mm=3.5)
AIR, BRAIN, VENTRICLE, GAP, SCALP, BRIDGE = range(6)


# ---- the definition ---------------------------------------------------------------------------------------------------------------------
def _table(n, w):
    """[i, j] = w * ((i - j) * (i - j)): the integer square is exact, the product is rounded once."""
    d = np.arange(n, dtype=np.int64)[:, None] - np.arange(n, dtype=np.int64)[None, :]
    return np.float64(w) * (d * d).astype(np.float64)


def edt2(mask, value, spacing, workers=8):
    """fp64 [X,Y,Z]: min over the voxels q with (mask[q] != 0) == (value != 0) of ((wx * dx^2) + (wy * dy^2)) + (wz * dz^2), w = the
    squared spacing rounded once, every product and sum rounded separately; +inf without such a voxel.  Brute force over every (target,
    member) pair, a plane of targets against a plane of members at a time (numpy releases the GIL: the planes of targets share threads)."""
    member = (np.asarray(mask) != 0) == (value != 0)
    X, Y, Z = member.shape
    sx, sy, sz = (np.float64(s) for s in spacing)
    tx, ty, tz = _table(X, sx * sx), _table(Y, sy * sy), _table(Z, sz * sz)
    txy = (tx[None, :, None, :] + ty[:, None, :, None]).reshape(X * Y, X * Y)      # [x + X * y of the target, x + X * y of the member]
    out = np.full((X * Y, Z), np.inf)
    with ThreadPoolExecutor(workers) as pool:
        for qz in range(Z):
            found = np.flatnonzero(member[:, :, qz].reshape(-1, order='F'))
            if not found.size:
                continue
            sub = txy if found.size == X * Y else txy[:, found]

            def plane(pz, sub=sub, qz=qz):
                np.minimum(out[:, pz], (sub + tz[pz, qz]).min(axis=1), out=out[:, pz])
            list(pool.map(plane, range(Z)))
    return out.reshape((X, Y, Z), order='F')


def spacing_of(affine):
    return tuple(float(np.linalg.norm(np.asarray(affine, np.float64)[:3, a])) for a in range(3))


def brain_mask(values, spacing=(1.0, 1.0, 1.0), bins=256, erode_mm=5.0, dilate_mm=6.0, keep_holes=False):
    """fp32 values [X,Y,Z] -> (mask bool [X,Y,Z] or None where the inputs are left as they are, report, stages): tissue = the raw mask of
    volume_foreground_ref.foreground; eroded = tissue farther than erode_mm from its complement; core = the largest component of that;
    grown = tissue within dilate_mm of the core; plus the holes.  stages: tissue, eroded, core, grown."""
    v = np.asarray(values, np.float32)
    cand = F.candidates(v)
    report = dict(threshold=None, bin=None, bins=int(bins), lo=None, hi=None, candidates=int(cand.sum()),
                  spacing=[float(s) for s in spacing], erode_mm=float(erode_mm), dilate_mm=float(dilate_mm), tissue=0, eroded=0,
                  components=0, core=0, kept=0, filled=0, source=None)
    if not cand.any():
        return None, report, {}
    lo, hi = float(v[cand].min()), float(v[cand].max())
    report['lo'], report['hi'] = lo, hi
    if hi == lo:
        return None, report, {}
    scale = bins / (hi - lo)
    b = F.bin_of(v, lo, scale, bins)
    k = F.otsu(np.bincount(b[cand], minlength=bins))
    if k is None:
        return None, report, {}
    report['bin'], report['threshold'] = k, lo + (k + 1) / scale
    tissue = cand & (b > k)
    report['tissue'] = int(tissue.sum())
    eroded = edt2(tissue, 0, spacing) > float(erode_mm) * float(erode_mm)
    report['eroded'] = int(eroded.sum())
    stages = dict(tissue=tissue, eroded=eroded)
    if not eroded.any():
        return None, report, stages
    core, report['components'] = F.largest(eroded)
    report['core'] = int(core.sum())
    grown = (edt2(core, 1, spacing) <= float(dilate_mm) * float(dilate_mm)) & tissue
    final = grown if keep_holes else F.fill_holes(grown)
    report['filled'] = int(final.sum() - grown.sum())
    report['kept'] = int(final.sum())
    stages.update(core=core, grown=grown)
    return final, report, stages


# ---- the phantom --------------------------------------------------------------------------------------------------------------------------
def phantom(shape=PHANTOM_SHAPE, seed=11):
    """-> (fp32 [X,Y,Z] at 1 mm, labels uint8 [X,Y,Z] holding AIR .. BRIDGE).  A bright ellipsoid brain of semi-axes 14, 11, 9 about the
    centre (s - 1) / 2 with a dark ventricle (a sphere of radius 2.5) in its middle; around it a dark gap 3 voxels wide (0 < the distance
    to the brain <= 3) and a bright scalp shell 3 voxels thick (3 < the distance <= 6); one bright bridge of 2 x 2 voxels across the gap
    along +x; air that is exactly 0 and a little positive noise everywhere else."""
    X, Y, Z = shape
    x, y, z = np.meshgrid(np.arange(X, dtype=np.float64), np.arange(Y, dtype=np.float64), np.arange(Z, dtype=np.float64), indexing='ij')
    cx, cy, cz = (X - 1) / 2, (Y - 1) / 2, (Z - 1) / 2
    brain = ((x - cx) / 14.0) ** 2 + ((y - cy) / 11.0) ** 2 + ((z - cz) / 9.0) ** 2 <= 1.0
    away = edt2(brain, 1, (1.0, 1.0, 1.0))
    labels = np.full(shape, AIR, np.uint8)
    labels[brain] = BRAIN
    labels[(x - cx) ** 2 + (y - cy) ** 2 + (z - cz) ** 2 <= 2.5 ** 2] = VENTRICLE
    labels[(away > 0) & (away <= 9.0)] = GAP
    labels[(away > 9.0) & (away <= 36.0)] = SCALP
    labels[(labels == GAP) & (x > cx) & (np.abs(y - cy) < 1.0) & (np.abs(z - cz) < 1.0)] = BRIDGE
    clean = np.zeros(shape)
    clean[labels == BRAIN] = (500.0 + 100.0 * np.cos(x / 5.0) * np.sin(y / 4.0))[labels == BRAIN]
    clean[(labels == VENTRICLE) | (labels == GAP)] = 15.0
    clean[(labels == SCALP) | (labels == BRIDGE)] = 600.0
    noise = np.abs(np.random.default_rng(seed).normal(0.0, 5.0, shape))
    return np.where(labels != AIR, clean + noise, 0.0).astype(np.float32), labels


def properties(mask, labels, spacing, dilate_mm):
    """What the geometry of the phantom forces on a brain mask -> {name: bool}: no scalp and no air voxel in it, every ventricle voxel in
    it, the bridge cut (no bridge voxel of the mask farther than dilate_mm from the brain), the mask at least 2 voxel spacings (of the
    finest axis) short of the scalp, and most of the brain in it."""
    mask = np.asarray(mask, bool)
    brainish = (labels == BRAIN) | (labels == VENTRICLE)
    from_brain, from_scalp = edt2(brainish, 1, spacing), edt2(labels == SCALP, 1, spacing)
    return dict(no_scalp=not mask[labels == SCALP].any(), no_air=not mask[labels == AIR].any(), ventricle=bool(mask[labels == VENTRICLE].all()),
                bridge_cut=bool((from_brain[mask & (labels == BRIDGE)] <= dilate_mm * dilate_mm).all()) and not mask[labels == BRIDGE].all(),
                short_of_scalp=bool(from_scalp[mask].min() >= (2.0 * min(spacing)) ** 2),
                brain=float(mask[brainish].mean()) > 0.9)
