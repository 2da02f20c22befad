"""Records what the reference itself computes for the training normalisation -> tests/golden/zscore.npz.

    python tests/golden/make_zscore_golden.py --reference /path/to/the/reference/checkout

For a handful of small seeded volumes the script calls the reference's own `normalize_volume` (tools/pre_process.py) on the fp32 values,
as tools/pre_process.py does with get_fdata(dtype=float32), and then applies the dataset's clamp line (dataset/dataset_brats.py:83,
`torch.clamp(t, -3.0, 3.0) / 3.0`) with torch on the CPU.  Only arrays are stored: per volume `in_<name>` (the voxels in their stored
dtype), `z_<name>` (normalize_volume's output: what the .npy files of the 2D pipeline hold) and `out_<name>` (after the clamp line).

tools/pre_process.py imports nibabel at module level.  Where nibabel is not installed the module cannot be imported, so the function is
loaded alone: its `def` is cut out of the parsed source (ast) and executed in a namespace that holds numpy and a logger - the two names
it uses.  Nothing of the reference's text is copied into this repository either way."""
import argparse
import ast
import logging
import os
import sys

import numpy as np
import torch

SHAPE = (24, 20, 12)


def load_normalize_volume(reference):
    path = os.path.join(reference, 'tools', 'pre_process.py')
    try:
        import nibabel  # noqa: F401
        sys.path.insert(0, os.path.join(reference, 'tools'))
        from pre_process import normalize_volume
        return normalize_volume
    except ImportError:
        pass
    with open(path) as f:
        tree = ast.parse(f.read(), path)
    fn = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == 'normalize_volume']
    assert len(fn) == 1, f'{path}: normalize_volume not found'
    ns = dict(np=np, logger=logging.getLogger('pre_process'))
    exec(compile(ast.Module(body=fn, type_ignores=[]), path, 'exec'), ns)
    return ns['normalize_volume']


def volumes():
    """name -> [X,Y,Z] array in its stored dtype."""
    rng = np.random.default_rng(511)
    X, Y, Z = SHAPE
    x, y, z = np.meshgrid(np.linspace(-1, 1, X), np.linspace(-1, 1, Y), np.linspace(-1, 1, Z), indexing='ij')
    inside = (x / 0.8) ** 2 + (y / 0.75) ** 2 + (z / 0.9) ** 2 < 1
    out = {}
    out['i2_ties'] = np.where(inside, rng.integers(1, 40, SHAPE), 0).astype(np.int16)              # many voxels per level, zero background
    out['f4_noise'] = (rng.standard_normal(SHAPE) * 300 + 500).astype(np.float32) * inside         # tails beyond 3 sigma get clamped
    out['f4_outliers'] = out['f4_noise'].copy()
    out['f4_outliers'][5, 5, 5], out['f4_outliers'][6, 7, 3] = 2.5e4, -1.0e4
    out['zeros'] = np.zeros(SHAPE, np.int16)                                                       # empty mask: mean 0, std 1
    out['constant'] = np.where(inside, 7, 0).astype(np.int16)                                      # std == 0 -> 1
    out['nan'] = out['f4_noise'].copy()
    out['nan'][3, 4, 5] = np.nan                                                                   # both moments NaN: all NaN
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', required=True, help='checkout of the reference (holds tools/pre_process.py)')
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.abspath(__file__)), 'zscore.npz'))
    a = ap.parse_args()
    normalize_volume = load_normalize_volume(a.reference)
    arrays = {}
    for name, vol in volumes().items():
        with np.errstate(all='ignore'):
            z = normalize_volume(vol.astype(np.float32))
        assert z.dtype == np.float32 and z.shape == vol.shape
        out = (torch.clamp(torch.from_numpy(np.ascontiguousarray(z)), -3.0, 3.0) / 3.0).numpy()
        arrays['in_' + name], arrays['z_' + name], arrays['out_' + name] = vol, z, out
    np.savez_compressed(a.out, **arrays)
    print(f'wrote {a.out}: {sorted(volumes())}')


if __name__ == '__main__':
    main()
