"""Non-local-means denoising of the inputs (--denoise; csrc/volume_denoise.hip).

Thermal noise in an input goes straight into the synthesised contrast, blurs the joint histogram of --coregister, widens the histogram
--bias_correct sharpens and inflates the z-score moments.  With --denoise every input is replaced by its 3D non-local-means estimate
on its own grid before any of those stages sees it:

    stored voxels --mud_volume_denoise_residual--> uint32 keys of the pseudo-residuals |eps|
    four times: mud_volume_denoise_select_hist --256 counts--> the host picks the bin of the lower median
    sigma = 1.4826 * median(|eps|)              (or --denoise_sigma)
    mud_volume_denoise_nlm --> fp32 [Z,Y,X], a volume like a regridded one, with the source's own geometry

All per-voxel work is the device's; the host sees 4 x 256 counts.  Counts are integers and the estimate accumulates in a fixed order:
two runs give the same bits.
"""
from __future__ import annotations

import json
import os

import numpy as np

from . import MudiffHipError
from .volume_intake import DEVICE_DTYPES, upload
from .volume_regrid import RegriddedVolume

MAX_SEARCH, MAX_PATCH = 5, 2
MAD_TO_SIGMA = 1.4826
DEFAULTS = dict(sigma=None, search=2, patch=1, beta=1.0, rician=False)


class DenoisedVolume(RegriddedVolume):
    """A RawVolume whose voxels live on the device (fp32 [Z,Y,X]) with the shape, affine and header of the volume it was made from."""


def check_options(sigma=None, search=2, patch=1, beta=1.0, rician=False):
    """ValueError (with the flag's name) for a value the kernels cannot run with."""
    if sigma is not None and not (np.isfinite(sigma) and sigma > 0):
        raise ValueError(f'--denoise_sigma must be finite and positive (got {sigma})')
    if not 1 <= int(search) <= MAX_SEARCH:
        raise ValueError(f'--denoise_search must be in [1, {MAX_SEARCH}] (got {search})')
    if not 1 <= int(patch) <= MAX_PATCH:
        raise ValueError(f'--denoise_patch must be in [1, {MAX_PATCH}] (got {patch})')
    if not (np.isfinite(beta) and beta > 0):
        raise ValueError(f'--denoise_beta must be finite and positive (got {beta})')


def select_lower_median(hist):
    """The exact lower median (rank (n - 1) // 2) of a set of uint32 keys by four passes of a 256-bin radix histogram, most significant
    byte first.  hist(prefix, which) -> the 256 counts of byte 3 - which over the keys whose `which` higher bytes equal prefix (the
    device's mud_volume_denoise_select_hist; numpy in the tests).  -> (key, n), key None for an empty set."""
    prefix, rank, n = 0, 0, 0
    for which in range(4):
        counts = np.asarray(hist(prefix, which)).astype(np.int64).reshape(-1)
        if counts.size != 256 or (counts < 0).any():
            raise MudiffHipError(f'radix select: pass {which} did not give 256 counts')
        if which == 0:
            n = int(counts.sum())
            if n == 0:
                return None, 0
            rank = (n - 1) // 2
        cum = np.cumsum(counts)
        b = int(np.searchsorted(cum, rank, side='right'))
        if b > 255:
            raise MudiffHipError(f'radix select: pass {which} holds {int(cum[-1])} keys, fewer than the rank {rank} left')
        rank -= int(cum[b - 1]) if b else 0
        prefix = (prefix << 8) | b
    return prefix, n


def sigma_of_key(key):
    """1.4826 x the fp32 whose bits the key is, in fp64."""
    return MAD_TO_SIGMA * float(np.array([int(key)], np.uint32).view(np.float32)[0])


def _meta(raw):
    if int(raw.code) not in DEVICE_DTYPES:
        raise MudiffHipError(f'denoise: unsupported NIfTI datatype code {raw.code}')
    return (int(raw.code), tuple(int(v) for v in raw.shape)) + tuple(float(v) for v in raw.scaling)


def estimate_sigma(raw, device, dev=None):
    """The noise level of a RawVolume from its pseudo-residuals -> (sigma, samples): 1.4826 x the lower median of |eps| over the voxels
    that are > 0 with six face neighbours inside the volume, valid and > 0; (0.0, 0) without such a voxel."""
    from . import ops
    if len(raw.shape) != 3:
        raise ValueError(f'denoise: expected a 3D volume, got shape {tuple(raw.shape)}')
    keys = ops.volume_denoise_residual(upload(raw, device) if dev is None else dev, *_meta(raw))
    key, n = select_lower_median(lambda prefix, which: ops.volume_denoise_select_hist(keys, prefix, which).cpu().numpy().view(np.uint32))
    return (0.0, 0) if key is None else (sigma_of_key(key), n)


def denoise(raw, device, sigma=None, search=2, patch=1, beta=1.0, rician=False):
    """A RawVolume (its voxels on the host, or on the device already) -> (DenoisedVolume, report).  report: sigma, estimated (bool),
    samples (the size of the estimation set; 0 with a given sigma), zeroed (nonzero voxels the Rician correction took to 0) and the
    options.  With nothing to estimate from, or an estimate that is not > 0, the input itself is returned and the report holds sigma 0."""
    from . import ops
    if len(raw.shape) != 3:
        raise ValueError(f'denoise: expected a 3D volume, got shape {tuple(raw.shape)}')
    check_options(sigma, search, patch, beta, rician)
    dev, meta = upload(raw, device), _meta(raw)
    report = dict(sigma=0.0, estimated=sigma is None, samples=0, zeroed=0, search=int(search), patch=int(patch), beta=float(beta),
                  rician=bool(rician))
    if sigma is None:
        sigma, report['samples'] = estimate_sigma(raw, device, dev)
        if not (np.isfinite(sigma) and sigma > 0):
            return raw, report
    report['sigma'] = float(sigma)
    out, zeroed = ops.volume_denoise_nlm(dev, *meta, int(search), int(patch), float(sigma), float(beta), bool(rician))
    report['zeroed'] = int(zeroed.cpu().numpy().view(np.uint32)[0])
    return DenoisedVolume(out, raw.shape, raw.affine, raw.header), report


# ---------------------------------------------------------------------------------------------------
# the pipeline's side
# ---------------------------------------------------------------------------------------------------
def denoise_suffix(reports):
    """What a [done] line gains under --denoise (nothing otherwise): ` | denoise=<name>,<name>,...`."""
    if not reports:
        return ''
    return ' | denoise=' + ','.join(str(r[0]) for r in reports)


def write_reports(reports, output_dir, target):
    """denoise_<t>.json next to the prediction: {input name: report}.  -> its path."""
    os.makedirs(output_dir, exist_ok=True)
    path = os.path.join(output_dir, f'denoise_{target.lower()}.json')
    with open(path, 'w') as f:
        json.dump({r[0]: r[1] for r in reports}, f, indent=1)
    return path
