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

import numpy as np

from . import MudiffHipError
from .volume_intake import upload, write_report_json
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


def estimate_sigma(raw, device, dev=None):
    """The noise level of a RawVolume from its pseudo-residuals -> (sigma, samples): 1.4826 x the lower median of |eps| over the voxels
    that are > 0 with six face neighbours inside the volume, valid and > 0; (0.0, 0) without such a voxel."""
    from . import ops
    if len(raw.shape) != 3:
        raise ValueError(f'denoise: expected a 3D volume, got shape {tuple(raw.shape)}')
    keys = ops.volume_denoise_residual(upload(raw, device) if dev is None else dev, *raw.kernel_meta('denoise'))
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
    dev, meta = upload(raw, device), raw.kernel_meta('denoise')
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
def add_flags(p):
    p.add_argument('--denoise', action='store_true',
                   help='replace every input by its 3D non-local-means estimate on its own grid (patch-similarity weighted mean over a '
                        'search window, on the GPU: mudiff_hip.volume_denoise) before --coregister / --regrid / --bias_correct see it; '
                        'denoise_<t>.json next to the prediction holds the noise level that was used.  --gt_volume / --eval_mask are '
                        'not denoised')
    p.add_argument('--denoise_sigma', type=float, default=DEFAULTS['sigma'],
                   help='the noise standard deviation, in stored intensity units (default: estimated per input from pseudo-residuals)')
    p.add_argument('--denoise_search', type=int, default=DEFAULTS['search'], help='search radius: candidates within this many voxels per axis (1 to 5)')
    p.add_argument('--denoise_patch', type=int, default=DEFAULTS['patch'], help='patch radius: patches of (2 r + 1)^3 voxels are compared (1 to 2)')
    p.add_argument('--denoise_beta', type=float, default=DEFAULTS['beta'], help='smoothing strength: the weights fall off with 2 beta sigma^2')
    p.add_argument('--denoise_rician', action='store_true',
                   help='with --denoise: average squared intensities and subtract the Rician bias 2 sigma^2 (magnitude images)')


def options_from(args):
    """A namespace's --denoise_* flags (any may be missing) -> IntakeOptions' `denoise`: the keyword arguments of denoise, or None
    without --denoise.  ValueError, naming the flag, for a value check_options refuses."""
    get = lambda k: getattr(args, 'denoise_' + k, DEFAULTS[k])      # noqa: E731
    kw = dict(sigma=None if get('sigma') is None else float(get('sigma')), search=int(get('search')), patch=int(get('patch')),
              beta=float(get('beta')), rician=bool(get('rician')))
    check_options(**kw)
    return dict(denoise=kw if getattr(args, 'denoise', False) else None)


def denoise_suffix(reports):
    """What a [done] line gains under --denoise (nothing otherwise): ` | denoise=<name>,<name>,...`."""
    if not reports:
        return ''
    return ' | denoise=' + ','.join(str(r[0]) for r in reports)


def write_reports(reports, output_dir, target):
    """denoise_<t>.json next to the prediction: {input name: report}.  -> its path."""
    return write_report_json('denoise', {r[0]: r[1] for r in reports}, output_dir, target)
