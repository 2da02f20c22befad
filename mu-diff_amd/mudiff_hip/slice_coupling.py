"""Slice-coupled sampling noise: the volume pipeline's --slice_coupling.

mudiff_hip.volume and mudiff_hip.cohort sample every axial slice of a volume as its own 2D draw, so neighbouring planes of the written
volume share no stochastic choice: the stripes of slice-wise synthesis in sagittal and coronal reformats.  Here the Gaussian draws of
neighbouring slices are correlated along z while every slice stays an exact sample of the model:

    draw(slice s) = sum_{j=-R..R} w_|j| * eta(s + j),      eta(.) the keyed white noise of ops.randn_keyed,      sum_j w_j^2 = 1

A sum of independent N(0, 1) variables with weights of unit square sum is N(0, 1): each slice's x_init, z and posterior noise are marginally
what the sampler expects (elements of one slice stay independent of each other, as they come from different Philox lanes).  Two slices d
apart correlate by coupling_correlation(sigma, d) = sum_j w_j w_{j+d}, about exp(-d^2 / (4 sigma^2)), and not at all for d > 2 R.  The keyed
generator makes it cheap: a draw is a pure function of its key, so a slice reads its neighbours' white noise without pre-drawing anything
and the result does not depend on batch size, chunking or sharding (ops.randn_keyed_coupled).

`coupling`, as GraphSampler.sample_keyed, ensemble.sample_ensemble and volume.predict_slices take it: None (independent slices), 'shared'
(every slice of a volume draws with slice key 0: identical draws, the limit sigma -> infinity) or (half_taps, R) from coupling_taps.

No trained checkpoint was available when this was written: how much it helps on real weights is unmeasured and the choice of sigma untuned.
"""
from __future__ import annotations

import math

import numpy as np

MAX_SIGMA = 10.0          # R = ceil(3 sigma) <= 30 stays within the kernel's MUD_COUPLING_MAX_RADIUS
MAX_RADIUS = 32
SHARED = 'shared'


def check_sigma(sigma, flag='--slice_coupling'):
    """-> float(sigma), ValueError naming `flag` unless 0 < sigma <= MAX_SIGMA."""
    try:
        s = float(sigma)
    except (TypeError, ValueError):
        raise ValueError(f"{flag} takes a positive number (sigma, in slices) or 'shared', got {sigma!r}") from None
    if not (math.isfinite(s) and 0.0 < s <= MAX_SIGMA):
        raise ValueError(f'{flag}: sigma must lie in (0, {MAX_SIGMA:g}], got {sigma}')
    return s


def coupling_taps(sigma):
    """-> (half_taps, R): R = ceil(3 sigma) and the fp64 weights w_0..w_R, w_j proportional to exp(-j^2 / (2 sigma^2)), normalised so that
    the square sum over j = -R..R is 1."""
    s = check_sigma(sigma, 'coupling_taps')
    R = int(math.ceil(3.0 * s))
    j = np.arange(R + 1, dtype=np.float64)
    w = np.exp(-(j * j) / (2.0 * s * s))
    w = w / math.sqrt(float(w[0] * w[0] + 2.0 * np.sum(w[1:] * w[1:])))
    return w, R


def coupling_correlation(sigma, lag):
    """The correlation of the draws of two slices `lag` apart: sum_j w_j w_{j+lag} over the taps of coupling_taps(sigma); exactly 0 for
    |lag| > 2 R."""
    w, R = coupling_taps(sigma)
    lag = abs(int(lag))
    if lag > 2 * R:
        return 0.0
    full = np.concatenate([w[:0:-1], w])                   # j = -R..R
    return float(np.sum(full[:full.size - lag] * full[lag:]))


def parse_flag(text):
    """--slice_coupling's value -> None (absent), 'shared' or sigma as a float; ValueError naming the flag otherwise."""
    if text is None:
        return None
    if isinstance(text, str) and text.strip().lower() == SHARED:
        return SHARED
    return check_sigma(text)


def coupling_from_flag(value):
    """parse_flag's result -> the `coupling` of the samplers: None, 'shared' or (half_taps, R)."""
    value = parse_flag(value)
    return value if value in (None, SHARED) else coupling_taps(value)


def check_coupling(coupling):
    """-> None, 'shared' or (contiguous fp64 half taps, R); ValueError for anything else."""
    if coupling is None or (isinstance(coupling, str) and coupling == SHARED):
        return coupling
    try:
        half, R = coupling
        half, R = np.ascontiguousarray(half, dtype=np.float64).reshape(-1), int(R)
    except (TypeError, ValueError):
        raise ValueError(f"coupling must be None, 'shared' or (half_taps, R), got {coupling!r}") from None
    if not 0 <= R <= MAX_RADIUS or half.size != R + 1 or not np.isfinite(half).all():
        raise ValueError(f'coupling: need R + 1 finite half taps with R in [0, {MAX_RADIUS}], got {half.size} taps and R = {R}')
    return half, R


def suffix(value):
    """What a [done] line gains under --slice_coupling (nothing without it)."""
    value = parse_flag(value)
    return '' if value is None else f' | slice_coupling={value if value == SHARED else format(value, "g")}'


def add_flags(p):
    p = p.later() if hasattr(p, 'later') else p          # volume.VolumeParser: the main option list and `late`'s are pinned, later flags go here
    p.add_argument('--slice_coupling', type=str, default=None, metavar='SIGMA|shared',
                   help='correlate the Gaussian draws of neighbouring slices along z (mudiff_hip.slice_coupling): every draw of slice s is '
                        'the keyed white noise of the slices s-R..s+R under Gaussian weights of width SIGMA slices (0 < SIGMA <= 10, '
                        "R = ceil(3 SIGMA)) and unit square sum, so each slice stays an exact sample of the model; 'shared' gives every "
                        'slice of a volume the same draws.  It switches the single-sample path from the torch generator\'s draws to keyed '
                        'draws (as --num_samples uses), so the volume differs from the default run of the same --seed.  The benefit on '
                        'trained weights is unmeasured and SIGMA untuned')
    p.add_argument('--through_plane', action='store_true',
                   help='measure the through-plane roughness of the written prediction on the GPU (mudiff_hip.volume_through_plane): mean '
                        '|dV/dz|, |d2V/dz2|, the in-plane analogues and their ratio over the slab, for --gt_volume too when given; writes '
                        'through_plane_<t>.json next to the prediction and prints one [through-plane] line')
