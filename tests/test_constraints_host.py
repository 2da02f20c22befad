"""Host: what the three known-target modes share (mudiff_hip.constraints): the batching that the one keyed loop
of volume.predict_slices and of ensemble.sample_ensemble rests on, the planning of an ensemble's chunks, and the refusals that come
before any device work."""
import argparse

import numpy as np
import pytest
import torch

from mudiff_hip import constraints as C
from mudiff_hip import thick as TK


def _thick(n, starts, L=3):
    """A ThickMeasurement of n thin slices with measured slabs of L from `starts` (host tensors: nothing here runs a kernel)."""
    w = np.full(L, 1.0 / L, np.float32)
    return TK.ThickMeasurement(torch.zeros(len(starts), 2, 2), starts, n, w, dict(slabs=[]), 1, dict(interp=False))


@pytest.mark.parametrize('n,B', [(1, 1), (5, 2), (6, 3), (7, 32)])
def test_batches_of_single_slices_are_the_ranges(n, B):
    """The identity the merged loop rests on: one-item units give exactly the ranges range(0, n, B) gave."""
    assert C.batches([[i] for i in range(n)], B) == [list(range(lo, min(lo + B, n))) for lo in range(0, n, B)]
    assert C.FREE.units(0, n) == [[i] for i in range(n)]
    assert TK.batches is C.batches


def test_batches_of_free_slices_and_slabs():
    m = _thick(7, [1, 4])
    assert m.units(0, 7) == [[0], [1, 2, 3], [4, 5, 6]]
    assert C.batches(m.units(0, 7), 4) == [[0, 1, 2, 3], [4, 5, 6]]
    with pytest.raises(ValueError, match='--batch_size 2 '):
        C.batches(m.units(0, 7), 2)


def _chunks(con, n, chunk):
    out, s0 = [], 0
    while s0 < n:
        s1 = con.chunk_end(s0, min(s0 + chunk, n))
        out.append((s0, s1))
        s0 = s1
    return out


def test_chunk_end():
    m = _thick(8, [1, 5])
    assert _chunks(m, 8, 3) == [(0, 1), (1, 4), (4, 5), (5, 8)]             # chunks 0, 1..3, 4, 5..7
    assert _chunks(m, 8, 8) == [(0, 8)]
    with pytest.raises(ValueError, match='chunk'):
        _chunks(m, 8, 2)
    assert _chunks(C.FREE, 8, 3) == [(0, 3), (3, 6), (6, 8)]        # the default: a chunk ends where it would


MODES = dict(known=(None, None), kspace=object(), thick=object())


@pytest.mark.parametrize('pair', [('known', 'kspace'), ('known', 'thick'), ('kspace', 'thick')])
def test_two_modes_are_refused_before_any_device_work(pair):
    from mudiff_hip import ensemble as E
    from mudiff_hip import volume as V
    args = argparse.Namespace(image_size=16, num_timesteps=4, nz=100)
    stacks = [np.zeros((2, 16, 16), np.float32)] * 3
    two = {k: MODES[k] for k in pair}
    with pytest.raises(ValueError, match='exclusive'):
        V.predict_slices(args, None, None, stacks, 'cpu', seed=1, **two)
    with pytest.raises(ValueError, match='exclusive'):
        E.sample_ensemble(args, None, None, (None, None, None), 2, 1, **two)


@pytest.mark.parametrize('mode', sorted(MODES))
def test_a_mode_needs_a_seed_and_the_captured_sampler(mode):
    from mudiff_hip import volume as V
    args = argparse.Namespace(image_size=16, num_timesteps=4, nz=100)
    stacks = [np.zeros((2, 16, 16), np.float32)] * 3
    for kw, msg in ((dict(seed=None), 'needs a seed'), (dict(seed=1, use_graph=False), 'captured sampler'),
                    (dict(seed=1, x_inits=torch.zeros(2, 1, 16, 16)), 'injected')):
        with pytest.raises(ValueError, match=msg):
            V.predict_slices(args, None, None, stacks, 'cpu', **{mode: MODES[mode]}, **kw)
