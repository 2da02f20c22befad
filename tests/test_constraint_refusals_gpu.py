"""GPU: what the checked wrappers of the known-target constraints refuse, word for word, and what they accept, bit for bit
(ops.known_constrain, kspace_constrain, slab_constrain, slab_kspace_constrain, band_constrain; ops.fft2, slab_average, band_measure;
the `check` of constraints.KnownRows, KSpaceRows, SlabRows, SlabKSpaceRows and thick_volume.BandMeasurement.check_volume).  DESIGN.md
section 5.24a.

Every refusal is raised in Python before anything is launched.  An accepted call is compared with the unchecked `*_into` launcher on
operands prepared by hand: with out=None, with out = x_new and with an x_new that is not contiguous; with keys, with injected noise and
clean.  Shapes: the smallest the kernels take - S = 16, 4 rows, 2 groups of L = 2, a band matrix of 2 thick over 4 thin slices; the
wrappers that are not bound to k-space get rows of 3 x 5 = 15 elements, so the quads' element-by-element tail runs."""
import functools
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
S, ROWS, GROUPS = 16, 4, 2
MEMBERS, WEIGHTS = [[0, 1], [2, 3]], [0.25, 0.75]
BAND_A = np.array([[0.5, 0.5, 0.0, 0.0], [0.0, 0.25, 0.5, 0.25]])
SEED, STEP = 0x0123456789ABCDEF, 3
GPU_ONLY = 'the MU-Diff HIP path needs tensors on an MI355X (got a CPU tensor); there is no CPU fallback'
LEVEL = '{}: need t (int64 [rows]) and two tables of one length'


@functools.lru_cache(maxsize=None)
def _o():
    """The operands, made once and never written: x3 [4,16,16], x4 [4,1,16,16], xr [4,3,5] and what goes with each."""
    from mudiff_hip import ops
    g = torch.Generator().manual_seed(5)
    rn = lambda *shape: torch.randn(*shape, generator=g).to(DEV)      # noqa: E731
    o = types.SimpleNamespace()
    o.x3, o.x4, o.xr, o.xb = rn(ROWS, S, S), rn(ROWS, 1, S, S), rn(ROWS, 3, 5), rn(1, ROWS, 3, 5)
    o.n3, o.n4, o.nr, o.nb = rn(ROWS, S, S), rn(ROWS, 1, S, S), rn(ROWS, 3, 5), rn(1, ROWS, 3, 5)
    o.known, o.kmask = rn(ROWS, 3, 5), (torch.rand(ROWS, 3, 5, generator=g) < 0.5).to(torch.uint8).to(DEV)
    o.yk, o.yg = torch.complex(rn(ROWS, S, S), rn(ROWS, S, S)), torch.complex(rn(GROUPS, S, S), rn(GROUPS, S, S))
    o.m1 = (torch.rand(1, S, S, generator=g) < 0.4).to(torch.uint8).to(DEV)
    o.mrows = (torch.rand(ROWS, S, S, generator=g) < 0.4).to(torch.uint8).to(DEV)
    o.ys, o.ys3, o.yb = rn(GROUPS, 3, 5), rn(GROUPS, S, S), rn(2, 3, 5)
    o.t = torch.tensor([1, 4, 2, 0], dtype=torch.int64, device=DEV)
    a = torch.tensor([0.99999994, 0.97, 0.81, 0.5, 0.12], dtype=torch.float64)
    o.a_tab, o.s_tab = a.float().to(DEV), torch.sqrt(1 - a * a).float().to(DEV)
    o.keys = torch.tensor([[40, 0], [41, 0], [7, 3], [8, 3]], dtype=torch.int64)
    o.kd = o.keys.to(DEV)
    o.tab, o.band = ops.slab_tables(MEMBERS, WEIGHTS), ops.band_tables(BAND_A)
    o.lv = (o.t, 0, o.a_tab, o.s_tab)
    return o


def _sampler(H=S, W=S):
    o = _o()
    return types.SimpleNamespace(B=ROWS, H=H, W=W, x=torch.empty(ROWS, 1, H, W, device=DEV), t=o.t,
                                 _diffusion_tables=lambda: (o.a_tab, o.s_tab, None, None))


def _band_measurement(y):
    from mudiff_hip.thick_volume import BandMeasurement
    return BandMeasurement(y, BAND_A)


def _ops():
    from mudiff_hip import ops
    return ops


def _rows(name, *fields):
    from mudiff_hip import constraints
    return getattr(constraints, name)(*fields)


# (what is called with the operands o and ops, the whole message)
REFUSALS = [
    # ops.known_constrain
    (lambda o, p: p.known_constrain(o.xr.cpu(), o.known, o.kmask, *o.lv, keys=o.keys), GPU_ONLY),
    (lambda o, p: p.known_constrain(o.xr, o.known.half(), o.kmask, *o.lv, keys=o.keys),
     'known_constrain: known must be a non-empty fp32 [rows, ...] tensor, got torch.float16 (4, 3, 5)'),
    (lambda o, p: p.known_constrain(o.xr.flatten(1), o.known, o.kmask, *o.lv, keys=o.keys),
     'known_constrain: x_new must be torch.float32 of shape (4, 3, 5), got torch.float32 (4, 15)'),
    (lambda o, p: p.known_constrain(o.xr, o.known, o.kmask.float(), *o.lv, keys=o.keys),
     'known_constrain: mask must be torch.uint8 of shape (4, 3, 5), got torch.float32 (4, 3, 5)'),
    (lambda o, p: p.known_constrain(o.xr, o.known, o.kmask, *o.lv, noise=o.nr.double()),
     'known_constrain: noise must be torch.float32 of shape (4, 3, 5), got torch.float64 (4, 3, 5)'),
    (lambda o, p: p.known_constrain(o.xr, o.known, o.kmask, *o.lv, keys=o.keys, out=torch.empty(ROWS, 5, 3, device=DEV)),
     'known_constrain: out must be torch.float32 of shape (4, 3, 5), got torch.float32 (4, 5, 3)'),
    (lambda o, p: p.known_constrain(None, o.known, o.kmask, *o.lv, keys=o.keys), 'known_constrain: x_new may be None only without a mask'),
    (lambda o, p: p.known_constrain(o.xr, o.known, o.kmask, *o.lv, keys=o.keys, out=torch.empty(ROWS, 5, 3, device=DEV).transpose(1, 2)),
     'known_constrain: out must be contiguous'),
    (lambda o, p: p.known_constrain(o.xr, o.known, o.kmask, o.t.int(), 0, o.a_tab, o.s_tab, keys=o.keys), LEVEL.format('known_constrain')),
    (lambda o, p: p.known_constrain(o.xr, o.known, o.kmask, None, 0, o.a_tab, o.s_tab, keys=o.keys), LEVEL.format('known_constrain')),
    (lambda o, p: p.known_constrain(o.xr, o.known, o.kmask, o.t, 0, o.a_tab, o.s_tab[:4], keys=o.keys), LEVEL.format('known_constrain')),
    (lambda o, p: p.known_constrain(o.xr, o.known, o.kmask, *o.lv), 'known_constrain: pass noise or keys'),
    (lambda o, p: p.known_constrain(o.xr, o.known, o.kmask, *o.lv, keys=o.keys[:3]), 'known_constrain: 3 keys for 4 rows'),
    (lambda o, p: p.known_constrain(o.xr, o.known, o.kmask, *o.lv, keys=torch.zeros(4, 3, dtype=torch.int64)),
     'randn_keyed: keys must be [rows, 2] = (slice, sample), got (4, 3)'),
    (lambda o, p: p.known_constrain(o.xr, o.known, o.kmask, *o.lv, keys=[[0, 0], [-1, 0], [2, 0], [3, 0]]), 'randn_keyed: slice indices must be >= 0'),
    (lambda o, p: p.known_constrain(o.xr, o.known, o.kmask, *o.lv, keys=[[0, 0], [1, 1 << 31], [2, 0], [3, 0]]),
     'randn_keyed: sample indices must lie in [0, 2^31)'),
    (lambda o, p: p.known_constrain(o.xr, o.known, o.kmask, *o.lv, keys=o.keys, seed=-1), 'randn_keyed: seed must lie in [0, 2^64), got -1'),
    # two faults: the operands before the level, the level before the seed
    (lambda o, p: p.known_constrain(o.xr, o.known, o.kmask.float(), None, 0, None, None, keys=o.keys, seed=-1),
     'known_constrain: mask must be torch.uint8 of shape (4, 3, 5), got torch.float32 (4, 3, 5)'),
    (lambda o, p: p.known_constrain(o.xr, o.known, o.kmask, *o.lv, seed=-1), 'known_constrain: pass noise or keys'),

    # ops.kspace_constrain
    (lambda o, p: p.kspace_constrain(o.x3, o.yk.cpu(), o.m1, *o.lv, keys=o.keys), GPU_ONLY),
    (lambda o, p: p.kspace_constrain(o.x4.expand(ROWS, 2, S, S), o.yk, o.m1, *o.lv, keys=o.keys),
     'kspace_constrain: x_new must be fp32 [rows, S, S] or [rows, 1, S, S], got torch.float32 (4, 2, 16, 16)'),
    (lambda o, p: p.kspace_constrain(o.x3[:, :, :8], o.yk, o.m1, *o.lv, keys=o.keys),
     'kspace_constrain: x_new must be fp32 [rows, S, S] or [rows, 1, S, S], got torch.float32 (4, 16, 8)'),
    (lambda o, p: p.kspace_constrain(o.x3[:, :8, :8], o.yk, o.m1, *o.lv, keys=o.keys), 'kspace_constrain: S must be a power of two in [16, 512], got 8'),
    (lambda o, p: p.kspace_constrain(o.x3, None, o.m1, *o.lv, keys=o.keys), 'kspace_constrain: y must be complex64 (4, 16, 16), got None'),
    (lambda o, p: p.kspace_constrain(o.x3, o.yk.real, o.m1, *o.lv, keys=o.keys),
     'kspace_constrain: y must be complex64 (4, 16, 16), got (torch.float32, (4, 16, 16))'),
    (lambda o, p: p.kspace_constrain(o.x3, o.yk, None, *o.lv, keys=o.keys), 'kspace_constrain: mask must be uint8 [1 or 4, 16, 16], got None'),
    (lambda o, p: p.kspace_constrain(o.x3, o.yk, o.mrows[:2], *o.lv, keys=o.keys),
     'kspace_constrain: mask must be uint8 [1 or 4, 16, 16], got (torch.uint8, (2, 16, 16))'),
    (lambda o, p: p.kspace_constrain(o.x3, o.yk, o.m1, *o.lv, noise=o.n4),
     'kspace_constrain: noise must be fp32 of shape (4, 16, 16), got torch.float32 (4, 1, 16, 16)'),
    (lambda o, p: p.kspace_constrain(o.x4, o.yk, o.m1, *o.lv, keys=o.keys, out=torch.empty(ROWS, 1, S, S, device=DEV, dtype=torch.float64)),
     'kspace_constrain: out must be fp32 of shape (4, 1, 16, 16), got torch.float64 (4, 1, 16, 16)'),
    (lambda o, p: p.kspace_constrain(o.x3, o.yk, o.m1, *o.lv, keys=o.keys, out=torch.empty(ROWS, S, S, device=DEV).transpose(1, 2)),
     'kspace_constrain: out must be contiguous'),
    (lambda o, p: p.kspace_constrain(o.x3, o.yk, o.m1, *o.lv, keys=o.keys, work=torch.empty_like(o.yg)),
     'kspace_constrain: work must be a contiguous complex64 (4, 16, 16), got torch.complex64 (2, 16, 16)'),
    (lambda o, p: p.kspace_constrain(o.x3, o.yk, o.m1, *o.lv, keys=o.keys, work=torch.empty_like(o.yk).transpose(1, 2)),
     'kspace_constrain: work must be a contiguous complex64 (4, 16, 16), got torch.complex64 (4, 16, 16)'),
    (lambda o, p: p.kspace_constrain(o.x3, o.yk, o.m1, o.t[:3], 0, o.a_tab, o.s_tab, keys=o.keys), LEVEL.format('kspace_constrain')),
    (lambda o, p: p.kspace_constrain(o.x3, o.yk, o.m1, *o.lv), 'kspace_constrain: pass noise or keys'),
    (lambda o, p: p.kspace_constrain(o.x3, o.yk, o.m1, *o.lv, keys=o.keys[:2]), 'kspace_constrain: 2 keys for 4 rows'),
    # two faults: the grid before y, y before the mask, out before work
    (lambda o, p: p.kspace_constrain(o.x3[:, :8, :8], None, None, *o.lv, keys=o.keys), 'kspace_constrain: S must be a power of two in [16, 512], got 8'),
    (lambda o, p: p.kspace_constrain(o.x3, None, None, *o.lv, keys=o.keys), 'kspace_constrain: y must be complex64 (4, 16, 16), got None'),
    (lambda o, p: p.kspace_constrain(o.x3, o.yk, o.m1, *o.lv, keys=o.keys, out=o.x4, work=torch.empty_like(o.yg)),
     'kspace_constrain: out must be fp32 of shape (4, 16, 16), got torch.float32 (4, 1, 16, 16)'),

    # ops.slab_constrain (and ops.slab_tables through it)
    (lambda o, p: p.slab_constrain(o.xr, o.ys.cpu(), MEMBERS, WEIGHTS, *o.lv, keys=o.keys), GPU_ONLY),
    (lambda o, p: p.slab_constrain(o.xr.half(), o.ys, MEMBERS, WEIGHTS, *o.lv, keys=o.keys),
     'slab_constrain: x_new must be a non-empty fp32 [rows, ...] tensor, got torch.float16 (4, 3, 5)'),
    (lambda o, p: p.slab_constrain(o.xr[:, :0], o.ys, MEMBERS, WEIGHTS, *o.lv, keys=o.keys),
     'slab_constrain: x_new must be a non-empty fp32 [rows, ...] tensor, got torch.float32 (4, 0, 5)'),
    (lambda o, p: p.slab_constrain(o.xr, o.ys, np.zeros((2, 0), np.int32), WEIGHTS, *o.lv, keys=o.keys),
     'slab_tables: members must be [groups, L] with L >= 1, got (2, 0)'),
    (lambda o, p: p.slab_constrain(o.xr, o.ys, MEMBERS, [0.5, 0.25, 0.25], *o.lv, keys=o.keys), 'slab_tables: weights must be [L] or (2, 2), got (3,)'),
    (lambda o, p: p.slab_constrain(o.xr, o.ys, MEMBERS, WEIGHTS, *o.lv, keys=o.keys, gains=[1.0, 1.0, 1.0]),
     'slab_tables: gains must be [L] or (2, 2), got (3,)'),
    (lambda o, p: p.slab_constrain(o.xr, None, MEMBERS, WEIGHTS, *o.lv, keys=o.keys), 'slab_constrain: y must be fp32 [2, 15], got None'),
    (lambda o, p: p.slab_constrain(o.xr, o.ys3, MEMBERS, WEIGHTS, *o.lv, keys=o.keys),
     'slab_constrain: y must be fp32 [2, 15], got (torch.float32, (2, 16, 16))'),
    (lambda o, p: p.slab_constrain(o.xr, o.ys, MEMBERS, WEIGHTS, *o.lv, noise=o.nr[:3]),
     'slab_constrain: noise must be fp32 of shape (4, 3, 5), got torch.float32 (3, 3, 5)'),
    (lambda o, p: p.slab_constrain(o.xr, o.ys, MEMBERS, WEIGHTS, *o.lv, keys=o.keys, out=o.xr.half()),
     'slab_constrain: out must be fp32 of shape (4, 3, 5), got torch.float16 (4, 3, 5)'),
    (lambda o, p: p.slab_constrain(o.xr, o.ys, MEMBERS, WEIGHTS, *o.lv, keys=o.keys, out=torch.empty(ROWS, 5, 3, device=DEV).transpose(1, 2)),
     'slab_constrain: out must be contiguous'),
    (lambda o, p: p.slab_constrain(o.xr, o.ys, MEMBERS, WEIGHTS, o.t, 0, None, o.s_tab, keys=o.keys), LEVEL.format('slab_constrain')),
    (lambda o, p: p.slab_constrain(o.xr, o.ys, MEMBERS, WEIGHTS, *o.lv), 'slab_constrain: pass noise or keys'),
    (lambda o, p: p.slab_constrain(o.xr, o.ys, MEMBERS, WEIGHTS, *o.lv, keys=o.keys[:1]), 'slab_constrain: 1 keys for 4 rows'),
    # two faults: x_new before the tables, the tables before y
    (lambda o, p: p.slab_constrain(o.xr.half(), o.ys, MEMBERS, [0.5, 0.25, 0.25], *o.lv, keys=o.keys),
     'slab_constrain: x_new must be a non-empty fp32 [rows, ...] tensor, got torch.float16 (4, 3, 5)'),
    (lambda o, p: p.slab_constrain(o.xr, None, MEMBERS, [0.5, 0.25, 0.25], *o.lv, keys=o.keys), 'slab_tables: weights must be [L] or (2, 2), got (3,)'),

    # ops.slab_kspace_constrain
    (lambda o, p: p.slab_kspace_constrain(o.x3, o.yg, o.m1.cpu(), MEMBERS, WEIGHTS, *o.lv, keys=o.keys), GPU_ONLY),
    (lambda o, p: p.slab_kspace_constrain(o.x3.double(), o.yg, o.m1, MEMBERS, WEIGHTS, *o.lv, keys=o.keys),
     'slab_kspace_constrain: x_new must be fp32 [rows, S, S] or [rows, 1, S, S], got torch.float64 (4, 16, 16)'),
    (lambda o, p: p.slab_kspace_constrain(o.x3[:, :8, :8], o.yg, o.m1, MEMBERS, WEIGHTS, *o.lv, keys=o.keys),
     'slab_kspace_constrain: S must be a power of two in [16, 512], got 8'),
    (lambda o, p: p.slab_kspace_constrain(o.x3, None, o.m1, MEMBERS, WEIGHTS, *o.lv, keys=o.keys),
     'slab_kspace_constrain: y must be complex64 (2, 16, 16), got None'),
    (lambda o, p: p.slab_kspace_constrain(o.x3, o.yk, o.m1, MEMBERS, WEIGHTS, *o.lv, keys=o.keys),
     'slab_kspace_constrain: y must be complex64 (2, 16, 16), got (torch.complex64, (4, 16, 16))'),
    (lambda o, p: p.slab_kspace_constrain(o.x3, o.yg, None, MEMBERS, WEIGHTS, *o.lv, keys=o.keys),
     'slab_kspace_constrain: mask must be uint8 [1 or 2, 16, 16], got None'),
    (lambda o, p: p.slab_kspace_constrain(o.x3, o.yg, o.mrows, MEMBERS, WEIGHTS, *o.lv, keys=o.keys),
     'slab_kspace_constrain: mask must be uint8 [1 or 2, 16, 16], got (torch.uint8, (4, 16, 16))'),
    (lambda o, p: p.slab_kspace_constrain(o.x4, o.yg, o.m1, MEMBERS, WEIGHTS, *o.lv, noise=o.n3),
     'slab_kspace_constrain: noise must be fp32 of shape (4, 1, 16, 16), got torch.float32 (4, 16, 16)'),
    (lambda o, p: p.slab_kspace_constrain(o.x3, o.yg, o.m1, MEMBERS, WEIGHTS, *o.lv, keys=o.keys, out=o.x4),
     'slab_kspace_constrain: out must be fp32 of shape (4, 16, 16), got torch.float32 (4, 1, 16, 16)'),
    (lambda o, p: p.slab_kspace_constrain(o.x3, o.yg, o.m1, MEMBERS, WEIGHTS, *o.lv, keys=o.keys, out=torch.empty(ROWS, S, S, device=DEV).transpose(1, 2)),
     'slab_kspace_constrain: out must be contiguous'),
    (lambda o, p: p.slab_kspace_constrain(o.x3, o.yg, o.m1, MEMBERS, WEIGHTS, *o.lv, keys=o.keys, work=torch.empty_like(o.yk)),
     'slab_kspace_constrain: work must be a contiguous complex64 (2, 16, 16), got torch.complex64 (4, 16, 16)'),
    (lambda o, p: p.slab_kspace_constrain(o.x3, o.yg, o.m1, MEMBERS, WEIGHTS, o.t, 0, o.a_tab, None, keys=o.keys), LEVEL.format('slab_kspace_constrain')),
    (lambda o, p: p.slab_kspace_constrain(o.x3, o.yg, o.m1, MEMBERS, WEIGHTS, *o.lv), 'slab_kspace_constrain: pass noise or keys'),
    (lambda o, p: p.slab_kspace_constrain(o.x3, o.yg, o.m1, MEMBERS, WEIGHTS, *o.lv, keys=o.keys[:3]), 'slab_kspace_constrain: 3 keys for 4 rows'),
    # two faults: the grid before the tables, the tables before y
    (lambda o, p: p.slab_kspace_constrain(o.x3[:, :8, :8], o.yg, o.m1, MEMBERS, [0.5, 0.25, 0.25], *o.lv, keys=o.keys),
     'slab_kspace_constrain: S must be a power of two in [16, 512], got 8'),
    (lambda o, p: p.slab_kspace_constrain(o.x3, None, o.m1, MEMBERS, [0.5, 0.25, 0.25], *o.lv, keys=o.keys),
     'slab_tables: weights must be [L] or (2, 2), got (3,)'),

    # ops.band_constrain
    (lambda o, p: p.band_constrain(o.xb, o.yb.cpu(), o.band, *o.lv, keys=o.keys), GPU_ONLY),
    (lambda o, p: p.band_constrain(o.xb, o.yb, o.tab, *o.lv, keys=o.keys), 'band_constrain: tables must come from ops.band_tables'),
    (lambda o, p: p.band_constrain(o.xb[:, :3], o.yb, o.band, *o.lv, keys=o.keys),
     'band_constrain: x must be a non-empty fp32 [sets, 4, ...] tensor, got torch.float32 (1, 3, 3, 5)'),
    (lambda o, p: p.band_constrain(o.xr, o.yb, o.band, *o.lv, keys=o.keys),
     'band_constrain: x must be a non-empty fp32 [sets, 4, ...] tensor, got torch.float32 (4, 3, 5)'),
    (lambda o, p: p.band_constrain(torch.empty(65536, 4, 1, device=DEV), o.yb, o.band, *o.lv, keys=o.keys),
     'band_constrain: sets * max(m, n) * row_len must be < 2^31 and sets <= 65535, got 65536 x 4 x 1'),
    (lambda o, p: p.band_constrain(o.xb, None, o.band, *o.lv, keys=o.keys), 'band_constrain: y must be fp32 [2, 15], got None'),
    (lambda o, p: p.band_constrain(o.xb, o.ys3, o.band, *o.lv, keys=o.keys), 'band_constrain: y must be fp32 [2, 15], got (torch.float32, (2, 16, 16))'),
    (lambda o, p: p.band_constrain(o.xb, o.yb, o.band, *o.lv, noise=o.nr),
     'band_constrain: noise must be fp32 of shape (1, 4, 3, 5), got torch.float32 (4, 3, 5)'),
    (lambda o, p: p.band_constrain(o.xb, o.yb, o.band, *o.lv, keys=o.keys, out=o.xb.double()),
     'band_constrain: out must be fp32 of shape (1, 4, 3, 5), got torch.float64 (1, 4, 3, 5)'),
    (lambda o, p: p.band_constrain(o.xb, o.yb, o.band, *o.lv, keys=o.keys, out=torch.empty(1, ROWS, 5, 3, device=DEV).transpose(2, 3)),
     'band_constrain: out must be contiguous'),
    (lambda o, p: p.band_constrain(o.xb, o.yb, o.band, *o.lv, keys=o.keys, work=torch.empty(2, 16, device=DEV)),
     'band_constrain: work must be a contiguous fp32 tensor of 2 x 15 elements'),
    (lambda o, p: p.band_constrain(o.xb, o.yb, o.band, o.t, 0, o.a_tab, o.s_tab[:1], keys=o.keys), LEVEL.format('band_constrain')),
    (lambda o, p: p.band_constrain(o.xb, o.yb, o.band, *o.lv), 'band_constrain: pass noise or keys'),
    (lambda o, p: p.band_constrain(o.xb, o.yb, o.band, *o.lv, keys=o.keys[:2]), 'band_constrain: 2 keys for 4 rows'),

    # ops.fft2, ops.slab_average, ops.band_measure
    (lambda o, p: p.fft2(o.x3.cpu()), GPU_ONLY),
    (lambda o, p: p.fft2(o.x4), 'fft2: x must be fp32 or complex64 [rows, S, S], got torch.float32 (4, 1, 16, 16)'),
    (lambda o, p: p.fft2(o.x3.half()), 'fft2: x must be fp32 or complex64 [rows, S, S], got torch.float16 (4, 16, 16)'),
    (lambda o, p: p.fft2(o.x3[:, :8, :8]), 'fft2: S must be a power of two in [16, 512], got 8'),
    (lambda o, p: p.fft2(o.x3, out=torch.empty_like(o.x3)),
     'fft2: out must be a contiguous complex64 tensor of shape (4, 16, 16), got torch.float32 (4, 16, 16)'),
    (lambda o, p: p.fft2(o.yk, out=torch.empty_like(o.yk).transpose(1, 2)),
     'fft2: out must be a contiguous complex64 tensor of shape (4, 16, 16), got torch.complex64 (4, 16, 16)'),
    (lambda o, p: p.slab_average(o.xr.cpu(), MEMBERS, WEIGHTS), GPU_ONLY),
    (lambda o, p: p.slab_average(o.xr.double(), MEMBERS, WEIGHTS),
     'slab_average: x must be a non-empty fp32 [rows, ...] tensor, got torch.float64 (4, 3, 5)'),
    (lambda o, p: p.slab_average(o.xr, MEMBERS, [[0.5, 0.5]]), 'slab_tables: weights must be [L] or (2, 2), got (1, 2)'),
    (lambda o, p: p.slab_average(o.xr, MEMBERS, WEIGHTS, out=torch.empty_like(o.xr)),
     'slab_average: out must be a contiguous fp32 tensor of shape (2, 3, 5), got torch.float32 (4, 3, 5)'),
    (lambda o, p: p.band_measure(o.xb.cpu(), o.band), GPU_ONLY),
    (lambda o, p: p.band_measure(o.xb, None), 'band_measure: tables must come from ops.band_tables'),
    (lambda o, p: p.band_measure(o.xb.half(), o.band), 'band_measure: x must be a non-empty fp32 [sets, 4, ...] tensor, got torch.float16 (1, 4, 3, 5)'),
    (lambda o, p: p.band_measure(torch.empty(65536, 4, 1, device=DEV), o.band),
     'band_measure: sets * max(m, n) * row_len must be < 2^31 and sets <= 65535, got 65536 x 4 x 1'),
    (lambda o, p: p.band_measure(o.xb, o.band, out=torch.empty_like(o.xb)),
     'band_measure: out must be a contiguous fp32 tensor of shape (1, 2, 3, 5), got torch.float32 (1, 4, 3, 5)'),

    # the batch-level constraints: `check` against a stand-in for the sampler
    (lambda o, p: _rows('KnownRows', o.x4, None).check(_sampler()), 'GraphSampler.sample_keyed: known needs known_mask'),
    (lambda o, p: _rows('KnownRows', o.x4, o.x4).check(_sampler()),
     'GraphSampler.sample_keyed: known (fp32) and known_mask (uint8) must be (4, 1, 16, 16), got (4, 1, 16, 16) and torch.float32 (4, 1, 16, 16)'),
    (lambda o, p: _rows('KnownRows', o.x3, o.mrows).check(_sampler()),
     'GraphSampler.sample_keyed: known (fp32) and known_mask (uint8) must be (4, 1, 16, 16), got (4, 16, 16) and torch.uint8 (4, 16, 16)'),
    (lambda o, p: _rows('KSpaceRows', o.yk, o.m1).check(_sampler(S, 32)),
     'GraphSampler.sample_keyed: kspace needs a square grid whose size is a power of two in [16, 512], got 16 x 32'),
    (lambda o, p: _rows('KSpaceRows', o.yk, o.m1).check(_sampler(8, 8)),
     'GraphSampler.sample_keyed: kspace needs a square grid whose size is a power of two in [16, 512], got 8 x 8'),
    (lambda o, p: _rows('KSpaceRows', o.yg, o.m1).check(_sampler()),
     'GraphSampler.sample_keyed: kspace = (y complex64 (4, 16, 16), mask uint8 [1 or 4, 16, 16]), got torch.complex64 (2, 16, 16) and '
     'torch.uint8 (1, 16, 16)'),
    (lambda o, p: _rows('KSpaceRows', o.yk, o.mrows[:2]).check(_sampler()),
     'GraphSampler.sample_keyed: kspace = (y complex64 (4, 16, 16), mask uint8 [1 or 4, 16, 16]), got torch.complex64 (4, 16, 16) and '
     'torch.uint8 (2, 16, 16)'),
    (lambda o, p: _rows('SlabRows', (o.ys, MEMBERS, WEIGHTS, None), None).check(_sampler()),
     'GraphSampler.sample_keyed: thick y must be fp32 (2, 16, 16), got torch.float32 (2, 3, 5)'),
    (lambda o, p: _rows('SlabRows', (o.ys3, [[0, 1], [2, 4]], WEIGHTS, None), None).check(_sampler()),
     'GraphSampler.sample_keyed: thick names 2 groups of 2 rows up to row 4 for a batch of 4 (at most 16 rows a group)'),
    (lambda o, p: _rows('SlabRows', (o.x3[:1], [list(range(17))], [1 / 17] * 17, None), None).check(_sampler()),
     'GraphSampler.sample_keyed: thick names 1 groups of 17 rows up to row 16 for a batch of 4 (at most 16 rows a group)'),
    (lambda o, p: _rows('SlabRows', (torch.cat([o.x3, o.x3[:1]]), [[0], [1], [2], [3], [0]], [1.0], None), None).check(_sampler()),
     'GraphSampler.sample_keyed: thick names 5 groups of 1 rows up to row 3 for a batch of 4 (at most 16 rows a group)'),
    (lambda o, p: _rows('SlabKSpaceRows', (o.yg, o.m1, MEMBERS, WEIGHTS, None)).check(_sampler(32, S)),
     'GraphSampler.sample_keyed: multislice needs a square grid whose size is a power of two in [16, 512], got 32 x 16'),
    (lambda o, p: _rows('SlabKSpaceRows', (o.yk, o.m1, MEMBERS, WEIGHTS, None)).check(_sampler()),
     'GraphSampler.sample_keyed: multislice = (y complex64 (2, 16, 16), mask uint8 [1 or 2, 16, 16], ...), got torch.complex64 (4, 16, 16) and '
     'torch.uint8 (1, 16, 16)'),
    (lambda o, p: _rows('SlabKSpaceRows', (o.yg, o.mrows, MEMBERS, WEIGHTS, None)).check(_sampler()),
     'GraphSampler.sample_keyed: multislice = (y complex64 (2, 16, 16), mask uint8 [1 or 2, 16, 16], ...), got torch.complex64 (2, 16, 16) and '
     'torch.uint8 (4, 16, 16)'),
    (lambda o, p: _rows('SlabKSpaceRows', (o.yg, o.m1, [[0, 1], [2, 4]], WEIGHTS, None)).check(_sampler()),
     'GraphSampler.sample_keyed: multislice names 2 groups of 2 rows up to row 4 for a batch of 4 (at most 16 rows a group)'),
    # two faults: the grid before the operands, the operands before the tables
    (lambda o, p: _rows('SlabKSpaceRows', (o.yk, o.m1, [[0, 1], [2, 4]], WEIGHTS, None)).check(_sampler(8, 8)),
     'GraphSampler.sample_keyed: multislice needs a square grid whose size is a power of two in [16, 512], got 8 x 8'),
    (lambda o, p: _rows('SlabKSpaceRows', (o.yk, o.m1, [[0, 1], [2, 4]], WEIGHTS, None)).check(_sampler()),
     'GraphSampler.sample_keyed: multislice = (y complex64 (2, 16, 16), mask uint8 [1 or 2, 16, 16], ...), got torch.complex64 (4, 16, 16) and '
     'torch.uint8 (1, 16, 16)'),
    (lambda o, p: _rows('SlabRows', (o.ys, [[0, 1], [2, 4]], WEIGHTS, None), None).check(_sampler()),
     'GraphSampler.sample_keyed: thick y must be fp32 (2, 16, 16), got torch.float32 (2, 3, 5)'),
    (lambda o, p: _band_measurement(o.ys3).check_volume(_sampler(), 6), 'GraphSampler.sample_lockstep: 6 rows are not whole stacks of 4 slices'),
    (lambda o, p: _band_measurement(o.yb).check_volume(_sampler(), 8),
     'GraphSampler.sample_lockstep: thick volume y must be fp32 (2, 16, 16), got torch.float32 (2, 3, 5)'),
    (lambda o, p: _band_measurement(o.ys3.double()).check_volume(_sampler(), 4),
     'GraphSampler.sample_lockstep: thick volume y must be fp32 (2, 16, 16), got torch.float64 (2, 16, 16)'),
]


@pytest.mark.parametrize('i', range(len(REFUSALS)))
def test_the_refusal_keeps_its_words_and_its_place(i):
    from mudiff_hip import MudiffHipError
    call, message = REFUSALS[i]
    with pytest.raises((MudiffHipError, ValueError)) as e:
        call(_o(), _ops())
    assert str(e.value) == message


# ---------------------------------------------------------------------------------------------------
# accepted calls: the checked wrapper against the unchecked launcher on operands prepared by hand
# ---------------------------------------------------------------------------------------------------
def _spread(t):
    """t's values in a tensor that is not contiguous: every other element of a last axis twice as long."""
    wide = torch.zeros(*t.shape[:-1], 2 * t.shape[-1], device=t.device, dtype=t.dtype)
    wide[..., ::2] = t
    v = wide[..., ::2]
    assert not v.is_contiguous() and torch.equal(v, t)
    return v


def _wrappers(o, p):
    """name -> (x_new, its noise, checked(x, **kw), unchecked(out, x, keys_dev, t, a_tab, s_tab, clean, noise))."""
    kwork = lambda n: torch.empty(n, S, S, device=DEV, dtype=torch.complex64)      # noqa: E731
    return {
        'known': (o.xr, o.nr, lambda x, t, a, s, **kw: p.known_constrain(x, o.known, o.kmask, t, 0, a, s, **kw),
                  lambda out, x, kd, t, a, s, clean, noise: p.known_constrain_into(out, x, o.known, o.kmask, kd, SEED, STEP, p.KIND_KNOWN, t, 0, a, s,
                                                                                   clean, noise)),
        'kspace': (o.x4, o.n4, lambda x, t, a, s, **kw: p.kspace_constrain(x, o.yk, o.mrows, t, 0, a, s, **kw),
                   lambda out, x, kd, t, a, s, clean, noise: p.kspace_constrain_into(out, x, o.yk, o.mrows, kwork(ROWS), kd, SEED, STEP, p.KIND_KSPACE,
                                                                                     t, 0, a, s, clean, noise)),
        'slab': (o.xr, o.nr, lambda x, t, a, s, **kw: p.slab_constrain(x, o.ys, MEMBERS, WEIGHTS, t, 0, a, s, **kw),
                 lambda out, x, kd, t, a, s, clean, noise: p.slab_constrain_into(out, x, o.ys, o.tab, kd, SEED, STEP, p.KIND_THICK, t, 0, a, s, clean,
                                                                                 noise)),
        'slab_kspace': (o.x3, o.n3, lambda x, t, a, s, **kw: p.slab_kspace_constrain(x, o.yg, o.m1, MEMBERS, WEIGHTS, t, 0, a, s, **kw),
                        lambda out, x, kd, t, a, s, clean, noise: p.slab_kspace_constrain_into(out, x, o.yg, o.m1, o.tab, kwork(GROUPS), kd, SEED, STEP,
                                                                                               p.KIND_MULTISLICE, t, 0, a, s, clean, noise)),
        'band': (o.xb, o.nb, lambda x, t, a, s, **kw: p.band_constrain(x, o.yb, o.band, t, 0, a, s, **kw),
                 lambda out, x, kd, t, a, s, clean, noise: p.band_constrain_into(out, x, o.yb, o.band, torch.empty(2, 15, device=DEV), kd, SEED, STEP,
                                                                                 p.KIND_BAND, t, 0, a, s, clean, noise)),
    }


@pytest.mark.parametrize('draw', ('keys', 'noise', 'clean'))
@pytest.mark.parametrize('name', ('known', 'kspace', 'slab', 'slab_kspace', 'band'))
def test_an_accepted_call_is_the_unchecked_launch_bit_for_bit(name, draw):
    o, p = _o(), _ops()
    x, eta, checked, unchecked = _wrappers(o, p)[name]
    kw = dict(seed=SEED, step=STEP, **dict(keys=dict(keys=o.keys), noise=dict(noise=eta), clean=dict(clean=True))[draw])
    level = (None, None, None) if draw == 'clean' else (o.t, o.a_tab, o.s_tab)
    want = unchecked(torch.empty_like(x), x, o.kd if draw == 'keys' else None, *level, draw == 'clean', eta if draw == 'noise' else None)
    assert not torch.equal(want, x)
    bits = lambda v: v.contiguous().view(torch.int32)      # noqa: E731
    got = checked(x, *level, **kw)                                          # out=None: a new tensor, x untouched
    assert got.data_ptr() != x.data_ptr() and got.is_contiguous() and torch.equal(bits(got), bits(want))
    mine = x.clone()
    got = checked(mine, *level, out=mine, **kw)                             # out is x_new: in place
    assert got is mine and torch.equal(bits(mine), bits(want))
    apart = _spread(x)
    got = checked(apart, *level, **kw)                                      # x_new not contiguous: a contiguous copy is read
    assert got.is_contiguous() and torch.equal(bits(got), bits(want)) and torch.equal(apart, x)
    other = torch.empty_like(x)
    kw_apart = dict(kw, noise=_spread(eta)) if draw == 'noise' else kw
    assert checked(apart, *level, out=other, **kw_apart) is other and torch.equal(bits(other), bits(want))
    with pytest.raises(p.MudiffHipError) as e:                              # and it cannot be the output
        checked(apart, *level, out=apart, **kw)
    assert str(e.value).endswith(': out must be contiguous')


def test_known_everywhere_writes_into_known_itself():
    """ops.known_constrain without a mask and without x_new, out = known: the keyed q_sample the re-noising step is."""
    o, p = _o(), _ops()
    want = p.known_constrain_into(torch.empty_like(o.known), None, o.known, None, o.kd, SEED, STEP, p.KIND_RENOISE, o.t, 1, o.a_tab, o.s_tab)
    mine = o.known.clone()
    got = p.known_constrain(None, mine, None, o.t, 1, o.a_tab, o.s_tab, keys=o.keys, seed=SEED, step=STEP, kind=p.KIND_RENOISE, out=mine)
    assert got is mine and torch.equal(mine.view(torch.int32), want.view(torch.int32))
    got = p.known_constrain(None, _spread(o.known), None, o.t, 1, o.a_tab, o.s_tab, keys=o.keys, seed=SEED, step=STEP, kind=p.KIND_RENOISE)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))


def test_a_checked_batch_constraint_applies_the_unchecked_launch():
    """check, then apply, of the four batch-level constraints against a stand-in for the sampler: the launch of the `*_into` launcher
    with the stand-in's level tables, and one complex workspace per sampler."""
    o, p = _o(), _ops()
    known4, mask4 = o.n4, (o.mrows[:, None] != 0).to(torch.uint8)
    cases = [
        (_rows('KnownRows', known4, mask4), p.KIND_KNOWN,
         lambda out, kind: p.known_constrain_into(out, o.x4, known4, mask4, o.kd, SEED, STEP, kind, o.t, 0, o.a_tab, o.s_tab)),
        (_rows('KSpaceRows', o.yk, o.m1), p.KIND_KSPACE,
         lambda out, kind: p.kspace_constrain_into(out, o.x4, o.yk, o.m1, torch.empty_like(o.yk), o.kd, SEED, STEP, kind, o.t, 0, o.a_tab, o.s_tab)),
        (_rows('SlabRows', (o.ys3, MEMBERS, WEIGHTS, None), None), p.KIND_THICK,
         lambda out, kind: p.slab_constrain_into(out, o.x4, o.ys3, o.tab, o.kd, SEED, STEP, kind, o.t, 0, o.a_tab, o.s_tab)),
        (_rows('SlabKSpaceRows', (o.yg, o.m1, MEMBERS, WEIGHTS, None)), p.KIND_MULTISLICE,
         lambda out, kind: p.slab_kspace_constrain_into(out, o.x4, o.yg, o.m1, o.tab, torch.empty_like(o.yk), o.kd, SEED, STEP, kind, o.t, 0, o.a_tab,
                                                        o.s_tab)),
    ]
    sampler = _sampler()
    for rows, kind, unchecked in cases:
        rows.check(sampler)
        work = getattr(sampler, '_ks_work', None)
        sampler.x.fill_(7.0)
        rows.apply(sampler, o.x4, o.kd, SEED, STEP, False)
        assert getattr(sampler, '_ks_work', None) is work
        want = unchecked(torch.empty_like(o.x4), kind)
        assert torch.equal(sampler.x.view(torch.int32), want.view(torch.int32)) and not torch.equal(want, o.x4)
    assert tuple(sampler._ks_work.shape) == (ROWS, S, S) and sampler._ks_work.dtype == torch.complex64
    assert sampler.thick_x_new is o.x4
