"""Precision guard of the fp8 cross-term plan: is MUD_PREC_PLAN=auto safe for THESE weights?

Under the default plan almost every large 3x3 convolution runs MUD_PREC_FP8X: the two cross terms of each split product go
through e4m3 MFMAs, with the activation images at CONSTANT power-of-two pre-scales (mud_common.h: CM_X_SA, CM_X_SAL).  They are
right while the conv input after its prologue stays inside about [5e-4, 112]; outside it they saturate or flush and those products
fall from ~2^-15 to ~2^-10 relative error.  Seeded weights stay inside; a trained checkpoint with large AdaGN gains or large
un-normalised gate-conv inputs may not.  This module measures that once per checkpoint and, where needed, switches exactly the
offending layers back to fp16 x 3 - before a GraphSampler is captured:

    cal = calibrate_plan(coefficients, g1, cond1, g2, cond2, cond3, n_time, opt)      # at the production B, H, W
    cal.decision        # 'auto' | 'per_layer' | 'off' | 'unchanged' (MUD_PREC_PLAN is already 'off')
    cal.to_dict()       # JSON-able record
    clear_plan(g1, g2)  # remove the overrides

Procedure (deterministic given its inputs; `decide` is the pure host rule):
  A  eager sample_from_model under prec_plan('off'), every step recorded;
  B  the same under 'auto' inside census(): every fp8x conv launch also runs the e4m3 range census (mud_e4m3_census) of its
     input after its prologue, into a slot per layer;
  dev_B = max over steps of max-abs(B - A) of x_0_1, x_0_2 and x_new.  dev_B <= threshold -> 'auto', nothing installed.
  Otherwise (per_layer) every layer whose census saw n_over > 0 or n_fp16_over > 0 is reverted and C is run; dev_C <= threshold
  -> 'per_layer'.  Otherwise, or with nothing flagged -> 'off': every layer that ran fp8x is reverted.
The draws come from a private torch.Generator (or the caller's): calibrating never consumes the global or the driver's RNG.
Overrides live on the generator by layer name (state_dict prefix; G2's merged gate conv is 'feat_att') and survive any rebuild of
the prepared-weight caches.  Plan eligibility depends on the grid size, so calibrate at the batch and image size the sampler uses.
"""
from __future__ import annotations

import math
import struct
import time

import torch

from . import ops

DEFAULT_THRESHOLD = 5e-4
CENSUS = None         # the active census() collector, or None: read by every fp8x ConvParam launch (backbones/layerspp.py)
COUNTS = ('n', 'n_over', 'n_under', 'n_fp16_over')


def _capturing():
    return torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()


class _Census:
    """Per-layer census slots of one census() context: (PlanScope, layer name) -> device accumulator (ops.new_census_slot)."""

    def __init__(self):
        self.slots = {}
        self.launches = 0

    def add(self, conv, x, pro):
        if _capturing():
            raise RuntimeError('precision.census() is eager only: a census launch cannot be captured into a graph')
        key = (id(conv.scope), conv.name)
        if key not in self.slots:
            self.slots[key] = (conv.scope, conv.name, ops.new_census_slot(x.device))
        ops.e4m3_census(x, pro, self.slots[key][2])
        self.launches += 1

    def table(self, scopes):
        """{label: {layer name: {n, n_over, n_under, n_fp16_over, amax}}} for the generators' PlanScopes {label: scope}."""
        out = {label: {} for label in scopes}
        for scope, name, t in self.slots.values():
            for label, s in scopes.items():
                if s is scope:
                    v = [int(c) for c in t.cpu().tolist()]
                    d = dict(zip(COUNTS, v[:4]))
                    d['amax'] = struct.unpack('<f', struct.pack('<I', v[4] & 0xFFFFFFFF))[0]
                    out[label][name] = d
        return out


class census:
    """Context: while active, every ConvParam launch that runs MUD_PREC_FP8X first launches the e4m3 range census of its input
    and prologue into a slot of its layer (`.slots`, `.launches`).  Eager only: refuses to start under graph capture."""

    def __enter__(self):
        global CENSUS
        if _capturing():
            raise RuntimeError('precision.census() is eager only (the current stream is capturing a graph)')
        if CENSUS is not None:
            raise RuntimeError('precision.census() does not nest')
        CENSUS = self.c = _Census()
        return self.c

    def __exit__(self, *exc):
        global CENSUS
        CENSUS = None
        return False


def record(conv, x, pro):
    """Hook of ConvParam.__call__ (fp8x launches inside census())."""
    CENSUS.add(conv, x, pro)


class launch_record:
    """Context: collects one ops.Launch (layer name, plan, kernel size, kernel, shape, ...) per convolution launch issued inside
    (`.launches`; `.plans()` = [(layer, plan)]).  Eager only, like census(): refuses to start under graph capture, and a launch
    captured while it is active raises."""

    def __enter__(self):
        if _capturing():
            raise RuntimeError('precision.launch_record() is eager only (the current stream is capturing a graph)')
        if ops.RECORD is not None:
            raise RuntimeError('precision.launch_record() does not nest')
        self.launches = ops.RECORD = []
        return self

    def __exit__(self, *exc):
        ops.RECORD = None
        return False

    def plans(self):
        return [(r.layer, r.prec) for r in self.launches]


# ---------------------------------------------------------------------------------------------------
def conv_layer_names(g):
    """Names of the layers of generator `g` that can run MUD_PREC_FP8X (3x3 convs on the matrix-core kernel), from module
    structure alone (no GPU): state_dict prefixes such as 'all_modules.22.Conv_0', and 'feat_att' for G2's merged gate conv."""
    from backbones.layerspp import ConvParam
    from backbones.ncsnpp_generator_adagn_feat import GATES_NAME
    names = []
    for n, m in g.named_modules():
        if not isinstance(m, torch.nn.Conv2d):
            continue
        O, I, k, _ = m.weight.shape
        if n.startswith('feat_att'):          # feat_att1_* / feat_att2_*: one merged launch of all gates (same input)
            if GATES_NAME not in names and k == 3 and ConvParam.uses_mfma(O, I, k):
                names.append(GATES_NAME)
        elif k == 3 and tuple(m.stride) == (1, 1) and tuple(m.padding) == (1, 1) and ConvParam.uses_mfma(O, I, k, m.stride, m.padding):
            names.append(n)
    return names


def set_plan(g, names):
    """Run exactly the layers `names` of generator `g` as fp16 x 3 (replaces its overrides)."""
    ov = g._plan_scope.overrides
    ov.clear()
    ov.update(names)


def clear_plan(*gens):
    """Remove every per-layer override of the generators: MUD_PREC_PLAN decides alone again."""
    for g in gens:
        g._plan_scope.overrides.clear()


def plan_overrides(g):
    return sorted(g._plan_scope.overrides)


# ---------------------------------------------------------------------------------------------------
def flagged_layers(table):
    """{gen: sorted names} of the layers whose census saw a saturating e4m3 image or fp16 piece."""
    return {gen: sorted(n for n, c in layers.items() if c['n_over'] > 0 or c['n_fp16_over'] > 0) for gen, layers in table.items()}


def decide(dev_b, table, threshold=DEFAULT_THRESHOLD, *, dev_c=None, per_layer=True, plan='auto'):
    """The decision rule, a pure host function of the deviations and the census table -> (decision, reverts {gen: [names]}).
    dev_b / dev_c: max-abs deviation from the 'off' run of run B ('auto') / run C ('auto' with the flagged layers reverted;
    None = not run yet).  'pending' asks the caller to run C with `reverts` installed and call again with dev_c."""
    if plan == 'off':
        return 'unchanged', {}
    if dev_b <= threshold:                     # (NaN compares False: never kept)
        return 'auto', {}
    flagged = {gen: ns for gen, ns in flagged_layers(table).items() if ns}
    if per_layer and flagged:
        if dev_c is None:
            return 'pending', flagged
        if dev_c <= threshold:
            return 'per_layer', flagged
    every = {gen: sorted(n for n, c in layers.items() if c['n'] > 0) for gen, layers in table.items()}
    return 'off', {gen: ns for gen, ns in every.items() if ns}


def merge_over_ranks(devs, table, names, group=None):
    """MAX over the ranks of `group` of the deviations (list of floats) and of every census counter of every layer in `names`
    ({gen: [names]}, the same on every rank) -> (devs, table).  Single process or no group: the inputs, zero-filled to `names`."""
    import torch.distributed as dist
    keys = [(gen, n) for gen in sorted(names) for n in names[gen]]
    zero = dict.fromkeys(COUNTS, 0)
    zero['amax'] = 0.0
    table = {gen: {n: dict(table.get(gen, {}).get(n, zero)) for n in names[gen]} for gen in sorted(names)}
    if group is None or not dist.is_initialized() or dist.get_world_size(group) == 1:
        return list(devs), table
    fix = lambda v: math.inf if math.isnan(v) else float(v)      # noqa: E731  (a NaN deviation must win the MAX)
    vals = [fix(v) for v in devs]
    for gen, n in keys:
        c = table[gen][n]
        vals += [float(c[k]) for k in COUNTS] + [fix(c['amax'])]
    dev = torch.device('cuda', torch.cuda.current_device()) if dist.get_backend(group) == 'nccl' else torch.device('cpu')
    t = torch.tensor(vals, dtype=torch.float64, device=dev)
    dist.all_reduce(t, op=dist.ReduceOp.MAX, group=group)
    v = t.cpu().tolist()
    out_devs, i = v[:len(devs)], len(devs)
    for gen, n in keys:
        c = dict(zip(COUNTS, (int(x) for x in v[i:i + 4])))
        c['amax'] = v[i + 4]
        table[gen][n] = c
        i += 5
    return out_devs, table


# ---------------------------------------------------------------------------------------------------
class Calibration:
    """Result of calibrate_plan."""

    def __init__(self, decision, threshold, shape, seed, world=1):
        self.decision, self.threshold, self.shape, self.seed, self.world = decision, float(threshold), list(shape), seed, world
        self.dev_b = self.dev_c = None
        self.steps = {}               # run -> per step [max-abs x_0_1, x_0_2, x_new] against run A
        self.census = {}              # gen -> layer -> counters (MAX over ranks)
        self.reverted = {}            # gen -> layer names installed as fp16 x 3
        self.census_launches = 0
        self.wall_s = 0.0

    def to_dict(self):
        return dict(decision=self.decision, threshold=self.threshold, dev_b=self.dev_b, dev_c=self.dev_c, shape=self.shape,
                    seed=self.seed, world=self.world, steps=self.steps, census=self.census, reverted=self.reverted,
                    census_launches=self.census_launches, wall_s=self.wall_s)

    def summary(self):
        dc = '' if self.dev_c is None else f' dev_C={self.dev_c:.3e}'
        rv = ' '.join(f'{g}:{len(ns)}' for g, ns in sorted(self.reverted.items())) or 'none'
        db = 'n/a' if self.dev_b is None else f'{self.dev_b:.3e}'
        return (f'fp8x precision calibration at B,H,W={tuple(self.shape)}: decision={self.decision} dev_B={db}{dc} '
                f'(threshold {self.threshold:g}), layers reverted to fp16x3: {rv}, {self.wall_s:.1f} s')


def _deviations(run_a, run_b):
    return [[float((b - a).abs().max()) for a, b in zip(sa, sb)] for sa, sb in zip(run_a, run_b)]


def calibrate_plan(coefficients, g1, cond1, g2, cond2, cond3, n_time, opt, x_init=None, zs=None, noises=None, seed=0,
                   threshold=DEFAULT_THRESHOLD, per_layer=True, apply=True, group=None):
    """Run the guard (module docstring) on one batch of conditions [B,1,H,W] - the batch the production sampler will take, at
    its B, H, W - and, unless apply=False, install its per-layer overrides on g1 / g2.  Draws not injected (x_init [B,1,H,W],
    zs / noises per step) come from a private torch.Generator seeded with `seed`.  `group` (torch.distributed, > 1 rank): every
    rank calibrates its own batch; deviations and census counters are MAX-reduced, so every rank installs the same overrides."""
    if ops.PREC_PLAN == 'fp16':
        raise ValueError("calibrate_plan: the guard measures the fp8 cross-term plan against fp16 x 3 and means nothing under the "
                         "single-pass 'fp16' plan (MUD_PREC_PLAN / ops.prec_plan)")
    from . import sampling as S
    t0 = time.perf_counter()
    B, _, H, W = cond1.shape
    dev = cond1.device
    import torch.distributed as dist
    world = dist.get_world_size(group) if group is not None and dist.is_initialized() else 1
    cal = Calibration('unchanged', threshold, (B, H, W), seed, world)
    if ops.PREC_PLAN == 'off':
        return cal
    gen = torch.Generator().manual_seed(int(seed))
    if x_init is None:
        x_init = torch.randn(B, 1, H, W, generator=gen)
    if zs is None:
        zs = [torch.randn(B, opt.nz, generator=gen) for _ in range(n_time)]
    if noises is None:
        noises = [torch.randn(B, 1, H, W, generator=gen) for _ in range(n_time)]
    x_init, zs, noises = x_init.to(dev), [z.to(dev) for z in zs], [e.to(dev) for e in noises]
    gens = {'g1': g1, 'g2': g2}
    saved = {k: plan_overrides(g) for k, g in gens.items()}

    def run():
        _, steps = S.sample_from_model(coefficients, g1, cond1, g2, cond2, cond3, n_time, x_init, None, opt, zs=zs, noises=noises,
                                       return_steps=True)
        return steps

    clear_plan(g1, g2)
    try:
        with ops.prec_plan('off'):
            run_a = run()
        with ops.prec_plan('auto'), census() as cs:
            run_b = run()
        cal.census_launches = cs.launches
        cal.steps['B'] = _deviations(run_a, run_b)
        del run_b
        names = {k: conv_layer_names(g) for k, g in gens.items()}
        (cal.dev_b,), cal.census = merge_over_ranks([max(max(s) for s in cal.steps['B'])], cs.table({k: g._plan_scope for k, g in gens.items()}),
                                                     names, group)
        cal.decision, reverts = decide(cal.dev_b, cal.census, threshold, per_layer=per_layer)
        if cal.decision == 'pending':
            for k, g in gens.items():
                set_plan(g, reverts.get(k, ()))
            with ops.prec_plan('auto'):
                cal.steps['C'] = _deviations(run_a, run())
            (cal.dev_c,), _ = merge_over_ranks([max(max(s) for s in cal.steps['C'])], {}, {}, group)
            cal.decision, reverts = decide(cal.dev_b, cal.census, threshold, dev_c=cal.dev_c, per_layer=per_layer)
        cal.reverted = reverts
    finally:
        for k, g in gens.items():       # on apply=False (or an error) the generators keep what they had
            set_plan(g, saved[k])
    if apply:
        for k, g in gens.items():
            set_plan(g, cal.reverted.get(k, ()))
    torch.cuda.synchronize(dev)
    cal.wall_s = time.perf_counter() - t0
    return cal
