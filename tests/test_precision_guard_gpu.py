"""GPU: the precision guard of the fp8 cross-term plan - the e4m3 range census kernel against a host restatement, its ABI
refusals, census mode changing nothing, the calibration on seeded weights (keeps 'auto') and on weights that push conv inputs out
of the e4m3 images' range (trips), and the driver's --calibrate end to end."""
import ctypes as C
import json
import os
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest
import torch

from conftest import PKG, REPO
from helpers import SMALL_CFGS, load_golden, sampler_inputs
from oracle import mudiff_oracle as O

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DEV = 'cuda:0'
THRESH = 5e-4

SA, SAL = 2, 13            # CM_X_SA, CM_X_SAL (mud_common.h)


def _fp16_lo(a32):
    """a - fp16(a) with the fp16 piece saturating at +-65504, in fp32 (the conv's staging)."""
    hi = np.clip(a32, -65504.0, 65504.0).astype(np.float16).astype(np.float32)
    return (a32 - hi).astype(np.float32)


def _host_prologue(x, sc, sh, mode):
    """fp32 result of the conv's prologue, evaluated in fp64 (fma: one rounding; SiLU exact)."""
    x64 = x.astype(np.float64)
    if mode == 0:
        return x.astype(np.float32)
    a = (x64 * sc.astype(np.float64) + sh.astype(np.float64)).astype(np.float32).astype(np.float64)
    if mode == 2:
        a = a / (1.0 + np.exp(-a))
    return a.astype(np.float32)


def _margin_ok(a32, rel=1e-3):
    """Every element >= rel away (relatively) from each threshold of the census, and not in the range where the fast SiLU's
    flush to zero and the exact one's tiny value could disagree."""
    m = np.abs(a32.astype(np.float64))
    lo = np.abs(_fp16_lo(a32).astype(np.float64))
    ok = np.ones(a32.shape, bool)
    for thr, v in ((448.0 / 2 ** SA, m), (2.0 ** -9 / 2 ** SA, m), (65504.0, m), (448.0 / 2 ** SAL, lo)):
        ok &= np.abs(v - thr) > rel * thr
    return ok & ((m == 0) | (m > 1e-30))


def _host_census(a32):
    m = np.abs(a32.astype(np.float64))
    lo = np.abs(_fp16_lo(a32).astype(np.float64))
    ms = m * 2 ** SA
    return dict(n=a32.size, n_over=int(((ms > 448) | (lo * 2 ** SAL > 448)).sum()), n_under=int(((ms > 0) & (ms < 2.0 ** -9)).sum()),
                n_fp16_over=int((m > 65504).sum()), amax=float(np.abs(a32).max()))


def _slot_dict(t):
    v = [int(c) for c in t.cpu().tolist()]
    return dict(n=v[0], n_over=v[1], n_under=v[2], n_fp16_over=v[3], amax=struct.unpack('<f', struct.pack('<I', v[4] & 0xFFFFFFFF))[0])


def _make_input(B, H, W, C, ld, mode, seed, lazy=False):
    """NHWC input whose every element, after the prologue, keeps its distance from the census thresholds; magnitudes spread
    log-uniformly over 1e-7 .. 2e5 so that every counter fires."""
    from mudiff_hip import ops
    rng = np.random.default_rng(seed)
    sc = (rng.uniform(0.5, 2.0, (B, C)) * rng.choice([-1, 1], (B, C))).astype(np.float32)
    sh = rng.uniform(-0.5, 0.5, (B, C)).astype(np.float32)
    x = np.zeros((B, H, W, ld), np.float32)
    x[..., C:] = np.nan                                      # padding channels beyond C must never be read
    core = (10.0 ** rng.uniform(-7, 5.3, (B, H, W, C)) * rng.choice([-1, 1], (B, H, W, C))).astype(np.float32)
    pro = None
    if lazy:       # producer-style (sum, sumsq) statistics; the prologue arrays come from LazyGN.tensors()
        core = rng.standard_normal((B, H, W, C)).astype(np.float32) * 3.0
        core[..., :C // 2] *= 1e4                            # half the channels far out of range after the affine
    x[..., :C] = core
    xt = torch.from_numpy(x).to(DEV)
    if lazy:
        xd = xt[..., :C].double()
        stats = torch.zeros(B, ld, 2, dtype=torch.float64, device=DEV)
        stats[:, :C, 0] = xd.sum((1, 2))
        stats[:, :C, 1] = (xd * xd).sum((1, 2))
        v = ops.View(xt, B, H, W, C, ld, stats=stats)
        G = 3 if C % 3 == 0 else 4
        gamma = torch.from_numpy(rng.uniform(50, 300, (B, C)).astype(np.float32)).to(DEV)
        beta = torch.from_numpy(rng.uniform(-1, 1, (B, C)).astype(np.float32)).to(DEV)
        lz = ops.gn_lazy(v, G, gamma, beta)
        assert isinstance(lz, ops.LazyGN)
        pro = (lz, None, mode)
        scs, shs = (t.cpu().numpy() for t in lz.tensors())
    else:
        v = ops.View(xt, B, H, W, C, ld)
        scs, shs = sc, sh
        if mode:
            pro = (torch.from_numpy(sc).to(DEV), torch.from_numpy(sh).to(DEV), mode)
    for _ in range(50):    # move elements that sit near a threshold (their count could differ by rounding) somewhere else
        a = _host_prologue(core, scs[:, None, None, :], shs[:, None, None, :], mode)
        bad = ~_margin_ok(a)
        if not bad.any():
            break
        core[bad] = (rng.uniform(0.3, 3.0, int(bad.sum())) * rng.choice([-1, 1], int(bad.sum()))).astype(np.float32)
    else:
        raise AssertionError('could not build a margin-safe input')
    x[..., :C] = core
    xt.copy_(torch.from_numpy(x))
    return v, pro, a


@pytest.mark.parametrize('case', [
    dict(B=3, H=7, W=9, C=12, ld=16, mode=0),
    dict(B=3, H=5, W=11, C=12, ld=12, mode=1),
    dict(B=3, H=7, W=9, C=20, ld=24, mode=2),
    dict(B=2, H=9, W=7, C=48, ld=52, mode=2, lazy=True),
    dict(B=1, H=3, W=5, C=1100, ld=1104, mode=2),           # more than 256 float4 columns per pixel
], ids=['none_ldx', 'affine', 'affine_silu_ldx', 'lazygn_silu', 'wide_c'])
def test_census_matches_host_restatement(case):
    from mudiff_hip import ops
    c = dict(case)
    lazy = c.pop('lazy', False)
    v, pro, a = _make_input(c['B'], c['H'], c['W'], c['C'], c['ld'], c['mode'], seed=zlib.crc32(repr(sorted(case.items())).encode()), lazy=lazy)
    want = _host_census(a)
    assert want['n_over'] > 0 and want['n_under'] + want['n_fp16_over'] > 0 or lazy
    slot = ops.new_census_slot(DEV)
    ops.e4m3_census(v, pro, slot)
    got = _slot_dict(slot)
    print(f'{case}: census {got} host {want}')
    for k in ('n', 'n_over', 'n_under', 'n_fp16_over'):
        assert got[k] == want[k], k
    assert abs(got['amax'] - want['amax']) <= 2 * np.spacing(np.float32(want['amax']))
    first = slot.clone()
    ops.e4m3_census(v, pro, slot)                               # accumulates: the counts double, the max stays
    twice = _slot_dict(slot)
    assert all(twice[k] == 2 * got[k] for k in ('n', 'n_over', 'n_under', 'n_fp16_over')) and int(slot[4]) == int(first[4])
    again = ops.new_census_slot(DEV)
    ops.e4m3_census(v, pro, again)
    assert torch.equal(again, first)                            # bit-reproducible
    if lazy:       # the conv still receives the lazy form: ops.conv folds the finalisation into its own prologue
        assert isinstance(pro[0], ops.LazyGN)


def test_census_abi_refuses_bad_arguments():
    import mudiff_hip
    from mudiff_hip import CensusArgs
    lib = mudiff_hip.load()
    x = torch.zeros(2, 4, 4, 16, device=DEV)
    sc = torch.ones(2, 16, device=DEV)
    out = torch.arange(1, 6, device=DEV, dtype=torch.int64)
    ref = out.clone()

    def args(**kw):
        a = CensusArgs()
        a.x, a.B, a.H, a.W, a.C, a.ldx, a.pro_mode = x.data_ptr(), 2, 4, 4, 16, 16, 0
        for k, val in kw.items():
            setattr(a, k, val)
        return a

    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    o = C.c_void_p(out.data_ptr())
    bad = [args(x=None), args(ldx=12), args(C=14, ldx=16), args(C=0), args(x=x.data_ptr() + 4), args(pro_mode=3), args(pro_mode=7),
           args(pro_mode=1), args(pro_mode=2, pro_scale=sc.data_ptr(), pro_shift=sc.data_ptr(), pro_ld=8),
           args(pro_mode=1, pro_scale=sc.data_ptr() + 4, pro_shift=sc.data_ptr(), pro_ld=16), args(B=0), args(H=0)]
    for a in bad:
        assert lib.mud_e4m3_census(C.byref(a), o, s) != 0
        assert lib.mud_last_error()
    assert lib.mud_e4m3_census(None, o, s) != 0
    assert lib.mud_e4m3_census(C.byref(args()), None, s) != 0
    assert lib.mud_e4m3_census(C.byref(args()), C.c_void_p(out.data_ptr() + 4), s) != 0
    torch.cuda.synchronize()
    assert torch.equal(out, ref)                                 # nothing was launched
    assert lib.mud_e4m3_census(C.byref(args()), o, s) == 0      # (the same call, well formed)
    torch.cuda.synchronize()
    assert int(out[0]) == 1 + 2 * 4 * 4 * 16


def _child(code, env_extra=None, timeout=900):
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([REPO, PKG, os.path.join(REPO, 'tests'), os.environ.get('PYTHONPATH', '')]))
    env.update(env_extra or {})
    p = subprocess.run([sys.executable, '-c', code], cwd=REPO, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                       timeout=timeout)
    print(p.stdout[-4000:])
    return p


def test_census_mode_changes_nothing():
    """Config-3 shapes (256x256, nf 64), B=32, eager, MUD_DETERMINISTIC=1 (a child process: read at import): the outputs of every
    step are bit-identical with and without the census context; every fp8x conv launch had exactly one census launch."""
    code = r'''
import torch
from helpers import load_golden, sampler_inputs
from oracle import mudiff_oracle as O
from mudiff_hip import ops, precision, sampling as S
from backbones.ncsnpp_generator_adagn_feat import NCSNpp, NCSNpp_adaptive
assert ops.DETERMINISTIC and ops.PREC_PLAN == "auto"
cfg = O.default_config()
g1, g2 = NCSNpp(cfg), NCSNpp_adaptive(cfg)
g1.load_state_dict(O.make_state_dict(cfg, "g1", 1234)); g2.load_state_dict(O.make_state_dict(cfg, "g2", 1234))
g1, g2 = g1.cuda().eval(), g2.cuda().eval()
sl = load_golden("batch_cfg3.npz")["slices_u8"].float() / 255.0 * 2.0 - 1.0
conds = [sl[:, c:c + 1].repeat(8, 1, 1, 1).contiguous().cuda() for c in range(3)]
x_init, zs, noises = sampler_inputs(cfg, 32)
coef = S.Posterior_Coefficients(cfg, "cuda:0")
run = lambda: S.sample_from_model(coef, g1, conds[0], g2, conds[1], conds[2], 4, x_init.cuda(), None, cfg, zs=[z.cuda() for z in zs],
                                  noises=[n.cuda() for n in noises], return_steps=True)[1]
plain = run()
ops.PROFILE.enable()
with precision.census() as cs:
    guarded = run()
names = [r[0] for r in ops.PROFILE.records]
ops.PROFILE.disable()
assert all(torch.equal(a, b) for sa, sb in zip(plain, guarded) for a, b in zip(sa, sb)), "census mode changed an output"
n8, nc = sum(n.endswith("_fp8x") for n in names), names.count("e4m3_census")
assert n8 > 0 and n8 == nc == cs.launches, (n8, nc, cs.launches)
table = cs.table({"g1": g1._plan_scope, "g2": g2._plan_scope})
assert any(c["n"] > 0 for t in table.values() for c in t.values())
for k, g in (("g1", g1), ("g2", g2)):
    assert set(table[k]) <= set(precision.conv_layer_names(g)), set(table[k]) - set(precision.conv_layer_names(g))
assert sum(len(t) for t in table.values()) == len(cs.slots)
print("CENSUS-NEUTRAL-OK", n8, {k: len(t) for k, t in table.items()})
'''
    p = _child(code, dict(MUD_DETERMINISTIC='1'))
    assert p.returncode == 0 and 'CENSUS-NEUTRAL-OK' in p.stdout, p.stderr[-3000:]


def _cfg3():
    from backbones.ncsnpp_generator_adagn_feat import NCSNpp, NCSNpp_adaptive
    cfg = O.default_config()
    g1, g2 = NCSNpp(cfg), NCSNpp_adaptive(cfg)
    g1.load_state_dict(O.make_state_dict(cfg, 'g1', 1234))
    g2.load_state_dict(O.make_state_dict(cfg, 'g2', 1234))
    sl = load_golden('batch_cfg3.npz')['slices_u8'].float() / 255.0 * 2.0 - 1.0
    conds = [sl[:, c:c + 1].repeat(8, 1, 1, 1).contiguous().to(DEV) for c in range(3)]
    x_init, zs, noises = sampler_inputs(cfg, 32, seed_x=77)
    draws = (x_init.to(DEV), [z.to(DEV) for z in zs], [n.to(DEV) for n in noises])
    return cfg, g1.to(DEV).eval(), g2.to(DEV).eval(), conds, draws


def _graph_steps(cfg, g1, g2, conds, draws):
    from mudiff_hip import sampling as S
    sampler = S.GraphSampler(S.Posterior_Coefficients(cfg, DEV), g1, g2, cfg, 32, 256, 256, DEV)
    x_init, zs, noises = draws
    _, steps = sampler.sample(*conds, x_init, 4, zs=zs, noises=noises, return_steps=True)
    del sampler
    return steps


def _max_step_dev(sa, sb):
    return max(float((a - b).abs().max()) for xa, xb in zip(sa, sb) for a, b in zip(xa, xb))


def test_seeded_weights_keep_auto():
    """Config 3, B=32, T=4, seeded weights: the decision is 'auto' with nothing installed, the driver's RNG is untouched, and a
    GraphSampler built afterwards gives the same outputs as one built before.  In a child process with MUD_DETERMINISTIC=1: under
    the fp8 plan the default path's run-to-run jitter (fp64 atomics order, ~1 ulp) is re-rounded by the e4m3 images into
    differences of the plan's own size (3e-4 measured between two samplers), so 'the same outputs' is checked bit for bit on the
    deterministic path."""
    code = r'''
import json, torch
import test_precision_guard_gpu as T
from mudiff_hip import ops, precision, sampling as S
assert ops.DETERMINISTIC
cfg, g1, g2, conds, draws = T._cfg3()
before = T._graph_steps(cfg, g1, g2, conds, draws)
cpu_rng, gpu_rng = torch.get_rng_state(), torch.cuda.get_rng_state()
cal = precision.calibrate_plan(S.Posterior_Coefficients(cfg, T.DEV), g1, conds[0], g2, conds[1], conds[2], 4, cfg)
assert torch.equal(torch.get_rng_state(), cpu_rng) and torch.equal(torch.cuda.get_rng_state(), gpu_rng), "calibration used a shared RNG"
print(cal.summary())
print("per step max-abs (x_0_1, x_0_2, x_new) auto vs off:", [["%.2e" % v for v in s] for s in cal.steps["B"]])
print(f"seeded config 3, B=32: dev_B = {cal.dev_b:.3e}, {cal.census_launches} census launches, {cal.wall_s:.2f} s")
assert cal.decision == "auto" and cal.reverted == {} and cal.dev_b <= T.THRESH
assert precision.plan_overrides(g1) == [] and precision.plan_overrides(g2) == []
assert cal.census_launches > 0 and len(cal.steps["B"]) == 4
json.dumps(cal.to_dict())
after = T._graph_steps(cfg, g1, g2, conds, draws)
d = T._max_step_dev(before, after)
print(f"GraphSampler after calibration vs before: {d:.2e}")
assert d <= 1e-4 and all(torch.equal(a, b) for sa, sb in zip(before, after) for a, b in zip(sa, sb))
print("KEEP-AUTO-OK")
'''
    p = _child(code, dict(MUD_DETERMINISTIC='1'))
    assert p.returncode == 0 and 'KEEP-AUTO-OK' in p.stdout, p.stderr[-3000:]


def _boost_blocks(g, factor):
    """Scale the gamma half of the AdaGN style bias of the first two down-path and the last three up-path residual blocks
    (the 256x256 level): their conv inputs after AdaGN + SiLU reach into the thousands."""
    res = [e for e in g._plan if e['kind'] == 'res']
    chosen = [e['idx'] for e in res if e['stage'] == 'down'][:2] + [e['idx'] for e in res if e['stage'] == 'up'][-3:]
    for i in chosen:
        m = g.all_modules[i]
        for gn in (m.GroupNorm_0, m.GroupNorm_1):
            gn.style.bias.data[:gn.in_channel] *= factor
    return [f'all_modules.{i}.{c}' for i in chosen for c in ('Conv_0', 'Conv_1')]


def test_guard_trips_on_out_of_range_inputs():
    from mudiff_hip import ops, precision, sampling as S
    cfg, g1, g2, conds, draws = _cfg3()
    boosted = {'g1': _boost_blocks(g1, 1000.0), 'g2': _boost_blocks(g2, 1000.0)}
    coef = S.Posterior_Coefficients(cfg, DEV)
    x_init, zs, noises = draws
    cal = precision.calibrate_plan(coef, g1, conds[0], g2, conds[1], conds[2], 4, cfg, x_init=x_init, zs=zs, noises=noises)
    print(cal.summary())
    assert cal.dev_b > THRESH, f'precondition: the boosted blocks must push the auto plan over the threshold (dev_B {cal.dev_b:.2e})'
    for k, names in boosted.items():
        seen = [n for n in names if cal.census[k][n]['n'] > 0]
        print(k, {n: (cal.census[k][n]['n_over'], cal.census[k][n]['amax']) for n in seen})
        assert seen and all(cal.census[k][n]['n_over'] > 0 for n in seen)
    assert cal.decision in ('per_layer', 'off')
    if cal.decision == 'per_layer':
        for k, names in boosted.items():
            assert set(n for n in names if cal.census[k][n]['n'] > 0) <= set(cal.reverted[k])
        assert cal.dev_c <= THRESH
    for k, g in (('g1', g1), ('g2', g2)):
        assert precision.plan_overrides(g) == sorted(cal.reverted.get(k, []))
    with ops.prec_plan('off'):
        _, ref = S.sample_from_model(coef, g1, conds[0], g2, conds[1], conds[2], 4, x_init, None, cfg, zs=zs, noises=noises, return_steps=True)
    got = _graph_steps(cfg, g1, g2, conds, draws)
    d = _max_step_dev(ref, got)
    print(f'GraphSampler after calibration ({cal.decision}) vs the off plan: {d:.2e}')
    assert d <= (1e-4 if cal.decision == 'off' else THRESH)

    def fp8x_layers():
        with precision.census() as cs:
            S.sample_from_model(coef, g1, conds[0], g2, conds[1], conds[2], 1, x_init, None, cfg, zs=zs, noises=noises)
        return {k: set(t) for k, t in cs.table({'g1': g1._plan_scope, 'g2': g2._plan_scope}).items()}

    applied = {k: set(v) for k, v in cal.reverted.items()}
    on = fp8x_layers()
    assert all(not (on.get(k, set()) & applied[k]) for k in applied)       # the reverted layers run fp16 x 3
    g1.load_state_dict(g1.state_dict()); g2.load_state_dict(g2.state_dict())    # same tensors: the prepared caches are rebuilt
    assert fp8x_layers() == on                                              # ... and the overrides survive it
    precision.clear_plan(g1, g2)
    off = fp8x_layers()
    assert all(applied[k] <= off[k] for k in applied)                       # clear_plan restores the fp8x launches


def _write_volumes(root, n=6, hw=32, seed=5):
    rng = np.random.default_rng(seed)
    os.makedirs(os.path.join(root, 'test'), exist_ok=True)
    for mod in ('T1', 'T2', 'FLAIR', 'T1CE'):
        np.save(os.path.join(root, 'test', mod + '.npy'), (rng.standard_normal((n, hw, hw)) * 2).astype(np.float32))


def test_driver_calibrate_end_to_end(tmp_path):
    from mudiff_hip import driver
    from backbones.ncsnpp_generator_adagn_feat import NCSNpp, NCSNpp_adaptive
    data, out = tmp_path / 'data', tmp_path / 'out'
    _write_volumes(str(data))
    cfg = O.default_config(**SMALL_CFGS['s32'])
    # in process: calibrating on the first (padded) batch leaves the production predictions as they were
    g1, g2 = NCSNpp(cfg), NCSNpp_adaptive(cfg)
    g1.load_state_dict(O.make_state_dict(cfg, 'g1', 1234)); g2.load_state_dict(O.make_state_dict(cfg, 'g2', 1234))
    g1, g2 = g1.to(DEV).eval(), g2.to(DEV).eval()
    src = driver.SliceSource('test', str(data), 'T2')
    _, plain, _ = driver.sample_slices(cfg, g1, g2, src, 4, torch.device(DEV))
    cfg.calibrate_threshold = THRESH
    cal = driver.calibrate_first_batch(cfg, g1, g2, src, 4, torch.device(DEV), rank=1, world=2)     # rank 1: slices 3..5, padded to 4
    assert cal.shape == [4, 32, 32] and cal.decision in ('auto', 'per_layer', 'off')
    _, calibrated, _ = driver.sample_slices(cfg, g1, g2, src, 4, torch.device(DEV))
    assert float(np.abs(calibrated - plain).max()) <= 1e-4
    # the CLI
    os.makedirs(out / 'exp7')
    for which, name in (('g1', 'gen_diffusive_1'), ('g2', 'gen_diffusive_2')):
        torch.save({'module.' + k: v for k, v in O.make_state_dict(cfg, which, 1234).items()}, out / 'exp7' / f'{name}.pth')
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([REPO, PKG, os.environ.get('PYTHONPATH', '')]))
    for k in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE'):
        env.pop(k, None)
    cmd = [sys.executable, '-m', 'mudiff_hip.driver', '--input_path', str(data), '--output_path', str(out), '--exp', 'exp7', '--target_modality', 'T2',
           '--image_size', '32', '--num_channels_dae', '32', '--ch_mult', '1', '2', '4', '--attn_resolutions', '16', '--batch_size', '4',
           '--no_png', '--calibrate', '--calibrate_threshold', '4e-4']
    p = subprocess.run(cmd, cwd=REPO, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    assert 'fp8x precision calibration' in p.stderr and 'Average PSNR' in p.stderr
    rec = json.loads((out / 'prec_calibration.json').read_text())
    print({k: rec[k] for k in ('decision', 'dev_b', 'shape', 'wall_s')})
    assert rec['shape'] == [4, 32, 32] and rec['threshold'] == 4e-4 and rec['decision'] in ('auto', 'per_layer', 'off')
