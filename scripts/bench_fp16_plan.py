"""The single-pass fp16 plan (MUD_PREC_PLAN=fp16, MUD_PREC_16X1) against the default plan ('auto') at BASELINE config 3 (256x256,
nf=64): slices/s of two captured samplers - one captured under each plan - on the same slices, alternated in one process, at
batch 32 and at batch 1; and a per-shape A/B of the 3x3 launches of a batch-32 G1 + G2 pass (the shapes of scripts/ab_prec.py:
the plan 'auto' gives that shape against MUD_PREC_16X1, interleaved rounds).  Prints one JSON line.

    python scripts/bench_fp16_plan.py [--slices 64] [--iters 3] [--rounds 5]
    rocprofv3 --kernel-trace --stats -d <dir> -o fp16 -- python scripts/bench_fp16_plan.py --iters 1 --rounds 1"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, 'mu-diff_amd')):
    if p not in sys.path:
        sys.path.insert(0, p)

from bench import bench_config, build_models, synthetic_batch  # noqa: E402
from mudiff_hip import ops  # noqa: E402
from mudiff_hip import sampling as S  # noqa: E402
from mudiff_hip.driver import pad_batch  # noqa: E402

# (H, Cin, Cout, prologue: 0 none / 2 AdaGN + SiLU, residual, fused skip conv, launches per G1 + G2 pass)
SHAPES = [(256, 192, 384, 0, 0, 0, 1), (256, 320, 64, 2, 0, 1, 2), (256, 256, 64, 2, 0, 1, 2), (256, 192, 64, 2, 0, 1, 2), (256, 128, 64, 2, 0, 1, 2),
          (256, 128, 128, 2, 1, 0, 2), (256, 128, 128, 0, 0, 0, 2), (256, 64, 64, 2, 0, 0, 12), (256, 64, 64, 2, 1, 0, 10),
          (128, 256, 256, 2, 1, 0, 2), (128, 256, 256, 0, 0, 0, 2), (128, 384, 128, 2, 0, 1, 2), (128, 256, 128, 2, 0, 1, 2), (128, 192, 128, 2, 0, 1, 2),
          (128, 128, 128, 2, 1, 0, 10), (128, 64, 128, 2, 0, 1, 2),
          (64, 512, 256, 2, 0, 1, 4), (64, 384, 256, 2, 0, 1, 2), (64, 256, 256, 2, 1, 0, 14), (64, 256, 256, 2, 0, 0, 6), (64, 128, 256, 2, 0, 1, 2)]


def timed_us(fn, n=5):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


def sampler_rates(cfg, g1, g2, conds, B, iters, dev):
    """slices/s of the 'auto' and the 'fp16' sampler on the same slices, alternated."""
    H, n = cfg.image_size, conds[0].shape[0]
    coef = S.Posterior_Coefficients(cfg, dev)
    samplers = {}
    for plan in ('auto', 'fp16'):
        with ops.prec_plan(plan):
            samplers[plan] = S.GraphSampler(coef, g1, g2, cfg, B, H, H, dev)
    gen = torch.Generator(device=dev).manual_seed(0)
    x0 = torch.randn(B, 1, H, H, device=dev, generator=gen)

    def run(plan):
        for b0 in range(0, n, B):
            cs = [pad_batch(c[b0:b0 + B], min(B, n - b0), B) for c in conds]
            samplers[plan].sample(*cs, x0, cfg.num_timesteps, generator=gen)

    for plan in samplers:
        run(plan)
    torch.cuda.synchronize()
    ts = {p: [] for p in samplers}
    for _ in range(iters):
        for plan in samplers:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(plan)
            torch.cuda.synchronize()
            ts[plan].append(time.perf_counter() - t0)
    return {p: n / min(v) for p, v in ts.items()}, {p: [round(t, 4) for t in v] for p, v in ts.items()}


def per_shape(B, rounds, dev):
    rows, tot = [], {'auto': 0.0, 'fp16': 0.0}
    for H, Cin, Cout, pro, res, skip, cnt in SHAPES:
        g = torch.Generator(device=dev).manual_seed(H + Cin + Cout)
        x = ops.View(torch.randn(B, H, H, Cin, device=dev, generator=g), B, H, H, Cin)
        w = torch.randn(Cout, Cin, 3, 3, device=dev, generator=g) / math.sqrt(Cin * 9)
        w1 = torch.randn(Cout, Cin, 1, 1, device=dev, generator=g) / math.sqrt(Cin)
        sc, sh = torch.rand(B, Cin, device=dev, generator=g) + 0.5, torch.randn(B, Cin, device=dev, generator=g)
        prol = (sc, sh, ops.PRO_AFFINE_SILU) if pro == 2 else None
        r = ops.View(torch.randn(B, H, H, Cout, device=dev, generator=g), B, H, H, Cout) if res else None
        b2 = torch.randn(B, Cout, device=dev, generator=g)
        out, so = ops.View.empty(B, H, H, Cout, dev), ops.View.empty(B, H, H, Cout, dev)
        kw = dict(mfma=True, pro=prol, bias2=b2, res=r, out_scale=0.7071 if res else 1.0, skip=(ops.pack_conv_weight(w1), None, so) if skip else None)
        mode = ops.PRO_AFFINE_SILU if pro == 2 else ops.PRO_NONE
        with ops.prec_plan('auto'):
            pa = ops.choose_prec(x, Cout, mode, skip=bool(skip))
        we = ops.fp8x_weight_exponent(w) if pa == ops.PREC_FP8X else 0
        wa = ops.pack_conv_weight(w, prec=pa, w_exp=we)
        w16 = ops.pack_conv_weight(w, prec=ops.PREC_16X1)
        runs = {'auto': lambda: ops.conv(x, wa, 3, Cout, out=out, prec=pa, w_exp=we, **kw),
                'fp16': lambda: ops.conv(x, w16, 3, Cout, out=out, prec=ops.PREC_16X1, **kw)}
        for fn in runs.values():
            fn()
        torch.cuda.synchronize()
        ts = {k: [] for k in runs}
        for _ in range(rounds):
            for k, fn in runs.items():
                ts[k].append(timed_us(fn))
        med = {k: float(np.median(v)) for k, v in ts.items()}
        for k in tot:
            tot[k] += med[k] * cnt
        rows.append(dict(H=H, cin=Cin, cout=Cout, pro=pro, res=res, skip=skip, per_pass=cnt, auto_plan={0: '16x3', 1: 'fp8x'}[pa],
                         auto_us=round(med['auto'], 1), fp16_us=round(med['fp16'], 1), speedup=round(med['auto'] / med['fp16'], 3),
                         fp16_tflops=round(2.0 * B * H * H * Cout * Cin * 9 / med['fp16'] / 1e6, 1)))
    return rows, tot


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--slices', type=int, default=64)
    ap.add_argument('--slices_b1', type=int, default=8)
    ap.add_argument('--iters', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=5)
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    torch.cuda.set_device(dev)
    cfg = bench_config()
    g1, g2, _ = build_models(cfg, dev, 0, 1)
    conds = synthetic_batch(cfg, a.slices, dev, seed=100)
    r32, t32 = sampler_rates(cfg, g1, g2, conds, 32, a.iters, dev)
    r1, t1 = sampler_rates(cfg, g1, g2, [c[:a.slices_b1] for c in conds], 1, a.iters, dev)
    rows, tot = per_shape(32, a.rounds, dev)
    print(json.dumps(dict(
        config=3, slices=a.slices, b32_auto_slices_per_s=round(r32['auto'], 3), b32_fp16_slices_per_s=round(r32['fp16'], 3),
        b32_speedup=round(r32['fp16'] / r32['auto'], 4), b32_s=t32, b1_slices=a.slices_b1, b1_auto_slices_per_s=round(r1['auto'], 3),
        b1_fp16_slices_per_s=round(r1['fp16'], 3), b1_speedup=round(r1['fp16'] / r1['auto'], 4), b1_s=t1,
        per_shape_b32=rows, weighted_pass_ms=dict(auto=round(tot['auto'] / 1e3, 3), fp16=round(tot['fp16'] / 1e3, 3)),
        slowest_shape_speedup=min(r['speedup'] for r in rows))))


if __name__ == '__main__':
    main()
