"""On-device LPIPS-alex at the evaluation size of the issue: N slice pairs of H x W (default 1024 of 256x256) with seeded weights.
Prints one JSON line: the per-launch-sequence device time of ops.lpips_u8 (HIP events), per-kernel event times of one call, and the
wall time of metrics.score_device(..., lpips=net) (quantise + PSNR / SSIM / MAE + LPIPS, host sync included).

    python scripts/bench_lpips.py [--n 1024] [--size 256] [--iters 5]
    rocprofv3 --kernel-trace --stats -d <dir> -o lpips -- python scripts/bench_lpips.py --iters 2      # device time per kernel"""
import argparse
import json
import os
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, 'mu-diff_amd')):
    if p not in sys.path:
        sys.path.insert(0, p)

from mudiff_hip import metrics, ops  # noqa: E402
from mudiff_hip.lpips_net import CONV_SHAPES, LpipsAlex  # noqa: E402


def seeded_net(seed=0):
    g = torch.Generator().manual_seed(seed)
    w = [torch.randn(*s, generator=g) * (2.0 / (s[1] * s[2] * s[3])) ** 0.5 for s in CONV_SHAPES]
    b = [(torch.rand(s[0], generator=g) - 0.5) * 0.2 for s in CONV_SHAPES]
    lin = [torch.rand(s[0], generator=g) * 0.2 for s in CONV_SHAPES]
    return LpipsAlex(w, b, lin)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=1024)
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--iters', type=int, default=5)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    n, H = args.n, args.size
    net = seeded_net().to(dev)
    g = torch.Generator(device=dev).manual_seed(1)
    gts = torch.rand(n, H, H, device=dev, generator=g) * 2 - 1
    preds = (gts + 0.1 * torch.randn(n, H, H, device=dev, generator=g)).clamp(-1.2, 1.1)
    p8, g8 = ops.quantize_u8(preds, -1.2, 1.1), ops.quantize_u8(gts, -1.2, 1.1)
    ops.lpips_u8(p8, g8, net)                                            # warm-up (and workspace allocation)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for _ in range(args.iters):
        e0.record()
        out = ops.lpips_u8(p8, g8, net)
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    walls = []
    for _ in range(max(2, args.iters // 2)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = metrics.score_device(preds, gts, lpips=net)
        walls.append((time.perf_counter() - t0) * 1e3)
    flop = 3.47e9 * n * (H * H / 65536.0)
    print(json.dumps(dict(n=n, size=H, lpips_ms=min(times), lpips_ms_all=[round(t, 3) for t in times],
                          tflops=flop / (min(times) * 1e-3) / 1e12, score_device_lpips_wall_ms=min(walls),
                          mean_lpips=res['lpips'], chunks=int(-(-n // max(1, ops.LPIPS_WS_CAP // ops.load().mud_lpips_ws_bytes(1, H, H)))),
                          finite=bool(torch.isfinite(out).all()))))


if __name__ == '__main__':
    main()
