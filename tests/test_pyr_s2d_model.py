"""Whole model with the input pyramid's FIR + stride-2 conv folded into one 3x3 launch on the space-to-depth view (MUD_PYR_S2D) on,
against off: G1 and G2 forward (eager) and two captured reverse steps at 32x32, B = 2, both against the CPU oracle."""
import pytest
import torch

from helpers import SMALL_CFGS, sampler_inputs, small_conds
from oracle import mudiff_oracle as O

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DEV = 'cuda:0'


def test_g1_g2_forward_and_captured_steps_with_the_switch_on_and_off(monkeypatch):
    """The folded launch computes the same operator with once-rounded composed weights (per-launch error: tests/test_pyr_s2d.py), so
    the model's deviation from the fp64-free CPU oracle may move only by what two whole passes differ by anyway - the ~1e-6 jitter
    of the producers' fp64 atomic GroupNorm statistics: switched on, no output of G1, G2 or either captured step may deviate from the
    oracle by more than the switched-off run does + 1e-5 (tests/test_in_up2_model.py's bar).  The launch record shows ONE pyramid
    launch per generator pass, at the folded size, and the pass has one fir_nhwc launch fewer."""
    from backbones.ncsnpp_generator_adagn_feat import NCSNpp, NCSNpp_adaptive
    from mudiff_hip import ops, precision, sampling as S
    cfg = O.default_config(**SMALL_CFGS['s32'], num_timesteps=2)
    sd1, sd2 = O.make_state_dict(cfg, 'g1', 1234), O.make_state_dict(cfg, 'g2', 1234)
    g1, g2 = NCSNpp(cfg), NCSNpp_adaptive(cfg)
    g1.load_state_dict(sd1)
    g2.load_state_dict(sd2)
    g1, g2 = g1.to(DEV).eval(), g2.to(DEV).eval()
    B = 2
    conds = small_conds(cfg, B)
    x_init, zs, noises = sampler_inputs(cfg, B)
    t = torch.full((B,), 1, dtype=torch.int64)
    r1 = O.g1_forward(sd1, cfg, x_init, *conds, t, zs[0])
    r2 = O.g2_forward(sd2, cfg, x_init, *conds, t, zs[0], r1)
    _, r_steps = O.sample_from_model(O.PosteriorCoefficients(cfg), sd1, sd2, cfg, *conds, x_init, zs, noises, return_steps=True)
    dconds, dx, dt = [c.to(DEV) for c in conds], x_init.to(DEV), t.to(DEV)
    coef = S.Posterior_Coefficients(cfg, DEV)

    def run(on):
        monkeypatch.setattr(ops, 'PYR_S2D', on)
        recs, firs = [], []
        y1 = None
        for net in (g1, g2):
            ops.PROFILE.enable()
            with precision.launch_record() as rec:
                y = net(dx, *dconds, dt, zs[0].to(DEV)) if net is g1 else net(dx, *dconds, dt, zs[0].to(DEV), y1)
            firs.append(ops.PROFILE.summary().get('fir_nhwc', {'n': 0})['n'])
            ops.PROFILE.disable()
            recs.append(rec.launches)
            if net is g1:
                y1 = y
        sampler = S.GraphSampler(coef, g1, g2, cfg, B, cfg.image_size, cfg.image_size, DEV)
        _, steps = sampler.sample(*dconds, dx, 2, zs=[v.to(DEV) for v in zs], noises=[v.to(DEV) for v in noises], return_steps=True)
        dev = [float((y1.cpu() - r1).abs().max()), float((y.cpu() - r2).abs().max())]
        dev += [max(float((a.cpu() - b).abs().max()) for a, b in zip(s, r)) for s, r in zip(steps, r_steps)]
        return dev, recs, firs

    d_on, rec_on, fir_on = run(True)
    d_off, rec_off, fir_off = run(False)
    names = ('G1 forward', 'G2 forward', 'captured step 1', 'captured step 2')
    for n, a, b in zip(names, d_on, d_off):
        print(f'MUD_PYR_S2D {n}: max-abs vs the CPU oracle on {a:.3e}, off {b:.3e}')
    for a, b in zip(d_on, d_off):
        assert a <= b + 1e-5, (d_on, d_off)
    nf = cfg.num_channels_dae
    for which in range(2):
        pyr_on = [r for r in rec_on[which] if r.mfma and r.sub2]
        pyr_off = [r for r in rec_off[which] if r.mfma and r.sub2]
        # one matrix-core pyramid launch per pass either way (the 1-channel level-0 down-sampler is a direct convolution): folded,
        # it runs at [B, 8, 8, 4 * 32] -> 64; unfolded, on the padded 17 x 17 image
        assert len(pyr_on) == 1 and len(pyr_off) == 1 and pyr_on[0].layer == pyr_off[0].layer
        assert pyr_on[0].shape == (B, 8, 8, 4 * nf, 2 * nf) and pyr_off[0].shape == (B, 17, 17, nf, 2 * nf), (pyr_on, pyr_off)
        assert pyr_on[0].prec == pyr_off[0].prec == ops.PREC_16X3
        assert pyr_on[0].s2d and not pyr_off[0].s2d          # (Launch.sub2 names the stride-2 form, Launch.s2d how it is computed)
        assert fir_off[which] - fir_on[which] == 1, (fir_off, fir_on)
        assert len(rec_on[which]) == len(rec_off[which])
