"""Whole model with the up-sampling residual blocks' Conv_0 up-sampling its input while staging it (MUD_IN_UP2) on, against off: G2's
forward (eager) and captured reverse steps at 32x32, B = 2 - with the skip path's switch (MUD_RES_UP2) on and off."""
import pytest
import torch

from helpers import SMALL_CFGS, sampler_inputs, small_conds
from oracle import mudiff_oracle as O

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DEV = 'cuda:0'


def test_g2_forward_and_captured_steps_with_the_switch_on_and_off(monkeypatch):
    """Both forms compute the same function, and the fused launch stages the bits the FIR launch wrote (tests/test_in_up2.py); what
    remains between two whole passes is the ~1e-6 jitter of the producers' fp64 atomic GroupNorm statistics.  Bound 1e-5 max-abs on
    every output of every step (tests/test_res_up2_model.py's).  Every up block of G2 loses its h_in FIR launch, whatever the skip
    path's switch says.  Measured on MI355X: G2 forward 2.6e-6 (MUD_RES_UP2 on) and 2.0e-6 (off), the two captured steps 2.5e-6 and
    2.8e-6; fir_nhwc launches per G2 pass 5 -> 3 and 7 -> 5."""
    from backbones.ncsnpp_generator_adagn_feat import NCSNpp, NCSNpp_adaptive
    from backbones.layerspp import ResnetBlockBigGANpp_Adagn
    from mudiff_hip import ops, sampling as S
    cfg = O.default_config(**SMALL_CFGS['s32'])
    g1, g2 = NCSNpp(cfg), NCSNpp_adaptive(cfg)
    g1.load_state_dict(O.make_state_dict(cfg, 'g1', 1234))
    g2.load_state_dict(O.make_state_dict(cfg, 'g2', 1234))
    g1, g2 = g1.to(DEV).eval(), g2.to(DEV).eval()
    n_up = sum(isinstance(m, ResnetBlockBigGANpp_Adagn) and m.up for m in g2.modules())
    assert n_up >= 1
    B = 2
    conds = [c.to(DEV) for c in small_conds(cfg, B)]
    x_init, zs, noises = sampler_inputs(cfg, B)
    x, z, t = x_init.to(DEV), zs[0].to(DEV), torch.full((B,), 1, dtype=torch.int64, device=DEV)
    coef = S.Posterior_Coefficients(cfg, DEV)

    def run(on, res_on):
        monkeypatch.setattr(ops, 'IN_UP2', on)
        monkeypatch.setattr(ops, 'RES_UP2', res_on)
        y1 = g1(x, *conds, t, z)
        ops.PROFILE.enable()
        y2 = g2(x, *conds, t, z, y1)
        names = {k: v['n'] for k, v in ops.PROFILE.summary().items()}
        ops.PROFILE.disable()
        steps = None
        if res_on:
            sampler = S.GraphSampler(coef, g1, g2, cfg, B, cfg.image_size, cfg.image_size, DEV)
            _, steps = sampler.sample(*conds, x, 2, zs=[v.to(DEV) for v in zs[:2]], noises=[v.to(DEV) for v in noises[:2]], return_steps=True)
        return y2, steps, names

    drops = {}
    for res_on in (True, False):
        y_on, steps_on, n_on = run(True, res_on)
        y_off, steps_off, n_off = run(False, res_on)
        drops[res_on] = n_off['fir_nhwc'] - n_on['fir_nhwc']
        e_fwd = float((y_on - y_off).abs().max())
        print(f'MUD_IN_UP2 on vs off (MUD_RES_UP2 {"on" if res_on else "off"}): fir_nhwc {n_off["fir_nhwc"]} -> {n_on["fir_nhwc"]}, '
              f'gn_from_sums {n_off.get("gn_from_sums", 0)} -> {n_on.get("gn_from_sums", 0)}; G2 forward max-abs {e_fwd:.2e}')
        assert e_fwd <= 1e-5
        if res_on:
            e_steps = [max(float((a - b).abs().max()) for a, b in zip(s_on, s_off)) for s_on, s_off in zip(steps_on, steps_off)]
            print(f'  captured steps {", ".join(f"{e:.2e}" for e in e_steps)}')
            assert max(e_steps) <= 1e-5
    # the switch switches: one FIR launch per up block is gone, the same number with the skip path's switch on and off
    assert drops[True] == n_up and drops[False] == n_up, (drops, n_up)
