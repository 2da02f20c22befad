"""Whole model with the up-sampling residual blocks' skip path up-sampled on load (MUD_RES_UP2) on, against off: G2's forward
(eager) and captured reverse steps at 32x32, B = 2."""
import pytest
import torch

from helpers import SMALL_CFGS, sampler_inputs, small_conds
from oracle import mudiff_oracle as O

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DEV = 'cuda:0'


def test_g2_forward_and_captured_steps_with_the_switch_on_and_off(monkeypatch):
    """Both forms compute the same function and the residual is formed term for term as the FIR launch forms it (same bits per
    launch: tests/test_res_up2.py); what remains between two whole passes is the ~1e-6 jitter of the producers' fp64 atomic
    GroupNorm statistics (ops.DETERMINISTIC).  Bound 1e-5 max-abs on every output of every step.  Measured on MI355X: G2 forward
    2.3e-6, the two captured steps 2.9e-6 and 2.7e-6."""
    from backbones.ncsnpp_generator_adagn_feat import NCSNpp, NCSNpp_adaptive
    from mudiff_hip import ops, sampling as S
    cfg = O.default_config(**SMALL_CFGS['s32'])
    g1, g2 = NCSNpp(cfg), NCSNpp_adaptive(cfg)
    g1.load_state_dict(O.make_state_dict(cfg, 'g1', 1234))
    g2.load_state_dict(O.make_state_dict(cfg, 'g2', 1234))
    g1, g2 = g1.to(DEV).eval(), g2.to(DEV).eval()
    B = 2
    conds = [c.to(DEV) for c in small_conds(cfg, B)]
    x_init, zs, noises = sampler_inputs(cfg, B)
    x, z, t = x_init.to(DEV), zs[0].to(DEV), torch.full((B,), 1, dtype=torch.int64, device=DEV)
    coef = S.Posterior_Coefficients(cfg, DEV)

    def run(on):
        monkeypatch.setattr(ops, 'RES_UP2', on)
        y1 = g1(x, *conds, t, z)
        ops.PROFILE.enable()
        y2 = g2(x, *conds, t, z, y1)
        names = {k: v['n'] for k, v in ops.PROFILE.summary().items()}
        ops.PROFILE.disable()
        sampler = S.GraphSampler(coef, g1, g2, cfg, B, cfg.image_size, cfg.image_size, DEV)
        _, steps = sampler.sample(*conds, x, 2, zs=[v.to(DEV) for v in zs[:2]], noises=[v.to(DEV) for v in noises[:2]], return_steps=True)
        return y2, steps, names

    y_on, steps_on, n_on = run(True)
    y_off, steps_off, n_off = run(False)
    # the switch switches: the two skip-path FIR launches of a generator pass are gone
    assert n_off['fir_nhwc'] - n_on['fir_nhwc'] == 2, (n_off['fir_nhwc'], n_on['fir_nhwc'])
    e_fwd = float((y_on - y_off).abs().max())
    e_steps = [max(float((a - b).abs().max()) for a, b in zip(s_on, s_off)) for s_on, s_off in zip(steps_on, steps_off)]
    print(f'MUD_RES_UP2 on vs off: G2 forward max-abs {e_fwd:.2e}; captured steps {", ".join(f"{e:.2e}" for e in e_steps)}')
    assert e_fwd <= 1e-5 and max(e_steps) <= 1e-5
