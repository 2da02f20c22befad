"""CPU: the host side of the single-pass fp16 plan (MUD_PREC_16X1) - packed sizes per plan, the packer's refusal of 1x1 weights
(nothing launched), the plan name in ops, and the CLI flags (--prec_plan on both CLIs; --calibrate refused under the fp16 plan)."""
import ctypes as C
import os
import subprocess
import sys

import pytest

from conftest import PKG, REPO


def _lib():
    import mudiff_hip
    if not os.path.isfile(mudiff_hip.lib_path()):
        import __graft_entry__
        __graft_entry__.build()
    return mudiff_hip.load()


def test_packed_weight_bytes_per_plan():
    import mudiff_hip
    lib = _lib()
    assert (mudiff_hip.PREC_16X3, mudiff_hip.PREC_FP8X, mudiff_hip.PREC_16X1) == (0, 1, 2)
    for ks, cin, cout in ((3, 64, 64), (3, 48, 96), (3, 20, 200), (1, 64, 128), (1, 36, 40), (3, 512, 256)):
        full = lib.mud_packed_weight_bytes(ks, cin, cout)
        assert lib.mud_packed_weight_bytes_prec(ks, cin, cout, mudiff_hip.PREC_16X3) == full
        if ks == 3:
            assert lib.mud_packed_weight_bytes_prec(ks, cin, cout, mudiff_hip.PREC_FP8X) == full
            # hi-only: 64-channel tiles * 16-channel chunks * taps * one 2 KiB fp16 plane + two planes of DMA slack
            hi = lib.mud_packed_weight_bytes_prec(ks, cin, cout, mudiff_hip.PREC_16X1)
            assert hi == -(-cout // 64) * -(-cin // 16) * 9 * 2048 + 4096
            assert 2 * (hi - 4096) == full - 8192                  # half the bytes of a 16x3 step
        else:
            assert lib.mud_packed_weight_bytes_prec(ks, cin, cout, mudiff_hip.PREC_16X1) == -1
    assert lib.mud_packed_weight_bytes_prec(3, 64, 64, mudiff_hip.PREC_16X1) == 1 * 4 * 9 * 2048 + 4096
    assert lib.mud_packed_weight_bytes_prec(2, 64, 64, mudiff_hip.PREC_16X3) == -1
    assert lib.mud_packed_weight_bytes_prec(3, 64, 64, 7) == -1
    assert lib.mud_packed_weight_bytes_prec(3, 0, 64, mudiff_hip.PREC_16X1) == -1


def test_packer_refuses_1x1_under_the_fp16_plan_without_launching():
    import mudiff_hip
    lib = _lib()
    src = (C.c_float * 64)()
    dst = (C.c_uint8 * 8192)()
    d = (C.addressof(dst) + 15) & ~15                              # 16-byte aligned host address: never dereferenced
    code = lib.mud_pack_weights_prec(C.cast(src, C.c_void_p), 0, 8, 1, 0, 1, 8, 8, 1, mudiff_hip.PREC_16X1, 0, C.c_void_p(d), None)
    assert code == 1                                               # MUD_ERR_ARG, before anything is launched
    assert 'MUD_PREC_16X1' in lib.mud_last_error().decode()


def test_prec_plan_fp16_is_accepted_and_restored():
    from mudiff_hip import ops
    assert 'fp16' in ops.PREC_PLANS and ops.PREC_16X1 == 2
    before = ops.PREC_PLAN
    with ops.prec_plan('fp16'):
        assert ops.PREC_PLAN == 'fp16'
        with ops.prec_plan('off'):
            assert ops.PREC_PLAN == 'off'
        assert ops.PREC_PLAN == 'fp16'
    assert ops.PREC_PLAN == before
    with pytest.raises(ValueError, match='unknown plan'):
        ops.prec_plan('bf16')


def test_calibrate_plan_refuses_the_fp16_plan():
    import torch
    from mudiff_hip import ops, precision
    with ops.prec_plan('fp16'), pytest.raises(ValueError, match='fp16'):
        precision.calibrate_plan(None, None, torch.zeros(1, 1, 8, 8), None, None, None, 1, None)


_VOL = ['--target_modality', 'T1CE', '--output_dir', 'o', '--exp', 'e']


def test_both_clis_parse_prec_plan(monkeypatch):
    from mudiff_hip import driver, ops, volume
    monkeypatch.setattr(ops, 'PREC_PLAN', 'auto')
    for plan in ('auto', 'off', 'all', 'fp16'):
        assert driver.parse_args(['--prec_plan', plan]).prec_plan == plan
        assert volume.build_argparser(_VOL + ['--prec_plan', plan]).prec_plan == plan
    a = driver.parse_args([])
    assert a.prec_plan is None and driver.effective_prec_plan(a) == 'auto'            # default: whatever MUD_PREC_PLAN says
    assert volume.build_argparser(_VOL).prec_plan is None
    monkeypatch.setattr(ops, 'PREC_PLAN', 'off')
    assert driver.effective_prec_plan(driver.parse_args([])) == 'off'
    assert driver.effective_prec_plan(driver.parse_args(['--prec_plan', 'fp16'])) == 'fp16'
    with pytest.raises(SystemExit):
        driver.parse_args(['--prec_plan', 'bf16'])
    assert volume.build_argparser(_VOL + ['--use_bf16']).use_bf16                      # still accepted, still a no-op


def test_calibrate_with_the_fp16_plan_is_an_argparse_error(monkeypatch, capsys):
    from mudiff_hip import driver, ops, volume
    monkeypatch.setattr(ops, 'PREC_PLAN', 'auto')
    assert driver.parse_args(['--calibrate']).calibrate
    assert driver.parse_args(['--calibrate', '--prec_plan', 'off']).calibrate
    for parse in (driver.parse_args, lambda v: volume.build_argparser(_VOL + v)):
        with pytest.raises(SystemExit) as e:
            parse(['--calibrate', '--prec_plan', 'fp16'])
        assert e.value.code == 2 and '--calibrate' in capsys.readouterr().err
    monkeypatch.setattr(ops, 'PREC_PLAN', 'fp16')                  # the plan from MUD_PREC_PLAN (read by ops at import)
    for parse in (driver.parse_args, lambda v: volume.build_argparser(_VOL + v)):
        with pytest.raises(SystemExit):
            parse(['--calibrate'])
        assert '--calibrate' in capsys.readouterr().err
        assert parse(['--calibrate', '--prec_plan', 'auto']).prec_plan == 'auto'


@pytest.mark.parametrize('module,extra', [('mudiff_hip.driver', []), ('mudiff_hip.volume', _VOL)])
def test_calibrate_refused_when_the_environment_selects_fp16(module, extra):
    env = dict(os.environ, MUD_PREC_PLAN='fp16', PYTHONPATH=os.pathsep.join([REPO, PKG, os.environ.get('PYTHONPATH', '')]))
    p = subprocess.run([sys.executable, '-m', module, '--calibrate'] + extra, cwd=REPO, env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=300)
    assert p.returncode == 2 and '--calibrate' in p.stderr and 'fp16' in p.stderr, p.stderr[-2000:]
