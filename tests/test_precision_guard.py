"""CPU: the precision guard of the fp8 cross-term plan (mudiff_hip.precision) - the decision rule on synthetic inputs, the census
ABI structs against gcc's layout, layer names from module structure, the JSON record, the CLI flags and the MAX merge over ranks
(gloo, world 2).  The census kernel and the calibration runs themselves: tests/test_precision_guard_gpu.py."""
import json
import os
import socket
import subprocess
import sys

import pytest
import torch
import torch.multiprocessing as mp

from conftest import PKG, REPO


def _c(n=100, over=0, under=0, f16=0, amax=1.0):
    return dict(n=n, n_over=over, n_under=under, n_fp16_over=f16, amax=amax)


TABLE = {'g1': {'all_modules.6.Conv_0': _c(over=3, amax=300.0), 'all_modules.6.Conv_1': _c(), 'all_modules.9.Conv_1': _c(f16=1, amax=7e4)},
         'g2': {'feat_att': _c(), 'all_modules.7.Conv_0': _c(under=5)}}


def test_decision_keeps_auto_at_and_below_the_threshold():
    from mudiff_hip.precision import decide
    assert decide(1e-4, TABLE, 5e-4) == ('auto', {})
    assert decide(5e-4, TABLE, 5e-4) == ('auto', {})              # exactly at the threshold: kept
    assert decide(5e-4, {}, 5e-4, dev_c=1.0) == ('auto', {})


def test_decision_reverts_exactly_the_flagged_layers():
    from mudiff_hip.precision import decide, flagged_layers
    want = {'g1': ['all_modules.6.Conv_0', 'all_modules.9.Conv_1']}       # n_over > 0 or n_fp16_over > 0; n_under alone is not a flag
    assert flagged_layers(TABLE) == dict(want, g2=[])
    assert decide(6e-4, TABLE, 5e-4) == ('pending', want)                   # run C with these reverted
    assert decide(6e-4, TABLE, 5e-4, dev_c=5e-4) == ('per_layer', want)
    assert decide(6e-4, TABLE, 5e-4, dev_c=2e-4, per_layer=False)[0] == 'off'


def test_decision_falls_back_to_off():
    from mudiff_hip.precision import decide
    every = {'g1': sorted(TABLE['g1']), 'g2': sorted(TABLE['g2'])}
    assert decide(6e-4, TABLE, 5e-4, dev_c=5.1e-4) == ('off', every)         # still over after the reverts
    clean = {g: {n: _c() for n in layers} for g, layers in TABLE.items()}
    assert decide(6e-4, clean, 5e-4) == ('off', every)                      # over, but nothing flagged
    assert decide(float('nan'), clean, 5e-4)[0] == 'off'
    idle = {'g1': {'a': _c(n=0), 'b': _c()}, 'g2': {'c': _c(n=0)}}         # layers that never ran fp8x are not reverted
    assert decide(1.0, idle, 5e-4) == ('off', {'g1': ['b']})


def test_decision_unchanged_when_the_plan_is_already_off(monkeypatch):
    from mudiff_hip import ops, precision
    assert precision.decide(1.0, TABLE, 5e-4, plan='off') == ('unchanged', {})
    monkeypatch.setattr(ops, 'PREC_PLAN', 'off')
    x = torch.zeros(2, 1, 8, 8)           # (host tensors: nothing may be launched)
    cal = precision.calibrate_plan(None, None, x, None, x, x, 4, None)
    assert cal.decision == 'unchanged' and cal.reverted == {} and cal.dev_b is None


def test_prec_plan_context_restores_the_plan(monkeypatch):
    from mudiff_hip import ops
    monkeypatch.setattr(ops, 'PREC_PLAN', 'auto')
    with ops.prec_plan('off'):
        assert ops.PREC_PLAN == 'off'
        with ops.prec_plan('all'):
            assert ops.PREC_PLAN == 'all'
        assert ops.PREC_PLAN == 'off'
    assert ops.PREC_PLAN == 'auto'
    with pytest.raises(ValueError):
        ops.prec_plan('fp8')


def test_census_structs_match_the_header_layout(tmp_path):
    import ctypes as C
    import mudiff_hip
    structs = {'mud_census_args': mudiff_hip.CensusArgs, 'mud_census_out': mudiff_hip.CensusOut}
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{os.path.join(REPO, "include", "mudiff_hip.h")}"', 'int main(void) {']
    for cname, cls in structs.items():
        lines.append(f'  printf("{cname} size %zu\\n", sizeof({cname}));')
        for fname, _ in cls._fields_:
            lines.append(f'  printf("{cname} {fname} %zu\\n", offsetof({cname}, {fname}));')
    lines += ['  return 0;', '}']
    src = tmp_path / 'layout.c'
    src.write_text('\n'.join(lines))
    exe = tmp_path / 'layout'
    subprocess.run(['gcc', '-std=c11', '-o', str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], check=True, stdout=subprocess.PIPE, text=True).stdout
    seen = 0
    for ln in out.strip().splitlines():
        cname, field, val = ln.split()
        cls = structs[cname]
        want = C.sizeof(cls) if field == 'size' else getattr(cls, field).offset
        assert int(val) == want, f'{cname}.{field}: header {val}, ctypes {want}'
        seen += 1
    assert seen == sum(len(c._fields_) + 1 for c in structs.values())
    from mudiff_hip import ops
    assert [f for f, _ in mudiff_hip.CensusOut._fields_] == list(ops.CENSUS_FIELDS) and C.sizeof(mudiff_hip.CensusOut) == 40


@pytest.mark.parametrize('cfg_kw', [dict(), dict(ch_mult=[1, 1, 2, 2, 4], num_timesteps=8)], ids=['config2', 'config5'])
def test_conv_layer_names_are_state_dict_prefixes(cfg_kw):
    from oracle import mudiff_oracle as O
    from mudiff_hip import precision
    from backbones.ncsnpp_generator_adagn_feat import GATES_NAME, NCSNpp, NCSNpp_adaptive
    cfg = O.default_config(**cfg_kw)
    for cls in (NCSNpp, NCSNpp_adaptive):
        g = cls(cfg)
        names, sd = precision.conv_layer_names(g), g.state_dict()
        assert len(names) == len(set(names)) > 20
        for n in names:
            if n == GATES_NAME:            # the merged gate conv: every feat_att1_* / feat_att2_* of the state_dict
                assert cls is NCSNpp_adaptive and any(k.startswith('feat_att1_') for k in sd) and any(k.startswith('feat_att2_') for k in sd)
            else:
                assert n + '.weight' in sd and sd[n + '.weight'].shape[-2:] == (3, 3), n
        r = next(e['idx'] for e in g._plan if e['kind'] == 'res')       # the first residual block
        assert f'all_modules.{r}.Conv_0' in names and f'all_modules.{r}.Conv_1' in names
        assert (GATES_NAME in names) == (cls is NCSNpp_adaptive)
        assert not any(n.endswith('Conv_2') for n in names)           # 1x1 skips never run the fp8x plan
        # the overrides live on the generator by name; every _Prepared block is bound to that one scope under its prefix
        assert g.all_modules[r].__dict__['_plan_bound'] == (g._plan_scope, f'all_modules.{r}.')
        precision.set_plan(g, names[:3])
        assert precision.plan_overrides(g) == sorted(names[:3])
        g.load_state_dict(sd)
        assert precision.plan_overrides(g) == sorted(names[:3])
        precision.clear_plan(g)
        assert precision.plan_overrides(g) == []


def test_calibration_record_round_trips_through_json():
    from mudiff_hip.precision import Calibration
    cal = Calibration('per_layer', 5e-4, (32, 256, 256), 0)
    cal.dev_b, cal.dev_c = 1.2e-3, 3.1e-4
    cal.steps = {'B': [[1e-4, 2e-4, 1.2e-3]] * 4, 'C': [[1e-4, 2e-4, 3.1e-4]] * 4}
    cal.census = TABLE
    cal.reverted = {'g1': ['all_modules.6.Conv_0']}
    cal.census_launches, cal.wall_s = 180, 12.5
    d = cal.to_dict()
    back = json.loads(json.dumps(d))
    assert back == d
    assert back['decision'] == 'per_layer' and back['reverted'] == {'g1': ['all_modules.6.Conv_0']} and back['shape'] == [32, 256, 256]
    assert back['census']['g1']['all_modules.9.Conv_1']['n_fp16_over'] == 1 and back['steps']['C'][3][2] == 3.1e-4
    assert 'decision=per_layer' in cal.summary()


def test_calibrate_flags_parse_in_both_clis():
    from mudiff_hip import driver, volume
    a = driver.build_parser().parse_args([])
    assert a.calibrate is False and a.calibrate_threshold == 5e-4
    a = driver.build_parser().parse_args(['--calibrate', '--calibrate_threshold', '2e-4'])
    assert a.calibrate is True and a.calibrate_threshold == 2e-4
    base = ['--target_modality', 'T1', '--output_dir', 'out', '--exp', 'e']
    v = volume.build_argparser(base)
    assert v.calibrate is False and v.calibrate_threshold == 5e-4
    v = volume.build_argparser(base + ['--calibrate', '--calibrate_threshold', '1e-4'])
    assert v.calibrate is True and v.calibrate_threshold == 1e-4


# ---- the merge over ranks (gloo, world 2, plain tensors) --------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        return s.getsockname()[1]


def _merge_worker(rank, world, port, q):
    for p in (REPO, PKG):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch.distributed as dist
    from mudiff_hip import precision
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        names = {'g1': ['a', 'b', 'c'], 'g2': ['feat_att']}
        if rank == 0:      # rank 0: under the threshold, layer a saturates;  rank 1: over it, layer c saturates its fp16 piece, 'b' never ran
            devs, table = [3e-4], {'g1': {'a': _c(over=2, amax=200.0), 'b': _c(), 'c': _c()}, 'g2': {'feat_att': _c()}}
        else:
            devs, table = [9e-4], {'g1': {'a': _c(), 'c': _c(f16=4, amax=7e4)}, 'g2': {'feat_att': _c(under=3)}}
        mdevs, mtable = precision.merge_over_ranks(devs, table, names, group=dist.group.WORLD)
        (dc,), _ = precision.merge_over_ranks([2e-4 * (1 + rank)], {}, {}, group=dist.group.WORLD)
        q.put((rank, mdevs, mtable, dc, precision.decide(mdevs[0], mtable, 5e-4), precision.decide(mdevs[0], mtable, 5e-4, dev_c=dc)))
    finally:
        dist.destroy_process_group()


def test_group_merge_is_a_max_and_every_rank_decides_the_same():
    world = 2
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_merge_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=120) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    (_, d0, t0, c0, p0, f0), (_, d1, t1, c1, p1, f1) = res
    assert d0 == d1 == [9e-4] and c0 == c1 == 4e-4
    assert t0 == t1
    assert t0['g1']['a'] == _c(over=2, amax=200.0) and t0['g1']['c'] == _c(f16=4, amax=7e4) and t0['g2']['feat_att'] == _c(under=3)
    assert t0['g1']['b'] == _c()                                          # seen on rank 0 only
    assert p0 == p1 == ('pending', {'g1': ['a', 'c']})
    assert f0 == f1 == ('per_layer', {'g1': ['a', 'c']})
