"""The child process of the volume tests' end-to-end runs: python tests/volume_child.py plan.json

plan.json is what volume_support.run_plan wrote: dict(steps=[...], ignore=None | 'RuntimeWarning' | 'all', log=path).  The steps run in
the order given, in this one process (the library, the checkpoints and torch are loaded once), and what they printed is written to the
log: {name: stdout}, or {name: dict(stdout=, error=)} for a volume step that says whether it raises."""
import contextlib
import io
import json
import os
import sys
import warnings

import numpy as np
import torch

from mudiff_hip import cohort as Co, volume as V, volume_intake as VI, volume_regrid as VR


@contextlib.contextmanager
def captured(out, ignore):
    """stdout into `out`, under the plan's warnings filter."""
    with contextlib.redirect_stdout(out), (warnings.catch_warnings() if ignore else contextlib.nullcontext()):
        if ignore:
            warnings.simplefilter('ignore', RuntimeWarning if ignore == 'RuntimeWarning' else Warning)
        yield


@contextlib.contextmanager
def saving_stacks(path):
    """While it lasts, volume.predict_from_conditions saves the condition stacks it is given to `path` before it samples."""
    sample = V.predict_from_conditions

    def spy(args, plan, evaluation, gen1, gen2, device, stacks, ref, **kw):
        np.savez(path, *[s.cpu().numpy() if torch.is_tensor(s) else np.asarray(s) for s in stacks])
        return sample(args, plan, evaluation, gen1, gen2, device, stacks, ref, **kw)

    V.predict_from_conditions = spy
    try:
        yield
    finally:
        V.predict_from_conditions = sample


def run_volume(step, ignore, where):
    out, err = io.StringIO(), None
    spy = saving_stacks(f"{where}/stacks_{step['name']}.npz") if step.get('stacks') else contextlib.nullcontext()
    try:
        with captured(out, ignore), spy:
            args = V.build_argparser(step['argv'])
            for k in [k for k in vars(args) if k.startswith(tuple(step.get('strip', ())))]:      # the options as an older parser leaves them
                delattr(args, k)
            V.predict_volume(args)
    except ValueError as e:
        if 'raises' not in step:
            raise
        err = str(e)
    if 'raises' not in step:
        return out.getvalue()
    assert (err is not None) == step['raises'], (step['name'], err)
    return dict(stdout=out.getvalue(), error=err)


def run_cohort(step, ignore):
    out = io.StringIO()
    with captured(out, ignore):
        args = Co.build_argparser(step['argv'])
        failures = Co.run(args, Co.read_manifest(args.manifest))[1]
    assert not failures, failures
    return out.getvalue()


def run_regrid(step):
    """The offline resampling of one file onto the grid of another."""
    ref = VI.read_nifti_raw(step['ref'])
    world = VR.world_affine_of(ref.affine, ref.header)
    r = VR.regrid_to(VI.read_nifti_raw(step['src']), ref.shape, world, 'cuda:0', step['mode'])
    assert isinstance(r, VR.RegriddedVolume) and r.code == 16 and r.shape == ref.shape
    V.write_nifti(step['out'], r.values_float32(), ref.affine)


def main(plan_path):
    with open(plan_path) as f:
        plan = json.load(f)
    where = os.path.dirname(plan['log'])
    log = {}
    for step in plan['steps']:
        if step['kind'] == 'volume':
            log[step['name']] = run_volume(step, plan['ignore'], where)
        elif step['kind'] == 'cohort':
            log[step['name']] = run_cohort(step, plan['ignore'])
        else:
            assert step['kind'] == 'regrid', step
            run_regrid(step)
    with open(plan['log'], 'w') as f:
        json.dump(log, f)


if __name__ == '__main__':
    main(sys.argv[1])
