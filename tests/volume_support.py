"""What the volume tests share: the tiny model, the child process of the end-to-end runs and a few small helpers.

The whole end-to-end fixture of a stage's GPU test (tests/test_volume_denoise_gpu.py is the model):

    @pytest.fixture(scope='module')
    def runs(tmp_path_factory):
        tmp = tmp_path_factory.mktemp('noisy')
        write_tiny_model(tmp)
        ...                                                 # write the stage's phantoms: p = {'flair': ..., 't2': ..., 't1': ...}
        model = model_argv(tmp, 2, 5, '--resize_back', '--input_flair', p['flair'], '--input_t2', p['t2'], '--input_t1', p['t1'])
        jobs = {'den_host': ['--denoise'], 'den_dev': ['--denoise', '--device_intake'], 'plain_host': []}
        steps = [volume_step(k, model + a + ['--output_dir', str(tmp / k)]) for k, a in jobs.items()]
        log = run_plan(tmp, steps, 900, ignore='RuntimeWarning')            # one fresh process: tests/volume_child.py
        return dict(tmp=tmp, log=log, pred=lambda k: payload(str(tmp / k / 'predicted_t1ce.nii.gz')))

and a test reads done_line(runs['log']['den_host']), runs['pred']('den_host') and the files under runs['tmp']."""
import gzip
import json
import os
import subprocess
import sys

import numpy as np

from conftest import PKG, REPO
from volume_intake_ref import CODES

DEV = 'cuda:0'
TINY_MODEL = dict(image_size=16, num_channels_dae=16, ch_mult=[1, 2], attn_resolutions=(4,), num_res_blocks=1)
CHILD = os.path.join(REPO, 'tests', 'volume_child.py')


# ---------------------------------------------------------------------------------------------------
# the tiny model
# ---------------------------------------------------------------------------------------------------
def write_tiny_model(tmp):
    """The two generators' checkpoints (seed 9) under tmp/results/exp0, where model_argv(tmp, ...) points."""
    import torch
    from oracle import mudiff_oracle as O
    cfg = O.default_config(**TINY_MODEL)
    exp = tmp / 'results' / 'exp0'
    exp.mkdir(parents=True)
    for which, name in (('g1', 'gen_diffusive_1'), ('g2', 'gen_diffusive_2')):
        torch.save({'module.' + k: v for k, v in O.make_state_dict(cfg, which, 9).items()}, str(exp / f'{name}.pth'))


def model_argv(tmp, half_range, batch_size, *extra):
    return ['--target_modality', 'T1CE', '--exp', 'exp0', '--output_path', str(tmp / 'results'), '--image_size', '16', '--num_channels_dae',
            '16', '--ch_mult', '1', '2', '--attn_resolutions', '4', '--num_res_blocks', '1', '--slice_half_range', str(half_range),
            '--batch_size', str(batch_size), '--seed', '31'] + list(extra)


def cli_argv(*extra):
    """The least the volume parser accepts (host tests of the flags)."""
    return ['--target_modality', 'T1CE', '--output_dir', 'out', '--exp', 'e'] + list(extra)


# ---------------------------------------------------------------------------------------------------
# child processes
# ---------------------------------------------------------------------------------------------------
def child_env():
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([REPO, PKG, os.environ.get('PYTHONPATH', '')]), MUD_DETERMINISTIC='1')
    for k in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE'):
        env.pop(k, None)
    return env


def run_module(module, argv, expect=0, timeout=900):
    """python -m module argv in a fresh process -> the CompletedProcess (text)."""
    p = subprocess.run([sys.executable, '-m', module] + argv, cwd=REPO, env=child_env(), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                       timeout=timeout)
    assert p.returncode == expect, (p.returncode, p.stdout[-3000:], p.stderr[-3000:])
    return p


def volume_step(name, argv, **options):
    """predict_volume(argv), its stdout logged under `name`.  Options: raises=bool (a ValueError is expected, or must not come: the log
    entry is dict(stdout=, error=)), strip=[prefixes] (attributes deleted from the parsed options), stacks=True (the condition stacks
    are saved to stacks_<name>.npz)."""
    return dict(kind='volume', name=name, argv=argv, **options)


def cohort_step(name, argv):
    """cohort.run on argv's manifest, no failures allowed, its stdout logged under `name`."""
    return dict(kind='cohort', name=name, argv=argv)


def regrid_step(src, ref, out, mode='linear'):
    """volume_regrid.regrid_to of the file src onto the grid of the file ref, written to out."""
    return dict(kind='regrid', src=src, ref=ref, out=out, mode=mode)


def run_plan(tmp, steps, timeout, ignore=None):
    """Runs the steps, in order, in one fresh process (tests/volume_child.py) -> {name: what the step logged}.  ignore: the warnings
    filter around every volume and cohort step: None, 'RuntimeWarning' or 'all'."""
    assert ignore in (None, 'RuntimeWarning', 'all')
    plan, log = str(tmp / 'plan.json'), str(tmp / 'log.json')
    with open(plan, 'w') as f:
        json.dump(dict(steps=steps, ignore=ignore, log=log), f)
    c = subprocess.run([sys.executable, CHILD, plan], cwd=REPO, env=child_env(), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                       timeout=timeout)
    assert c.returncode == 0, c.stdout[-3000:] + c.stderr[-3000:]
    with open(log) as f:
        return json.load(f)


def load_stacks(tmp, name):
    """The condition stacks a volume step with stacks=True saved, in their order."""
    return [v for _, v in sorted(np.load(str(tmp / f'stacks_{name}.npz')).items(), key=lambda kv: int(kv[0].split('_')[1]))]


# ---------------------------------------------------------------------------------------------------
# small helpers
# ---------------------------------------------------------------------------------------------------
def payload(path):
    """The bytes inside a .gz file (a NIfTI without the gzip header's time stamp)."""
    with gzip.open(path, 'rb') as f:
        return f.read()


def done_lines(text, count=1):
    lines = [ln for ln in text.splitlines() if ln.startswith('[done]')]
    assert len(lines) == count
    return lines


def done_line(text):
    """The single [done] line of one run's stdout."""
    return done_lines(text)[0]


def raw_volume(vol, scale=(1.0, 0.0), affine=None):
    """A RawVolume of the stored [X,Y,Z] array, little-endian, with the slope and intercept a header would hold."""
    from mudiff_hip import volume_intake as VI
    return VI.RawVolume(np.ascontiguousarray(vol.reshape(-1, order='F')), CODES[vol.dtype.str[1:]], '<', float(np.float32(scale[0])),
                        float(np.float32(scale[1])), vol.shape, np.eye(4) if affine is None else affine, None)


def to_device_zyx(a, dtype=None, device=DEV):
    """[X,Y,Z] host array -> [Z,Y,X] device tensor."""
    import torch
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype).transpose(2, 1, 0))).to(device)


def to_host_xyz(t):
    """[Z,Y,X] device tensor -> [X,Y,Z] host array."""
    return t.cpu().numpy().transpose(2, 1, 0)
