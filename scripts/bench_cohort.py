"""End-to-end per-subject wall time of the volume pipeline on a synthetic cohort, two ways in ONE process:

  (A) one `mudiff_hip.volume.predict_volume` per subject, as separate runs would do it short of the interpreter start: host intake
      (numpy), a fresh model, fresh weight packing and a freshly captured sampler for every subject;
  (B) `mudiff_hip.cohort` over the same subjects: model and sampler once, device intake and re-assembly, reads and writes on threads.

The cohort: --subjects (8) subjects of 240 x 240 x 155, int16, gzip, an ellipsoidal non-zero region (about a quarter of the voxels) with
integer intensities; BASELINE config 3's model (256 x 256, nf = 64, batches of 32) with seeded weights, --resize_back.  Writes
profiles/cohort_bench.json (or --out): subjects/s, per-stage seconds and the GPU-busy share (sampling seconds / wall) of both, and
whether the files of (A) and (B) are identical.  One pass each, no repetitions: the numbers are what one run of each costs.

--norm is passed through to both (mudiff_hip.volume's flag): with `zscore` (B)'s stage table gains the prefetch
threads' moments seconds and read_wait, the main thread's seconds waiting for a read (moments included).

    python scripts/bench_cohort.py [--subjects 8] [--norm percentile] [--out profiles/cohort_bench.json]"""
import argparse
import gzip
import json
import os
import struct
import sys
import tempfile
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, 'mu-diff_amd')):
    if p not in sys.path:
        sys.path.insert(0, p)

from bench import bench_config, random_weights_  # noqa: E402
from mudiff_hip import cohort as Co  # noqa: E402
from mudiff_hip import volume as V  # noqa: E402
from mudiff_hip import volume_intake as VI  # noqa: E402

SHAPE = (240, 240, 155)


def write_int16_nifti(path, vol):
    """Single-file NIfTI-1, int16, gzip level 1 (building the cohort is not what is timed)."""
    raw = bytearray(348)
    struct.pack_into('<i', raw, 0, 348)
    struct.pack_into('<8h', raw, 40, 3, *vol.shape, 1, 1, 1, 1)
    struct.pack_into('<h', raw, 70, 4)
    struct.pack_into('<h', raw, 72, 16)
    struct.pack_into('<8f', raw, 76, *([1.0] * 8))
    struct.pack_into('<f', raw, 108, 352.0)
    struct.pack_into('<h', raw, 254, 1)
    for r in range(3):
        struct.pack_into('<4f', raw, 280 + 16 * r, *[1.0 if c == r else 0.0 for c in range(4)])
    raw[344:348] = b'n+1\0'
    with gzip.open(path, 'wb', compresslevel=1) as f:
        f.write(bytes(raw) + b'\0\0\0\0' + vol.astype('<i2').tobytes(order='F'))


def make_cohort(root, n):
    x, y, z = np.meshgrid(*[np.linspace(-1, 1, s, dtype=np.float32) for s in SHAPE], indexing='ij')
    inside = (x / 0.8) ** 2 + (y / 0.85) ** 2 + (z / 0.9) ** 2 < 1
    rows = ['id\tt1\tt1ce\tt2\tflair']
    for i in range(n):
        sid = f'sub{i:02d}'
        os.makedirs(os.path.join(root, sid))
        rng = np.random.default_rng(100 + i)
        for m in ('t1', 't1ce', 't2', 'flair'):
            vol = np.where(inside, rng.integers(1, 1500, SHAPE, dtype=np.int16), 0).astype(np.int16)
            write_int16_nifti(os.path.join(root, sid, f'{m}.nii.gz'), vol)
        rows.append('\t'.join([sid] + [f'{sid}/{m}.nii.gz' for m in ('t1', 't1ce', 't2', 'flair')]))
    manifest = os.path.join(root, 'cohort.tsv')
    with open(manifest, 'w') as f:
        f.write('\n'.join(rows) + '\n')
    return manifest, float(inside.mean())


def make_checkpoints(root):
    from backbones.ncsnpp_generator_adagn_feat import NCSNpp, NCSNpp_adaptive
    cfg = bench_config()
    os.makedirs(os.path.join(root, 'results', 'bench'))
    for cls, name, seed in ((NCSNpp, 'gen_diffusive_1', 1), (NCSNpp_adaptive, 'gen_diffusive_2', 2)):
        torch.manual_seed(1234)
        net = cls(cfg)
        random_weights_(net, seed)
        torch.save(net.state_dict(), os.path.join(root, 'results', 'bench', f'{name}.pth'))


class Timed:
    """Seconds spent inside chosen functions of mudiff_hip.volume, or of `mod` (each call ends in a device synchronise)."""

    def __init__(self):
        self.t, self.saved = {}, []

    def wrap(self, name, key, mod=V):
        fn = getattr(mod, name)

        def timed(*a, **k):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn(*a, **k)
            torch.cuda.synchronize()
            self.t[key] = self.t.get(key, 0.0) + time.perf_counter() - t0
            return out
        self.saved.append((mod, name, fn))
        setattr(mod, name, timed)

    def restore(self):
        for mod, name, fn in self.saved:
            setattr(mod, name, fn)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--subjects', type=int, default=8)
    ap.add_argument('--norm', type=str, default='percentile', choices=list(V.NORMS))
    ap.add_argument('--out', type=str, default=os.path.join(REPO, 'profiles', 'cohort_bench.json'))
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_cohort.py measures on a GPU'
    with tempfile.TemporaryDirectory() as root:
        manifest, fill = make_cohort(root, a.subjects)
        make_checkpoints(root)
        model = ['--target_modality', 'T1CE', '--exp', 'bench', '--output_path', os.path.join(root, 'results'), '--num_channels_dae', '64',
                 '--image_size', '256', '--batch_size', '32', '--resize_back'] + ([] if a.norm == 'percentile' else ['--norm', a.norm])
        subjects = Co.read_manifest(manifest)

        # (A) the parent's way
        tm = Timed()
        for name, key in (('load_generators', 'load_model'), ('host_stacks', 'read_and_intake'), ('predict_slices', 'sample'),
                          ('reconstruct_volume_from_slices', 'assemble'), ('write_nifti', 'write')):
            tm.wrap(name, key)
        tm.wrap('read_nifti_raw', 'read_and_intake', VI)          # (the host path reads the files as stored, then normalises: one stage)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for s in subjects:
            V.predict_volume(V.build_argparser(model + ['--output_dir', os.path.join(root, 'A', s.id), '--input_flair', s.inputs['FLAIR'],
                                                        '--input_t2', s.inputs['T2'], '--input_t1', s.inputs['T1']]))
        torch.cuda.synchronize()
        wall_a = time.perf_counter() - t0
        tm.restore()
        stages_a = dict(tm.t, wall=wall_a)

        # (B) the cohort
        args = Co.build_argparser(model + ['--output_dir', os.path.join(root, 'B'), '--manifest', manifest])
        report, failures = Co.run(args, subjects)
        assert not failures, failures
        stages_b = report['timing']
        same = all(gzip.open(os.path.join(root, 'A', s.id, 'predicted_t1ce.nii.gz')).read() ==
                   gzip.open(os.path.join(root, 'B', s.id, 'predicted_t1ce.nii.gz')).read() for s in subjects)
    n = len(subjects)
    out = dict(what='scripts/bench_cohort.py: per-subject volume prediction, (A) predict_volume per subject with host intake and a fresh '
                    'model and sampler each time, (B) mudiff_hip.cohort with device intake; one process, one pass each',
               device=torch.cuda.get_device_name(0), norm=a.norm, subjects=n, shape=list(SHAPE), nonzero_fraction=fill, slices_per_subject=SHAPE[2],
               A=dict(subjects_per_s=n / wall_a, seconds_per_subject=wall_a / n, stages_s=stages_a, gpu_busy_share=stages_a['sample'] / wall_a,
                      note='sample includes the per-subject warm-up and hipGraph capture'),
               B=dict(subjects_per_s=n / stages_b['wall'], seconds_per_subject=stages_b['wall'] / n, stages_s=stages_b,
                      gpu_busy_share=stages_b['sample'] / stages_b['wall'],
                      note='read and write are thread seconds that overlap the GPU; write_wait is the main thread waiting for them; wall '
                           'includes the single model load and capture'),
               files_identical=bool(same), deterministic_mode=os.environ.get('MUD_DETERMINISTIC', '0') == '1')
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
