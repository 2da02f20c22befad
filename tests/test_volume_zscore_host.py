"""Not GPU: --norm zscore, the training normalisation of the volume pipeline.  The host function against
what the reference itself computed (tests/golden/zscore.npz, recorded by tests/golden/make_zscore_golden.py), the 2D route's inputs,
the moments of both intake paths, and that a default run's flags, reports and log lines are the ones it had."""
import json
import os

import numpy as np
import pytest
import torch

import volume_intake_ref as R

NAMES = ('i2_ties', 'f4_noise', 'f4_outliers', 'zeros', 'constant', 'nan')
BASE = ['--target_modality', 'T1CE', '--exp', 'e', '--output_dir', 'o']


@pytest.fixture(scope='module')
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, 'zscore.npz'))


def _host(vol):
    from mudiff_hip import volume as V
    with np.errstate(invalid='ignore'):
        return V.zscore_to_minus1_1(vol)


@pytest.mark.parametrize('name', NAMES)
def test_host_function_equals_the_reference_bit_for_bit(golden, name):
    """normalize_volume + the dataset's clamp line, as recorded from the reference, on the float64 array read_nifti returns."""
    want = golden['out_' + name]
    got = _host(golden['in_' + name].astype(np.float64))
    assert got.dtype == np.float32 and got.shape == want.shape
    assert np.array_equal(got, want, equal_nan=True)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    if name == 'zeros':
        assert not got.any()                                       # empty mask: mean 0, std 1
    if name == 'constant':
        assert set(np.unique(got).tolist()) == {-1.0, 0.0}         # std 0 -> 1: the brain at 0, the background clamped
    if name == 'nan':
        assert np.isnan(got).all()
    if name == 'f4_outliers':
        assert got.max() == 1.0 and got.min() == -1.0              # the clamp is exercised on both sides


@pytest.mark.parametrize('name', NAMES)
@pytest.mark.parametrize('half', [2, 20])
def test_condition_slices_equal_the_npy_route(golden, name, half):
    """The 2D driver's inputs: the z-scored planes s0..s1 as pre_process writes them to .npy, then BratsDataset's clamp line on each."""
    from mudiff_hip import volume as V
    z = golden['z_' + name]
    s0, s1 = R.slab_range(z.shape[2], half)
    want = [(torch.clamp(torch.from_numpy(np.ascontiguousarray(z[:, :, k])), -3.0, 3.0) / 3.0).numpy() for k in range(s0, s1 + 1)]
    slices, a, b = V.extract_center_slices(_host(golden['in_' + name].astype(np.float64)), half)
    assert (a, b) == (s0, s1) and len(slices) == len(want)
    for got, ref in zip(slices, want):
        assert np.array_equal(got, ref, equal_nan=True)


def test_load_and_preprocess_volume_takes_norm(tmp_path, golden):
    from mudiff_hip import volume as V
    path = R.write_nifti_typed(tmp_path / 'v.nii.gz', np.asfortranarray(golden['in_i2_ties']))
    slices, shp, _, _, s0, s1 = V.load_and_preprocess_volume(path, 3, norm='zscore')
    assert shp == (24, 20, 12) and (s0, s1) == (3, 9)
    assert np.array_equal(np.stack(slices, 0), np.moveaxis(golden['out_i2_ties'][:, :, 3:10], 2, 0))
    default = V.load_and_preprocess_volume(path, 3)[0]
    assert np.array_equal(np.stack(default, 0), np.stack(V.load_and_preprocess_volume(path, 3, norm='percentile')[0], 0))
    assert np.stack(default, 0).min() == -1.0 and np.stack(slices, 0).min() > -0.7      # the background: -1 against about -0.6
    with pytest.raises(ValueError, match='norm'):
        V.load_and_preprocess_volume(path, 3, norm='minmax')


@pytest.mark.parametrize('dtype,scale', [('u1', (0.0, 0.0)), ('i2', (1.0, 0.0)), ('u2', (0.5, 2.0)), ('i4', (0.0123, -5.5)), ('f4', (1.0, 0.0)),
                                         ('f4', (2.5, -1.0)), ('f8', (0.0, 0.0))])
def test_moments_of_a_raw_volume_are_the_host_paths(tmp_path, dtype, scale):
    """volume_intake.zscore_moments on the stored array == numpy's reductions on read_nifti(...).astype(float32), bit for bit, for every
    datatype, scaled or not (f8 goes through read_nifti)."""
    from mudiff_hip import volume as V
    from mudiff_hip import volume_intake as VI
    vol = R.synthetic((37, 29, 11), 'noise' if dtype[0] == 'f' else 'ties', dtype, seed=12)
    path = R.write_nifti_typed(tmp_path / 'v.nii.gz', vol, '<', *scale)
    data = V.read_nifti(path)[0].astype(np.float32)
    vals = data[data != 0]
    mean, std = VI.zscore_moments(VI.read_nifti_raw(path))
    assert isinstance(mean, np.float32) and isinstance(std, np.float32)
    assert mean.tobytes() == vals.mean().tobytes() and std.tobytes() == vals.std().tobytes()
    assert (mean, std) == V.zscore_moments_f32(data)


def test_moments_fallbacks():
    from mudiff_hip import volume_intake as VI
    raw = lambda a: VI.RawVolume(np.ascontiguousarray(a.reshape(-1, order='F')), R.CODES['i2'], '<', 1.0, 0.0, a.shape, np.eye(4), None)  # noqa: E731
    assert VI.zscore_moments(raw(np.zeros((5, 4, 3), np.int16))) == (0.0, 1.0)
    flat = np.zeros((5, 4, 3), np.int16)
    flat[1:3] = 9
    assert VI.zscore_moments(raw(flat)) == (9.0, 1.0)


def test_norm_flag_defaults_to_percentile():
    from mudiff_hip import cohort as Co
    from mudiff_hip import volume as V
    from mudiff_hip import volume_metrics as VM
    assert V.build_argparser(BASE).norm == 'percentile' and V.build_argparser(BASE + ['--norm', 'zscore']).norm == 'zscore'
    assert Co.build_argparser(BASE + ['--manifest', 'm']).norm == 'percentile'
    assert Co.build_argparser(BASE + ['--manifest', 'm', '--norm', 'zscore']).norm == 'zscore'
    m = ['--pred', 'p', '--gt', 'g']
    assert VM.build_parser().parse_args(m).norm == 'percentile' and VM.build_parser().parse_args(m + ['--norm', 'zscore']).norm == 'zscore'
    for parse in (V.build_argparser, lambda a: Co.build_argparser(a + ['--manifest', 'm'])):
        with pytest.raises(SystemExit):
            parse(BASE + ['--norm', 'minmax'])
    assert V.norm_suffix('percentile') == '' and V.norm_suffix('zscore') == ' | norm=zscore'


@pytest.mark.parametrize('norm', ['percentile', 'zscore'])
def test_done_line_names_the_mode_only_when_it_is_not_the_default(monkeypatch, capsys, tmp_path, norm):
    """predict_from_conditions with the sampler stubbed out: the [done] line is the old one by default."""
    from mudiff_hip import volume as V
    args = V.build_argparser(BASE[:-1] + [str(tmp_path), '--image_size', '8', '--slice_half_range', '2'] + (['--norm', 'zscore'] if norm == 'zscore' else []))
    monkeypatch.setattr(V, 'predict_slices', lambda *a, **k: np.zeros((5, 8, 8), np.float32))
    stacks = [np.zeros((5, 8, 8), np.float32)] * 3
    V.predict_from_conditions(args, 'auto', None, None, None, 'cpu', stacks, ((8, 8, 9), np.eye(4), None, 2, 6), write=lambda *a: None)
    line = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith('[done]')]
    want = f"[done] saved: {tmp_path}/predicted_t1ce.nii.gz | shape=(8, 8, 9) | slices=2..6"
    assert line == [want + (' | norm=zscore' if norm == 'zscore' else '')]


@pytest.mark.parametrize('norm', ['percentile', 'zscore'])
def test_cohort_computes_the_moments_on_the_prefetch_thread(tmp_path, norm):
    """The sampler stubbed out: in zscore mode every RawVolume reaches the main thread with its moments, computed by the thread that read
    it; the cohort report names the mode.  By default neither exists and the report has exactly the keys it had."""
    import threading
    from mudiff_hip import cohort as Co
    from mudiff_hip import volume as V
    rng = np.random.default_rng(1)
    rows = ['id\tt1\tt1ce\tt2\tflair']
    for sid in ('a', 'b'):
        os.makedirs(tmp_path / sid)
        for m in ('t1', 't1ce', 't2', 'flair'):
            R.write_nifti_typed(tmp_path / sid / f'{m}.nii.gz', (rng.integers(0, 50, (8, 8, 9))).astype(np.int16))
        rows.append('\t'.join([sid] + [f'{sid}/{m}.nii.gz' for m in ('t1', 't1ce', 't2', 'flair')]))
    (tmp_path / 'c.tsv').write_text('\n'.join(rows) + '\n')
    out = tmp_path / 'out'
    args = Co.build_argparser(['--target_modality', 'T1CE', '--exp', 'e', '--output_dir', str(out), '--manifest', str(tmp_path / 'c.tsv'),
                               '--image_size', '8', '--slice_half_range', '2'] + (['--norm', 'zscore'] if norm == 'zscore' else []))
    threads, seen = [], []
    real = Co._read_subject

    def read(*a):
        threads.append(threading.current_thread())
        return real(*a)

    def predict(sargs, plan, evaluation, conds, ref, write, calibrate, timing):
        seen.append([r.moments for r in conds])
        assert sargs.norm == norm

    Co._read_subject = read
    try:
        report, failures = Co.run(args, Co.read_manifest(args.manifest), predict=predict)
    finally:
        Co._read_subject = real
    assert not failures and len(seen) == 2 and all(t is not threading.main_thread() for t in threads)
    saved = json.load(open(out / 'cohort_t1ce.json'))
    old_keys = ['target', 'subjects', 'failed', 'aggregate', 'std_definition', 'timing']
    old_timing = ['read', 'intake', 'sample', 'assemble', 'write', 'write_wait', 'score', 'wall']
    if norm == 'percentile':
        assert all(m is None for ms in seen for m in ms)
        assert list(saved) == old_keys and list(saved['timing']) == old_timing
    else:
        for sid, ms in zip(('a', 'b'), seen):
            for m, got in zip(V.MODALITY_ORDERS['T1CE'], ms):
                data = V.read_nifti(str(tmp_path / sid / f'{m.lower()}.nii.gz'))[0].astype(np.float32)
                assert got == V.zscore_moments_f32(data)
        assert saved['norm'] == 'zscore' and [k for k in saved if k != 'norm'] == old_keys
        assert set(saved['timing']) == set(old_timing) | {'moments', 'read_wait'} and saved['timing']['moments'] > 0
