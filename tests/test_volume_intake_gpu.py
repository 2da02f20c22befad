"""GPU: the device intake (csrc/volume_intake.hip, mudiff_hip.volume_intake), `python -m mudiff_hip.volume --device_intake` and
`python -m mudiff_hip.cohort`.  Every comparison is exact: the census against np.sort, the slab against the host's numpy expression,
the assembled volume and the written files against the host path's bytes."""
import ctypes
import gzip
import json
import os

import numpy as np
import pytest
import torch

import volume_intake_ref as R
import volume_support as VS

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
FRACTIONS = (0.01, 0.99, 0.5, 0.999)


def _dev_raw(vol):
    from mudiff_hip import volume_intake as VI
    return VI.upload(VS.raw_volume(vol), DEV)


def _census(vol, slope, inter, fractions=FRACTIONS):
    from mudiff_hip import volume_intake as VI
    rec = VI.census(_dev_raw(vol), R.CODES[vol.dtype.str[1:]], vol.shape, slope, inter, fractions)
    return VI.CensusRecord.from_bytes(rec.cpu().numpy().tobytes(), len(fractions))


def _check_census(vol, slope=1.0, inter=0.0):
    rec = _census(vol, slope, inter)
    s = R.sorted_selected(R.values_float32(vol, slope, inter))
    assert rec.n == s.size and rec.n_nonfinite == int((~np.isfinite(s)).sum())
    if s.size:
        assert rec.min.tobytes() == s[0].tobytes() and rec.max.tobytes() == s[-1].tobytes()
    for q, (first, w) in zip(FRACTIONS, rec.windows):
        a, want = R.window(s, q)
        assert first == a and w.tobytes() == want.tobytes(), (q, first, a, w, want)
    return rec


@pytest.mark.parametrize('dtype', ['u1', 'i2', 'u2', 'i4', 'f4'])
@pytest.mark.parametrize('scale', [(1.0, 0.0), (0.0123, -5.5)], ids=['unscaled', 'scaled'])
@pytest.mark.parametrize('kind', ['ties', 'noise'])
def test_census_is_np_sort(dtype, scale, kind):
    _check_census(R.synthetic((37, 29, 11), kind, dtype, seed=2), *scale)


@pytest.mark.parametrize('kind', ['single', 'zeros'])
def test_census_of_one_voxel_and_of_none(kind):
    rec = _check_census(R.synthetic((37, 29, 11), kind, 'i2'))
    assert rec.n == (1 if kind == 'single' else 0)
    if kind == 'single':
        assert all(first == 0 and w.tolist() == [77.0] for first, w in rec.windows)


def test_census_brats_sized_and_thresholds():
    """240 x 240 x 155 int16 with thousands of ties per level; the thresholds that come out equal np.percentile on the data."""
    from mudiff_hip import volume_intake as VI
    vol = R.synthetic((240, 240, 155), 'ties', 'i2', seed=3)
    rec = _check_census(vol)
    vals = R.values_float32(vol)
    sel = vals[vals != 0]
    assert rec.n == sel.size > 1_000_000
    lo, den, degenerate = VI.thresholds(_census(vol, 1.0, 0.0, (0.01, 0.99)))
    want_lo, want_hi = np.percentile(sel, 1.0), np.percentile(sel, 99.0)
    assert not degenerate and lo.tobytes() == want_lo.tobytes() and den.tobytes() == (want_hi - want_lo).tobytes()


def test_census_counts_non_finite_voxels():
    vol = R.synthetic((20, 9, 5), 'noise', 'f4', seed=4)
    vol[3, 3, 3], vol[4, 4, 4], vol[5, 5, 1] = np.nan, np.inf, -np.inf
    rec = _census(vol, 1.0, 0.0)
    assert rec.n_nonfinite == 3 and rec.n == int((vol != 0).sum())


@pytest.mark.parametrize('dtype,scale,shape,half', [('i2', (1.0, 0.0), (37, 29, 11), 3), ('f4', (1.0, 0.0), (64, 70, 9), 20),
                                                    ('u1', (0.5, 2.0), (130, 65, 7), 2), ('i4', (0.0123, -5.5), (29, 37, 12), 4),
                                                    ('u2', (1.0, 0.0), (240, 240, 20), 6)])
def test_slab_normalise_is_the_host_function(dtype, scale, shape, half):
    """load-side equality: census -> thresholds -> slab normalise == robust_minmax_to_minus1_1 + extract_center_slices + stack."""
    from mudiff_hip import volume as V
    from mudiff_hip import volume_intake as VI
    vol = R.synthetic(shape, 'ties' if dtype != 'f4' else 'noise', dtype, seed=6)
    host64 = vol.astype(np.float64)
    if R.is_scaled(*scale):
        host64 = host64 * float(np.float32(scale[0])) + float(np.float32(scale[1]))
    slices, s0, s1 = V.extract_center_slices(V.robust_minmax_to_minus1_1(host64), half)
    want = torch.from_numpy(np.stack(slices, 0))[:, None]
    raw = VI.RawVolume(np.ascontiguousarray(vol.reshape(-1, order='F')), R.CODES[dtype], '<', scale[0], scale[1], shape, np.eye(4), None)
    got = VI.condition_from_raw(raw, half, shape[0], DEV) if shape[0] == shape[1] else None
    dev_raw = VI.upload(raw, DEV)
    slope, inter = scale if raw.scaled else (1.0, 0.0)
    rec = VI.CensusRecord.from_bytes(VI.census(dev_raw, raw.code, shape, slope, inter).cpu().numpy().tobytes(), 2)
    lo, den, degenerate = VI.thresholds(rec)
    t = VI.slab_normalise(dev_raw, raw.code, shape, slope, inter, lo, den, degenerate, s0, s1)
    assert not degenerate and t.dtype == torch.float32 and torch.equal(t.cpu(), want)
    if got is not None:
        assert torch.equal(got.cpu(), want)


def test_slab_normalise_degenerate_flag_writes_zeros():
    from mudiff_hip import volume_intake as VI
    vol = R.synthetic((37, 29, 11), 'ties', 'i2', seed=7)
    t = VI.slab_normalise(_dev_raw(vol), R.CODES['i2'], vol.shape, 1.0, 0.0, 0.0, 1.0, True, 2, 8)
    assert tuple(t.shape) == (7, 1, 37, 29) and not t.any()
    raw = VI.RawVolume(np.zeros(16 * 16 * 5, np.int16), R.CODES['i2'], '<', 1.0, 0.0, (16, 16, 5), np.eye(4), None)
    c = VI.condition_from_raw(raw, 1, 16, DEV)                    # an all-zero volume: zeros, like the host
    assert tuple(c.shape) == (3, 1, 16, 16) and not c.any()


@pytest.mark.parametrize('shape,s0,s1', [((37, 29, 11), 2, 8), ((64, 64, 5), 0, 4), ((130, 70, 9), 4, 4)])
def test_assemble_is_reconstruct_volume_from_slices(tmp_path, shape, s0, s1):
    from mudiff_hip import volume as V
    from mudiff_hip import volume_intake as VI
    rng = np.random.default_rng(8)
    n = s1 - s0 + 1
    planes, planes2 = (rng.random((n, shape[0], shape[1]), dtype=np.float32) for _ in range(2))
    want, want2 = (V.reconstruct_volume_from_slices(list(p), shape, s0, s1) for p in (planes, planes2))
    vol, vol2 = (VI.to_host_volume(v) for v in VI.assemble(torch.from_numpy(planes).to(DEV), shape, s0, s1, torch.from_numpy(planes2).to(DEV)))
    one = VI.to_host_volume(VI.assemble(torch.from_numpy(planes).to(DEV), shape, s0, s1))
    for got, ref in ((vol, want), (vol2, want2), (one, want)):
        assert got.shape == shape and got.dtype == np.float32 and got.flags['F_CONTIGUOUS'] and np.array_equal(got, ref)
    V.write_nifti(str(tmp_path / 'dev.nii.gz'), vol, np.eye(4))
    V.write_nifti(str(tmp_path / 'host.nii.gz'), want, np.eye(4))
    assert gzip.open(tmp_path / 'dev.nii.gz').read() == gzip.open(tmp_path / 'host.nii.gz').read()


def test_c_abi_rejects_bad_arguments_without_launching():
    import mudiff_hip
    lib = mudiff_hip.load()
    vol = torch.zeros(16 * 16 * 4, dtype=torch.int16, device=DEV)
    out = torch.full((4, 16, 16), 5.0, device=DEV)
    rec = torch.zeros(ctypes.sizeof(mudiff_hip.VolumeCensusRecord), dtype=torch.uint8, device=DEV)
    nws = lib.mud_volume_census_ws_bytes()
    ws = torch.zeros(nws, dtype=torch.uint8, device=DEV)
    q = (ctypes.c_double * 5)(0.1, 0.2, 0.3, 0.4, 0.5)
    census = lambda v, code, nq, r=rec, w=ws, nb=nws, qq=q: lib.mud_volume_census(v, code, 16, 16, 4, 1.0, 0.0, qq, nq, r.data_ptr(),   # noqa: E731
                                                                                   None if w is None else w.data_ptr(), nb, None)
    assert census(None, 4, 2) == 1 and b'null' in lib.mud_last_error()
    assert census(vol.data_ptr(), 64, 2) == 1 and b'datatype' in lib.mud_last_error()          # f8 is not read on the device
    assert census(vol.data_ptr(), 4, 5) == 1 and b'ranks' in lib.mud_last_error()
    assert census(vol.data_ptr(), 4, 2, nb=16) == 1 and b'workspace' in lib.mud_last_error()
    assert census(vol.data_ptr() + 2, 4, 2) == 1 and b'aligned' in lib.mud_last_error()
    bad_q = (ctypes.c_double * 2)(0.5, 1.5)
    assert census(vol.data_ptr(), 4, 2, qq=bad_q) == 1
    slab = lambda v, code, s0, s1, o=out: lib.mud_volume_slab_normalise(v, code, 16, 16, 4, 1.0, 0.0, 0.0, 1.0, 0, s0, s1,          # noqa: E731
                                                                        None if o is None else o.data_ptr(), None)
    assert slab(vol.data_ptr(), 4, 1, 4) == 1 and b'slab' in lib.mud_last_error()
    assert slab(vol.data_ptr(), 4, 2, 1) == 1 and slab(vol.data_ptr(), 4, -1, 2) == 1
    assert slab(vol.data_ptr(), 3, 0, 3) == 1 and slab(None, 4, 0, 3) == 1 and slab(vol.data_ptr(), 4, 0, 3, None) == 1
    planes = torch.ones(2, 16, 16, device=DEV)
    asm = lambda p, p2, s0, s1, v, v2: lib.mud_volume_assemble(p, p2, 16, 16, 4, s0, s1, v, v2, None)                               # noqa: E731
    assert asm(None, None, 1, 2, out.data_ptr(), None) == 1 and b'null' in lib.mud_last_error()
    assert asm(planes.data_ptr(), None, 3, 4, out.data_ptr(), None) == 1 and b'slab' in lib.mud_last_error()
    assert asm(planes.data_ptr(), planes.data_ptr(), 1, 2, out.data_ptr(), None) == 1
    torch.cuda.synchronize()
    assert float(out.min()) == 5.0 and float(out.max()) == 5.0 and not rec.any()                # nothing was launched
    assert asm(planes.data_ptr(), None, 1, 2, out.data_ptr(), None) == 0                        # the library still works afterwards
    torch.cuda.synchronize()
    assert out[0].sum() == 0 and out[1].sum() == 256 and out[3].sum() == 0


# ---------------------------------------------------------------------------------------------------
# end to end: the volume CLI with and without --device_intake, then the cohort
# ---------------------------------------------------------------------------------------------------
def _subject(root, sid, shape, seed, dtype='i2', scale=(0.0, 0.0)):
    rng = np.random.default_rng(seed)
    os.makedirs(root / sid)
    aff = np.diag([1.0, 1.0, 2.5, 1.0])
    paths = {}
    for m in ('t1', 't1ce', 't2', 'flair'):
        v = (rng.integers(100, 150, shape) * (rng.random(shape) > 0.2)).astype(dtype)
        paths[m] = R.write_nifti_typed(root / sid / f'{sid}_{m}.nii.gz', np.asfortranarray(v), '<', *scale, affine=aff)
    seg = ((rng.random(shape) < 0.3) * 4).astype('u1')
    paths['seg'] = R.write_nifti_typed(root / sid / f'{sid}_seg.nii.gz', np.asfortranarray(seg), affine=aff)
    return paths


def test_device_intake_and_cohort_write_the_host_path_files(tmp_path):
    VS.write_tiny_model(tmp_path)
    model = VS.model_argv(tmp_path, 3, 4, '--resize_back')
    data = tmp_path / 'brats'
    subjects = {'s_a': _subject(data, 's_a', (16, 16, 9), 1), 's_b': _subject(data, 's_b', (20, 12, 11), 2, scale=(0.5, 3.0)),
                's_c': _subject(data, 's_c', (16, 16, 9), 3)}
    os.remove(subjects['s_c']['t2'])                                   # deliberately missing
    (tmp_path / 'test.list').write_text('s_a\ns_c\ns_b\n')
    single = {}
    for sid in ('s_a', 's_b'):
        p = subjects[sid]
        inputs = ['--input_flair', p['flair'], '--input_t2', p['t2'], '--input_t1', p['t1'], '--gt_volume', p['t1ce'], '--eval_mask', p['seg']]
        host, dev = str(tmp_path / f'{sid}_host'), str(tmp_path / f'{sid}_dev')
        a = VS.run_module('mudiff_hip.volume', model + inputs + ['--output_dir', host])
        b = VS.run_module('mudiff_hip.volume', model + inputs + ['--output_dir', dev, '--device_intake'])
        assert VS.payload(host + '/predicted_t1ce.nii.gz') == VS.payload(dev + '/predicted_t1ce.nii.gz')
        assert json.load(open(host + '/metrics_t1ce.json')) == json.load(open(dev + '/metrics_t1ce.json'))
        assert a.stdout.replace(host, 'OUT') == b.stdout.replace(dev, 'OUT')      # the same lines, too
        single[sid] = host
    # an ensemble through both paths (mean and std volumes)
    p = subjects['s_b']
    inputs = ['--input_flair', p['flair'], '--input_t2', p['t2'], '--input_t1', p['t1'], '--num_samples', '2']
    VS.run_module('mudiff_hip.volume', model + inputs + ['--output_dir', str(tmp_path / 'ens_host')])
    VS.run_module('mudiff_hip.volume', model + inputs + ['--output_dir', str(tmp_path / 'ens_dev'), '--device_intake'])
    for name in ('predicted_t1ce.nii.gz', 'predicted_t1ce_std.nii.gz'):
        assert VS.payload(str(tmp_path / 'ens_host' / name)) == VS.payload(str(tmp_path / 'ens_dev' / name))
    # the cohort: three subjects, one of them broken
    out = tmp_path / 'cohort'
    c = VS.run_module('mudiff_hip.cohort', model + ['--brats_root', str(data), '--subjects', str(tmp_path / 'test.list'), '--score', '--output_dir',
                                           str(out), '--io_threads', '2'], expect=1)
    assert '[cohort] skipped s_c' in c.stderr and 'FAILED s_c' in c.stderr and '[cohort] brain: PSNR ' in c.stdout
    for sid in ('s_a', 's_b'):
        assert VS.payload(str(out / sid / 'predicted_t1ce.nii.gz')) == VS.payload(single[sid] + '/predicted_t1ce.nii.gz')
        assert json.load(open(out / sid / 'metrics_t1ce.json')) == json.load(open(single[sid] + '/metrics_t1ce.json'))
    assert not (out / 's_c' / 'predicted_t1ce.nii.gz').exists()
    from mudiff_hip import cohort as Co
    rep = json.load(open(out / 'cohort_t1ce.json'))
    rows = [Co.subject_row(sid, json.load(open(out / sid / 'metrics_t1ce.json'))) for sid in ('s_a', 's_b')]
    assert rep['subjects'] == rows and rep['aggregate'] == Co.aggregate(rows) and [f['id'] for f in rep['failed']] == ['s_c']
    for name in ('slab', 'brain', 'tumor', 'healthy'):
        vals = [r['metrics'][name]['mae'] for r in rows]
        assert rep['aggregate'][name]['mae']['count'] == 2
        assert abs(rep['aggregate'][name]['mae']['mean'] - np.mean(vals)) <= 1e-15 and abs(rep['aggregate'][name]['mae']['std'] - np.std(vals)) <= 1e-15
    assert rep['timing']['wall'] > 0 and rep['timing']['sample'] > 0
