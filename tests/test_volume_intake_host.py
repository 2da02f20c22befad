"""CPU: the host half of the device intake (mudiff_hip.volume_intake) and of the cohort entry point (mudiff_hip.cohort): thresholds from
census windows against np.percentile on the data, the fallback chain against robust_minmax_to_minus1_1, the raw NIfTI reader against
read_nifti, manifest / BraTS parsing, the cohort's aggregation arithmetic and its skip-and-continue path with the sampler stubbed."""
import ctypes
import json
import math
import os
import subprocess

import numpy as np
import pytest

from conftest import REPO
import volume_intake_ref as R


def _record(values, pmin=1.0, pmax=99.0):
    from mudiff_hip import volume_intake as VI
    return VI.CensusRecord.from_sorted(R.sorted_selected(values), (pmin / 100.0, pmax / 100.0))


def _cases():
    rng = np.random.default_rng(0)
    yield 'n1', np.array([3.5], np.float32)
    yield 'n2', np.array([-2.0, 7.25], np.float32)
    yield 'n17', rng.standard_normal(17).astype(np.float32)
    yield 'n5000_ties', rng.integers(1, 40, 5000).astype(np.float32)
    yield 'n5000_negatives', (rng.standard_normal(5000) * 300).astype(np.float32)
    yield 'n2.4M_ties', rng.integers(1, 1500, 2_400_000).astype(np.float32)
    yield 'n2.4M_distinct', rng.random(2_400_000, dtype=np.float32) + np.float32(0.5)
    yield 'scaled_i2', R.values_float32(rng.integers(-2000, 2000, 300_000).astype(np.int16), 0.0123, -5.5)


@pytest.mark.parametrize('name,vals', list(_cases()), ids=[c[0] for c in _cases()])
@pytest.mark.parametrize('pmin,pmax', [(1.0, 99.0), (0.5, 99.9), (50.0, 99.0)])
def test_thresholds_equal_numpy_percentile_on_the_data(name, vals, pmin, pmax):
    from mudiff_hip import volume_intake as VI
    sel = vals[vals != 0]
    lo, hi = np.percentile(sel, pmin), np.percentile(sel, pmax)
    got_lo, got_den, degenerate = VI.thresholds(_record(vals, pmin, pmax), pmin, pmax)
    if hi <= lo:                                        # the host's min / max fallback
        lo, hi = float(sel.min()), float(sel.max())
        if hi <= lo:
            assert degenerate
            return
        want_lo, want_den = np.float32(lo), np.float32(hi - lo)
    else:
        want_lo, want_den = lo, hi - lo
    assert not degenerate
    assert np.float32(got_lo).tobytes() == np.float32(want_lo).tobytes(), (got_lo, want_lo)
    assert np.float32(got_den).tobytes() == np.float32(want_den).tobytes(), (got_den, want_den)


@pytest.mark.parametrize('kind', ['flat', 'empty', 'zeros', 'two_levels', 'ties', 'noise'])
def test_fallback_chain_matches_the_host_function(kind):
    """thresholds + the numpy normalisation expression == robust_minmax_to_minus1_1, bit for bit, on the volumes that walk its
    fallback chain (flat: every selected voxel equal; two_levels: percentiles equal, min / max not)."""
    from mudiff_hip import volume as V
    from mudiff_hip import volume_intake as VI
    rng = np.random.default_rng(3)
    shape = (12, 10, 7)
    if kind == 'flat':
        vol = np.where(rng.random(shape) > 0.4, 9.0, 0.0)
    elif kind == 'empty':
        vol = np.zeros((0, 4, 4))
    elif kind == 'zeros':
        vol = np.zeros(shape)
    elif kind == 'two_levels':
        vol = np.full(shape, 5.0)
        vol[0, 0, 0], vol[1, 1, 1] = 1.0, 11.0
    elif kind == 'ties':
        vol = rng.integers(0, 6, shape).astype(np.float64)
    else:
        vol = rng.standard_normal(shape) * (rng.random(shape) > 0.2)
    want = V.robust_minmax_to_minus1_1(vol)
    vals = vol.astype(np.float32)
    lo, den, degenerate = VI.thresholds(_record(vals))
    got = np.zeros(shape if kind != 'empty' else vol.shape, np.float32) if degenerate else R.normalise(vals, lo, den)
    assert got.dtype == want.dtype == np.float32 and got.tobytes() == want.tobytes()
    if kind in ('flat', 'empty', 'zeros'):
        assert degenerate and not got.any()
    if kind == 'two_levels':
        assert (float(lo), float(den)) == (1.0, 10.0)


def test_thresholds_refuse_non_finite_volumes():
    from mudiff_hip import volume_intake as VI
    with pytest.raises(ValueError, match='non-finite'):
        VI.thresholds(_record(np.array([1.0, np.inf, 2.0], np.float32)))


@pytest.mark.parametrize('dtype', ['u1', 'i2', 'u2', 'i4', 'f4', 'f8', 'i1'])
@pytest.mark.parametrize('endian', ['<', '>'])
@pytest.mark.parametrize('scale', [(0.0, 0.0), (1.0, 0.0), (0.37, -3.0), (1.0, 2.0)])
def test_read_nifti_raw_is_read_nifti_without_the_conversion(tmp_path, dtype, endian, scale):
    from mudiff_hip import volume as V
    from mudiff_hip import volume_intake as VI
    vol = R.synthetic((9, 7, 5), 'noise', dtype, seed=5)
    aff = np.diag([1.0, 2.0, 3.0, 1.0])
    path = R.write_nifti_typed(tmp_path / 'v.nii.gz', vol, endian, *scale, affine=aff)
    want, want_aff, _ = V.read_nifti(path)
    raw = VI.read_nifti_raw(path)
    direct = endian == '<' and dtype in R.CODES
    assert raw.shape == (9, 7, 5) and np.array_equal(raw.affine, want_aff)
    if direct:
        assert raw.code == R.CODES[dtype] and raw.data.dtype == np.dtype('<' + dtype) and raw.data.tobytes() == vol.tobytes(order='F')
        assert np.float32(raw.slope) == np.float32(scale[0]) and np.float32(raw.inter) == np.float32(scale[1])
        assert raw.scaled == R.is_scaled(*scale)
    else:                                            # through read_nifti, as float32
        assert raw.code == R.CODES['f4'] and raw.data.dtype == np.float32 and not raw.scaled
    assert raw.values_float64().astype(np.float32).tobytes() == want.astype(np.float32).tobytes()
    if direct:
        assert raw.values_float64().tobytes() == want.tobytes()
        slope, inter = (raw.slope, raw.inter) if raw.scaled else (1.0, 0.0)
        assert R.values_float32(raw.data, slope, inter).reshape(raw.shape, order='F').tobytes() == want.astype(np.float32).tobytes()


def test_record_struct_matches_the_header(tmp_path):
    import mudiff_hip
    cls = mudiff_hip.VolumeCensusRecord
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{os.path.join(REPO, "include", "mudiff_hip.h")}"', 'int main(void) {',
             '  printf("size %zu\\n", sizeof(mud_volume_census_record));']
    lines += [f'  printf("{f} %zu\\n", offsetof(mud_volume_census_record, {f}));' for f, _ in cls._fields_]
    lines += ['  return 0;', '}']
    (tmp_path / 'l.c').write_text('\n'.join(lines))
    subprocess.run(['gcc', '-std=c11', '-o', str(tmp_path / 'l'), str(tmp_path / 'l.c')], check=True)
    out = dict(ln.split() for ln in subprocess.run([str(tmp_path / 'l')], check=True, stdout=subprocess.PIPE, text=True).stdout.splitlines())
    assert int(out.pop('size')) == ctypes.sizeof(cls)
    assert {k: int(v) for k, v in out.items()} == {f: getattr(cls, f).offset for f, _ in cls._fields_}


def test_device_intake_flag_defaults_off():
    from mudiff_hip import volume as V
    base = ['--target_modality', 'T1CE', '--exp', 'e', '--output_dir', 'o']
    assert V.build_argparser(base).device_intake is False and V.build_argparser(base + ['--device_intake']).device_intake is True


# ---------------------------------------------------------------------------------------------------
# the cohort
# ---------------------------------------------------------------------------------------------------
def test_manifest_parsing(tmp_path):
    from mudiff_hip import cohort as Co
    m = tmp_path / 'c.tsv'
    m.write_text('id\tt1\tt1ce\tt2\tflair\tgt\tmask\n'
                 'a\ta/t1.nii.gz\ta/t1ce.nii.gz\ta/t2.nii.gz\ta/flair.nii.gz\ta/t1ce.nii.gz\ta/seg.nii.gz\n'
                 'b\t/abs/t1.nii\t\t/abs/t2.nii\t/abs/flair.nii\t\t\n')
    a, b = Co.read_manifest(str(m))
    assert a.id == 'a' and a.inputs['T1CE'] == str(tmp_path / 'a/t1ce.nii.gz') and a.gt == str(tmp_path / 'a/t1ce.nii.gz')
    assert a.mask == str(tmp_path / 'a/seg.nii.gz')
    assert b.inputs == {'T1': '/abs/t1.nii', 'T1CE': None, 'T2': '/abs/t2.nii', 'FLAIR': '/abs/flair.nii'} and b.gt is None and b.mask is None
    m.write_text('id\tt1\tt2\n')
    with pytest.raises(ValueError, match='no subjects'):
        Co.read_manifest(str(m))
    m.write_text('id\tt1\tt2\nx\t1\t2\n')
    with pytest.raises(ValueError, match='t1ce, flair'):
        Co.read_manifest(str(m))
    m.write_text('id\tt1\tt1ce\tt2\tflair\nx\t1\t2\t3\t4\nx\t1\t2\t3\t4\n')
    with pytest.raises(ValueError, match='unique'):
        Co.read_manifest(str(m))


def test_brats_layout(tmp_path):
    from mudiff_hip import cohort as Co
    lst = tmp_path / 'test.list'
    lst.write_text('BraTS_001\n\n# a comment\nBraTS_007\n')
    s = Co.brats_subjects('/data/brats', str(lst), 'T2')
    assert [x.id for x in s] == ['BraTS_001', 'BraTS_007']
    assert s[1].inputs['FLAIR'] == '/data/brats/BraTS_007/BraTS_007_flair.nii.gz'
    assert s[1].gt == '/data/brats/BraTS_007/BraTS_007_t2.nii.gz' and s[1].mask == '/data/brats/BraTS_007/BraTS_007_seg.nii.gz'


def test_cohort_parser_shares_the_volume_flags_and_checks_its_own():
    from mudiff_hip import cohort as Co
    base = ['--target_modality', 'T1', '--exp', 'e', '--output_dir', 'o']
    a = Co.build_argparser(base + ['--manifest', 'm.tsv', '--batch_size', '8', '--num_samples', '3', '--prec_plan', 'fp16', '--resize_back'])
    assert (a.batch_size, a.num_samples, a.prec_plan, a.resize_back, a.io_threads, a.score) == (8, 3, 'fp16', True, 4, False)
    for bad in ([], ['--manifest', 'm', '--brats_root', 'r', '--subjects', 's'], ['--brats_root', 'r'], ['--manifest', 'm', '--io_threads', '0'],
                ['--manifest', 'm', '--input_t1', 'x.nii']):
        with pytest.raises(SystemExit):
            Co.build_argparser(base + bad)


def test_aggregation_arithmetic():
    from mudiff_hip import cohort as Co
    row = lambda sid, **regions: dict(id=sid, metrics={k: dict(psnr=v[0], ssim3d=v[1], mae=v[2], voxels=10) for k, v in regions.items()})  # noqa: E731
    rows = [row('a', slab=(20.0, 0.5, 0.25), tumor=(10.0, None, 0.5)), row('b', slab=(30.0, 0.75, 0.125), tumor=(math.inf, None, 0.25)),
            row('c', slab=(40.0, 1.0, 0.0)), row('d', slab=(50.0, 0.75, 0.125))]
    agg = Co.aggregate(rows)
    assert agg['slab']['psnr'] == dict(mean=35.0, std=math.sqrt(125.0), count=4)
    assert agg['slab']['ssim3d'] == dict(mean=0.75, std=math.sqrt(0.03125), count=4)
    assert agg['slab']['mae'] == dict(mean=0.125, std=math.sqrt(0.0078125), count=4)
    assert agg['tumor']['psnr'] == dict(mean=10.0, std=0.0, count=1)                # inf is not averaged
    assert agg['tumor']['ssim3d'] == dict(mean=None, std=None, count=0)
    assert agg['tumor']['mae'] == dict(mean=0.375, std=0.125, count=2)
    lines = Co.format_lines(agg)
    assert lines[0] == '[cohort] slab: PSNR 35.0000 +- 11.1803 dB | SSIM3D 0.750000 +- 0.176777 | MAE 0.125000 +- 0.088388 | subjects 4'
    assert 'SSIM3D n/a' in lines[1]


def test_a_bad_subject_is_skipped_and_the_run_continues(tmp_path, capsys):
    """Three subjects, the sampler stubbed out: one has a missing file, one has volumes of different shapes; the third is predicted,
    the failures are reported and the table holds the good subject only."""
    from mudiff_hip import cohort as Co
    from mudiff_hip import volume as V
    rng = np.random.default_rng(1)
    rows = ['id\tt1\tt1ce\tt2\tflair']
    for sid, shapes in (('good', [(8, 8, 9)] * 4), ('missing', [(8, 8, 9)] * 4), ('mismatch', [(8, 8, 9), (8, 8, 9), (8, 6, 9), (8, 8, 9)])):
        os.makedirs(tmp_path / sid)
        for m, shp in zip(('t1', 't1ce', 't2', 'flair'), shapes):
            R.write_nifti_typed(tmp_path / sid / f'{m}.nii.gz', (rng.integers(0, 50, shp)).astype(np.int16))
        rows.append('\t'.join([sid] + [f'{sid}/{m}.nii.gz' for m in ('t1', 't1ce', 't2', 'flair')]))
    os.remove(tmp_path / 'missing' / 't2.nii.gz')
    (tmp_path / 'c.tsv').write_text('\n'.join(rows) + '\n')
    out = tmp_path / 'out'
    args = Co.build_argparser(['--target_modality', 'T1CE', '--exp', 'e', '--output_dir', str(out), '--manifest', str(tmp_path / 'c.tsv'),
                               '--image_size', '8', '--slice_half_range', '2'])
    seen = []

    def predict(sargs, plan, evaluation, conds, ref, write, calibrate, timing):
        shp, aff, hdr, s0, s1 = ref
        seen.append((os.path.basename(sargs.output_dir), shp, s0, s1, calibrate))
        os.makedirs(sargs.output_dir, exist_ok=True)
        write(os.path.join(sargs.output_dir, 'predicted_t1ce.nii.gz'), np.zeros(shp, np.float32), aff, hdr)

    report, failures = Co.run(args, Co.read_manifest(args.manifest), predict=predict)
    assert seen == [('good', (8, 8, 9), 2, 6, True)]
    assert [f[0] for f in failures] == ['missing', 'mismatch'] and 'share shape' in failures[1][1]
    assert V.read_nifti(str(out / 'good' / 'predicted_t1ce.nii.gz'))[0].shape == (8, 8, 9)
    saved = json.load(open(out / 'cohort_t1ce.json'))
    assert [r['id'] for r in saved['subjects']] == ['good'] and [f['id'] for f in saved['failed']] == ['missing', 'mismatch']
    assert 'ddof = 0' in saved['std_definition'] and set(saved['timing']) >= {'read', 'intake', 'sample', 'assemble', 'write', 'wall'}
    err = capsys.readouterr().err
    assert '[cohort] skipped missing' in err and '[cohort] skipped mismatch' in err
