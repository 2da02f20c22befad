"""GPU: --regrid_interp cubic.  mud_volume_bspline_coeffs and mud_volume_regrid_cubic against the fp64 numpy
restatement (tests/volume_bspline_ref.py), bit for bit: every stored datatype that matters to the recursion, axes of 1 and 2 voxels,
axes longer than a tile of the x pass and than a workgroup of the y and z passes, non-finite voxels, the background guard and the
clamp; the C ABI's argument checks; volume_regrid.regrid_to(mode='cubic'); then `predict_volume --regrid --regrid_interp cubic` against
the same run on inputs resampled beforehand, byte for byte, --coregister with the flag, and the flag's default."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import volume_bspline_ref as S
import volume_intake_ref as R
import volume_regrid_ref as G
import volume_support as VS

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SRC_SHAPE, OUT_SHAPE = (13, 9, 7), (11, 12, 6)


def _bits(a):
    return np.ascontiguousarray(a).view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _stored(vol, scale=(1.0, 0.0)):
    """-> (the device array of the stored voxels, datatype code, slope, inter, the fp32 values the pipeline sees)."""
    from mudiff_hip import volume_intake as VI
    raw = VS.raw_volume(vol, scale)
    slope, inter = (raw.slope, raw.inter) if raw.scaled else (1.0, 0.0)
    return VI.upload(raw, DEV), raw.code, slope, inter, np.asfortranarray(R.values_float32(vol, *scale))


def _device_coeffs(vol, scale=(1.0, 0.0)):
    """-> (device fp64 [Z,Y,X], the non-finite count, the values)."""
    import mudiff_hip
    dev, code, slope, inter, values = _stored(vol, scale)
    coeffs = torch.full(vol.shape[::-1], -7.0, device=DEV, dtype=torch.float64)
    bad = torch.full((1,), 99, device=DEV, dtype=torch.int32)
    mudiff_hip.check(mudiff_hip.load().mud_volume_bspline_coeffs(dev.data_ptr(), code, *vol.shape, slope, inter, coeffs.data_ptr(), bad.data_ptr(),
                                                                  None), 'volume_bspline_coeffs')
    torch.cuda.synchronize()
    return coeffs, int(bad.cpu()[0]), values


# x: 300 crosses nine chunks of the x pass, 13 and 5 end inside one; y x z = 63, 2 and 6 lines end inside a tile of 64 lines.
# y: 257 positions per thread; z: 130.  1 and 2: the lines that have no recursion / no interior.
COEFF_CASES = [('i2', (13, 9, 7), (0.5, -3.0)), ('f4', (5, 1, 2), (1.0, 0.0)), ('u1', (2, 2, 2), (1.0, 0.0)), ('f4', (300, 3, 2), (1.0, 0.0)),
               ('u2', (3, 257, 2), (1.0, 0.0)), ('f4', (2, 3, 130), (1.0, 0.0)), ('f4', (70, 23, 17), (1.0, 0.0))]


@pytest.mark.parametrize('dtype,shape,scale', COEFF_CASES)
def test_coefficients_are_the_reference_bit_for_bit(dtype, shape, scale):
    vol = R.synthetic(shape, 'noise', dtype, seed=61)
    bad = 0
    if shape == (300, 3, 2):                                                       # a NaN and an inf are read as 0 and counted
        vol[17, 1, 0], vol[299, 2, 1], bad = np.nan, -np.inf, 2
    got, counted, values = _device_coeffs(vol, scale)
    want, want_bad = S.coefficients(values)
    got = got.cpu().numpy().transpose(2, 1, 0)
    err = np.abs(got - want).max() / max(float(np.abs(want).max()), 1e-30)
    print('max relative difference', err, '| bit-equal', float((_bits(got) == _bits(want)).mean()))
    assert counted == want_bad == bad
    assert np.isfinite(got).all() and np.abs(want).max() > 0
    assert np.array_equal(_bits(got), _bits(want))


def _matrix(name):
    """Reference voxel index of OUT_SHAPE -> coordinate in SRC_SHAPE."""
    M = np.eye(4)
    if name == 'oblique':                                                          # a rotation with anisotropic scaling about the centres
        lin = G.oblique_linear()
        M[:3, :3] = lin
        M[:3, 3] = (np.array(SRC_SHAPE) - 1) / 2.0 - lin @ ((np.array(OUT_SHAPE) - 1) / 2.0)
    elif name == 'half':                                                           # a pure half-voxel shift
        M[:3, 3] = 0.5
    elif name == 'partly_outside':                                                 # a third of the output lies outside the source
        M[:3, :3] = np.diag([1.3, 0.9, 1.1]) @ np.array([[1.0, 0.1, 0], [-0.1, 1.0, 0.05], [0, -0.05, 1.0]])
        M[:3, 3] = (-2.3, -1.7, 0.4)
    else:
        assert name == 'identity'
    return M


def _sources():
    f4 = R.synthetic(SRC_SHAPE, 'noise', 'f4', seed=62)
    f4[:5], f4[:, :4, :4] = 0, 0                                                   # air: a slab and a bar of exact zeros
    i2 = R.synthetic(SRC_SHAPE, 'noise', 'i2', seed=63) // 100
    i2[8:], i2[:, 6:, :] = 6, 6                                                    # stored 6 -> 6 * 0.5 - 3 = 0: air by the voxel's value
    return {'f4': (np.asfortranarray(f4), (1.0, 0.0)), 'i2': (np.asfortranarray(i2.astype('i2')), (0.5, -3.0))}


@pytest.fixture(scope='module')
def prepared():
    """Per source: the device arrays, the device coefficients and the reference's, made once."""
    out = {}
    for key, (vol, scale) in _sources().items():
        coeffs, _, values = _device_coeffs(vol, scale)
        want = S.coefficients(values)[0]
        assert np.array_equal(_bits(coeffs.cpu().numpy().transpose(2, 1, 0)), _bits(want))
        out[key] = dict(stored=_stored(vol, scale), coeffs=coeffs, ref=want, values=values)
    return out


def _device_cubic(p, M, lo, hi, out_shape=OUT_SHAPE):
    import mudiff_hip
    dev, code, slope, inter, values = p['stored']
    out = torch.full(out_shape[::-1], 5.0, device=DEV)
    m = (C.c_double * 12)(*np.asarray(M, np.float64)[:3, :4].reshape(-1).tolist())
    mudiff_hip.check(mudiff_hip.load().mud_volume_regrid_cubic(p['coeffs'].data_ptr(), *values.shape, dev.data_ptr(), code, slope, inter, m, lo, hi,
                                                                *out_shape, out.data_ptr(), None), 'volume_regrid_cubic')
    torch.cuda.synchronize()
    return out.cpu().numpy().transpose(2, 1, 0)


@pytest.mark.parametrize('source', ['f4', 'i2'])
@pytest.mark.parametrize('name', ['oblique', 'half', 'identity', 'partly_outside'])
def test_interpolation_is_the_reference_bit_for_bit(prepared, name, source):
    p, M = prepared[source], _matrix(name)
    lo, hi = S.value_range(p['values'])
    assert lo < 0 < hi
    got = _device_cubic(p, M, lo, hi)
    want = S.interpolate(p['ref'], p['values'], M, OUT_SHAPE, lo, hi)
    free = S.interpolate(p['ref'], p['values'], M, OUT_SHAPE, lo, hi, guard=False, clamp=False)
    inside = S.in_range(M, SRC_SHAPE, OUT_SHAPE)[0]
    guarded, clamped = int(((free != 0) & (want == 0)).sum()), int(((free < lo) | (free > hi)).sum())
    print(f'{int(inside.sum())} of {inside.size} in range | guard {guarded} voxels | clamp {clamped} voxels | bit-equal',
          float((_bits(got) == _bits(want)).mean()), '| max diff', float(np.abs(got.astype(np.float64) - want).max()))
    assert got.dtype == np.float32 and np.array_equal(_bits(got), _bits(want))
    assert got.min() >= lo and got.max() <= hi and np.count_nonzero(got) >= 0.1 * got.size
    assert not got[~inside].any() and not np.signbit(got[got == 0]).any()          # +0 outside the source and in the air
    if name == 'identity':
        assert np.array_equal(got[:, :9, :], p['values'][:11, :, :6]) and not got[:, 9:, :].any()      # it interpolates
    elif name == 'partly_outside':
        assert 0.2 * inside.size <= inside.sum() <= 0.8 * inside.size
    else:
        assert guarded > 0                                                         # (the guard is what made those voxels 0)
    # the clamp: rarely met with the source's own range (`clamped`), so once more with a range the values leave on both sides
    tight = _device_cubic(p, M, lo / 4, hi / 4)
    assert np.array_equal(_bits(tight), _bits(S.interpolate(p['ref'], p['values'], M, OUT_SHAPE, lo / 4, hi / 4)))
    assert tight.min() == np.float32(lo / 4) and tight.max() == np.float32(hi / 4)


def test_c_abi_rejects_bad_arguments_without_launching():
    import mudiff_hip
    lib = mudiff_hip.load()
    src = torch.zeros(16 * 8 * 4, dtype=torch.int16, device=DEV)
    coeffs = torch.full((4, 8, 16), 5.0, device=DEV, dtype=torch.float64)
    bad = torch.full((1,), 7, device=DEV, dtype=torch.int32)
    out = torch.full((4, 8, 16), 5.0, device=DEV)
    eye = [1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0, 0]
    ptr = lambda t: None if t is None else t.data_ptr()      # noqa: E731

    def prefilter(s=src, code=4, dims=(16, 8, 4), c=coeffs, b=bad):
        return lib.mud_volume_bspline_coeffs(ptr(s), code, *dims, 1.0, 0.0, ptr(c), ptr(b), None)

    def cubic(c=coeffs, dims=(16, 8, 4), s=src, code=4, m=eye, lo=-1.0, hi=1.0, size=(16, 8, 4), o=out):
        mm = None if m is None else (C.c_double * 12)(*m)
        return lib.mud_volume_regrid_cubic(ptr(c), *dims, ptr(s), code, 1.0, 0.0, mm, lo, hi, *size, ptr(o), None)

    for call, words in ((lambda: prefilter(s=None), (b'null', b'vol')), (lambda: prefilter(c=None), (b'null', b'coeffs')),
                        (lambda: prefilter(b=None), (b'null', b'nonfinite')), (lambda: prefilter(code=64), (b'datatype',)),
                        (lambda: prefilter(dims=(16, 0, 4)), (b'size',)),
                        (lambda: cubic(c=None), (b'null', b'coeffs')), (lambda: cubic(s=None), (b'null', b'src')),
                        (lambda: cubic(m=None), (b'null', b'(m)')), (lambda: cubic(o=None), (b'null', b'out')),
                        (lambda: cubic(m=eye[:5] + [float('nan')] + eye[6:]), (b'm[5]', b'finite')),
                        (lambda: cubic(m=eye[:3] + [float('inf')] + eye[4:]), (b'm[3]', b'finite')),
                        (lambda: cubic(lo=2.0, hi=1.0), (b'lo', b'hi')), (lambda: cubic(lo=0.5, hi=1.0), (b'lo', b'hi')),
                        (lambda: cubic(lo=-1.0, hi=-0.5), (b'lo', b'hi')), (lambda: cubic(lo=float('-inf')), (b'lo', b'finite')),
                        (lambda: cubic(hi=float('nan')), (b'hi', b'finite')), (lambda: cubic(code=64), (b'datatype',)),
                        (lambda: cubic(size=(0, 8, 4)), (b'output size',)), (lambda: cubic(dims=(16, 8, -1)), (b'size',))):
        assert call() == 1
        msg = lib.mud_last_error()
        assert all(w in msg for w in words), msg
    torch.cuda.synchronize()
    assert float(out.min()) == 5.0 == float(out.max()) and float(coeffs.min()) == 5.0 == float(coeffs.max()) and int(bad.cpu()[0]) == 7
    assert prefilter() == 0 and cubic() == 0                                       # the library still works afterwards
    torch.cuda.synchronize()
    assert not out.any() and not coeffs.any() and int(bad.cpu()[0]) == 0


def test_regrid_to_cubic(prepared):
    from mudiff_hip import volume_regrid as VR
    vol, scale = _sources()['i2']
    raw = VS.raw_volume(vol, scale)
    assert VR.regrid_to(raw, vol.shape, np.eye(4), DEV, 'cubic') is raw             # on the grid already: untouched
    aff = _matrix('oblique')                                                       # the reference's affine, the source's being the identity
    found = {}
    r = VR.regrid_to(raw, OUT_SHAPE, aff, DEV, 'cubic', found=found)
    assert isinstance(r, VR.RegriddedVolume) and r.code == 16 and r.shape == OUT_SHAPE and r.scaling == (1.0, 0.0) and found == {'nonfinite': 0}
    assert r.dev.dtype == torch.float32 and tuple(r.dev.shape) == OUT_SHAPE[::-1]
    want = S.regrid(prepared['i2']['values'], VR.grid_matrix(np.eye(4), aff), OUT_SHAPE)
    assert np.array_equal(_bits(r.values_float32()), _bits(want)) and want.any()
    linear = VR.regrid_to(raw, OUT_SHAPE, aff, DEV).values_float32()
    assert not np.array_equal(linear, want) and (linear == 0).any() and not want[linear == 0].any()      # another interpolant, no new tissue
    nan = np.asfortranarray(vol.astype('f4'))
    nan[3, 3, 3] = np.nan
    VR.regrid_to(VS.raw_volume(nan), OUT_SHAPE, aff, DEV, 'cubic', found=found)
    assert found == {'nonfinite': 1}
    with pytest.raises(ValueError, match='mode must be one of'):
        VR.regrid_to(raw, OUT_SHAPE, aff, DEV, 'sinc')


# ---------------------------------------------------------------------------------------------------
# end to end: the tiny model of tests/test_volume_regrid_gpu.py, inputs on three grids
# ---------------------------------------------------------------------------------------------------
def _affine(lin, centre_of):
    a = np.eye(4)
    a[:3, :3] = lin
    a[:3, 3] = -np.asarray(lin) @ ((np.array(centre_of) - 1) / 2.0)
    return a


@pytest.fixture(scope='module')
def runs(tmp_path_factory):
    """One child process for every sampling run of this module: the log of each run."""
    from mudiff_hip import volume as V
    tmp = tmp_path_factory.mktemp('bspline')
    VS.write_tiny_model(tmp)
    rng = np.random.default_rng(7)
    ref_shape, obl_shape = (16, 16, 9), (18, 14, 11)
    ref_aff = _affine(np.diag([1.0, 1.0, 2.5]), ref_shape)
    obl_aff = _affine(G.oblique_linear() @ np.diag([1.0, 1.0, 2.0]), obl_shape)
    shift_aff = ref_aff.copy()
    shift_aff[:3, 3] += ref_aff[:3, :3] @ (0.5, -0.25, 0.0)                         # the same shape, a fraction of a voxel off

    def volume(shape, dtype):
        return np.asfortranarray(((100 + 50 * rng.random(shape)) * (rng.random(shape) > 0.2)).astype(dtype))

    p = {k: str(tmp / f'{k}.nii.gz') for k in ('flair', 't2', 't1', 't2_pre', 't1_pre')}
    V.write_nifti(p['flair'], volume(ref_shape, 'f4'), ref_aff)
    R.write_nifti_typed(p['t2'], volume(obl_shape, 'i2'), affine=obl_aff)
    R.write_nifti_typed(p['t1'], volume(ref_shape, 'i2'), '<', 0.5, 3.0, affine=shift_aff)
    model = VS.model_argv(tmp, 3, 4)
    raw_in = ['--input_flair', p['flair'], '--input_t2', p['t2'], '--input_t1', p['t1']]
    pre_in = ['--input_flair', p['flair'], '--input_t2', p['t2_pre'], '--input_t1', p['t1_pre']]
    jobs = {'cubic_host': raw_in + ['--regrid', '--regrid_interp', 'cubic'],
            'cubic_dev': raw_in + ['--regrid', '--regrid_interp', 'cubic', '--device_intake'], 'pre': pre_in,
            'coreg': raw_in + ['--coregister', '--coregister_strides', '4', '--regrid_interp', 'cubic'],
            'linear_flag': raw_in + ['--regrid', '--regrid_interp', 'linear'], 'no_flag': raw_in + ['--regrid']}
    jobs = {k: model + a + ['--output_dir', str(tmp / k)] for k, a in jobs.items()}
    offline = [VS.regrid_step(p[k], p['flair'], p[k + '_pre'], 'cubic') for k in ('t2', 't1')]
    log = VS.run_plan(tmp, offline + [VS.volume_step(k, argv) for k, argv in jobs.items()], 900)
    return dict(tmp=tmp, paths=p, log=log, pred=lambda k: VS.payload(str(tmp / k / 'predicted_t1ce.nii.gz')))


def _done_out(runs, name):
    """The run's [done] line with its own output directory replaced."""
    return VS.done_line(runs['log'][name]).replace(os.path.join(str(runs['tmp']), name), 'OUT')


def test_cubic_run_writes_the_file_of_the_run_on_resampled_inputs(runs):
    want = runs['pred']('pre')
    assert runs['pred']('cubic_host') == want and runs['pred']('cubic_dev') == want
    assert want != runs['pred']('no_flag')                                         # (the interpolant reaches the prediction)
    for name in ('cubic_host', 'cubic_dev'):
        assert _done_out(runs, name).endswith(' | regrid=T2,T1 | interp=cubic')
    assert ' | interp=' not in _done_out(runs, 'pre') and ' | regrid=' not in _done_out(runs, 'pre')


def test_coregister_with_the_flag(runs):
    line = _done_out(runs, 'coreg')
    assert ' | regrid=T2,T1 | interp=cubic | coreg=' in line
    assert os.path.exists(runs['tmp'] / 'coreg' / 'coreg_t1ce.json') and len(runs['pred']('coreg')) > 0


def test_linear_is_the_default(runs):
    assert runs['pred']('linear_flag') == runs['pred']('no_flag')
    assert _done_out(runs, 'linear_flag') == _done_out(runs, 'no_flag') and _done_out(runs, 'no_flag').endswith(' | regrid=T2,T1')
