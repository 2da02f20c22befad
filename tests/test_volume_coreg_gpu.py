"""GPU: --coregister.  mud_volume_joint_hist against the fp64 numpy restatement (tests/volume_coreg_ref.py) on
volume_regrid_ref's grids: equal counts for an identity, a shift, a flip and a dyadic scale, within twice the number of samples that sit
on a bin edge for an oblique matrix; equality with a histogram of mud_volume_regrid's output; every stored datatype on either side;
NaN voxels; an empty overlap; two runs; the C ABI's argument checks; then the recovery of a known rigid motion on the device against
the same search on the host, and `predict_volume --coregister` end to end through the host path and --device_intake."""
import ctypes as C
import json
import os
import warnings

import numpy as np
import pytest
import torch

import volume_coreg_ref as K
import volume_intake_ref as R
import volume_regrid_ref as G
import volume_support as VS

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
STRIDES, BINS = (1, 2, 3), (32, 64)


def _device_hist(fix, mov, M, stride, ranges, bins, fix_scale=(1.0, 0.0), mov_scale=(1.0, 0.0)):
    """fix / mov: the stored [X,Y,Z] arrays -> host int64 [bins, bins]."""
    from mudiff_hip import volume_coreg as VC
    from mudiff_hip import volume_intake as VI
    sides = []
    for vol, scale in ((fix, fix_scale), (mov, mov_scale)):
        raw = VS.raw_volume(vol, scale)
        sides += [VI.upload(raw, DEV), (raw.code, vol.shape) + ((raw.slope, raw.inter) if raw.scaled else (1.0, 0.0))]
    out = VC.joint_hist(*sides, M, stride, ranges, bins)
    assert out.dtype == np.int64 and out.shape == (bins, bins)
    return out


@pytest.fixture(scope='module')
def source():
    return R.synthetic(G.SRC_SHAPE, 'noise', 'f4', seed=51)


def _fixed(shape):
    return R.synthetic(tuple(shape), 'noise', 'f4', seed=61)


@pytest.mark.parametrize('name', G.EXACT_CASES + ('oblique',))
def test_histogram_is_the_reference(source, name):
    _, sa, rs, ra = G.case(name)
    M, fix = G.matrix(sa, ra), _fixed(G.case(name)[2])
    for stride in STRIDES:
        for bins in BINS:
            ranges = K.ranges_of(fix, source, bins)
            want, info = K.joint_hist(fix, source, M, stride, ranges, bins, details=True)
            got = _device_hist(fix, source, M, stride, ranges, bins)
            diff = int(np.abs(got - want).sum())
            print(name, stride, bins, 'counted', info['counted'], 'of', info['points'], 'sum|dev - ref|', diff)
            assert info['counted'] > 0 and int(got.sum()) == info['counted']
            if name in G.EXACT_CASES:
                assert np.array_equal(got, want)
            else:
                ne = K.n_edge(info, ranges, bins, float(np.abs(source).max()), source.shape)
                assert ne <= 1e-3 * info['counted'] and info['counted'] >= 0.4 * info['points']
                assert diff <= 2 * ne


@pytest.mark.parametrize('name', G.EXACT_CASES)
def test_histogram_equals_the_histogram_of_the_regrid_kernel(source, name):
    from mudiff_hip import volume_intake as VI
    from mudiff_hip import volume_regrid as VR
    _, sa, rs, ra = G.case(name)
    M, fix = G.matrix(sa, ra), _fixed(rs)
    out = VR.regrid(VI.upload(VS.raw_volume(source), DEV), 16, source.shape, 1.0, 0.0, M, rs).cpu().numpy().transpose(2, 1, 0)
    for stride in (1, 3):
        ranges = K.ranges_of(fix, source, 32)
        _, info = K.joint_hist(fix, source, M, stride, ranges, 32, details=True)
        f, m = (a[::stride, ::stride, ::stride][info['inside']] for a in (fix, out))
        want = np.bincount(K.bin_of(f, ranges[0], ranges[1], 32) * 32 + K.bin_of(m, ranges[2], ranges[3], 32), minlength=1024).reshape(32, 32)
        assert np.array_equal(_device_hist(fix, source, M, stride, ranges, 32), want) and want.sum() > 0


@pytest.mark.parametrize('dtype,scale', [('u1', (1.0, 0.0)), ('i2', (1.0, 0.0)), ('u2', (1.0, 0.0)), ('i4', (1.0, 0.0)), ('f4', (1.0, 0.0)),
                                         ('i2', (0.0123, -5.5))])
def test_every_stored_datatype_on_either_side(dtype, scale):
    _, sa, rs, ra = G.case('flip')
    M = G.matrix(sa, ra)
    typed_src, typed_fix = R.synthetic(G.SRC_SHAPE, 'noise', dtype, seed=52), R.synthetic(rs, 'noise', dtype, seed=62)
    plain_src, plain_fix = R.synthetic(G.SRC_SHAPE, 'noise', 'f4', seed=51), _fixed(rs)
    for fix, mov, fs, ms in ((plain_fix, typed_src, (1.0, 0.0), scale), (typed_fix, plain_src, scale, (1.0, 0.0)), (typed_fix, typed_src, scale, scale)):
        fv, mv = np.asfortranarray(R.values_float32(fix, *fs)), np.asfortranarray(R.values_float32(mov, *ms))
        ranges = K.ranges_of(fv, mv, 32)
        want = K.joint_hist(fv, mv, M, 2, ranges, 32)
        assert np.array_equal(_device_hist(fix, mov, M, 2, ranges, 32, fs, ms), want) and want.sum() > 0 and np.count_nonzero(want) > 8


def test_a_nan_voxel_in_either_volume_is_not_counted(source):
    _, sa, rs, ra = G.case('shift')
    M = G.matrix(sa, ra)
    fix, mov = _fixed(rs).copy(order='F'), source.copy(order='F')
    ranges = K.ranges_of(fix, mov, 32)
    clean = K.joint_hist(fix, mov, M, 1, ranges, 32)
    fix[10, 5, 3], fix[11, 5, 3] = np.nan, np.inf           # both map inside the source under the shift (3, -2, 1)
    mov[40, 12, 16] = np.nan                                 # fixed voxel (37, 14, 15)
    want, info = K.joint_hist(fix, mov, M, 1, ranges, 32, details=True)
    assert int(clean.sum()) - info['counted'] == 3
    got = _device_hist(fix, mov, M, 1, ranges, 32)
    assert np.array_equal(got, want) and int(got.sum()) == info['counted']


def test_an_empty_overlap_gives_an_empty_histogram(source):
    from mudiff_hip import volume_coreg as VC
    _, sa, rs, ra = G.case('outside')
    fix = _fixed(rs)
    got = _device_hist(fix, source, G.matrix(sa, ra), 1, K.ranges_of(fix, source, 32), 32)
    assert not got.any() and VC.nmi(got) == 0.0


def test_two_runs_are_bit_identical(source):
    _, sa, rs, ra = G.case('oblique')
    fix = _fixed(rs)
    ranges = K.ranges_of(fix, source, 64)
    a, b = (_device_hist(fix, source, G.matrix(sa, ra), 1, ranges, 64) for _ in range(2))
    assert np.array_equal(a, b) and a.sum() > 0


def test_c_abi_rejects_bad_arguments_without_launching():
    import mudiff_hip
    lib = mudiff_hip.load()
    fix = torch.zeros(16 * 8 * 4, dtype=torch.int16, device=DEV)
    mov = torch.zeros(12 * 8 * 4, dtype=torch.float32, device=DEV)
    hist = torch.full((32 * 32,), 5, dtype=torch.int32, device=DEV)
    eye = [1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0, 0]
    nan, inf = float('nan'), float('inf')

    def call(f=fix, fdt=4, fdims=(16, 8, 4), v=mov, vdt=16, vdims=(12, 8, 4), m=eye, stride=1, ranges=(0.0, 1.0, 0.0, 1.0), bins=32, h=hist):
        mm = None if m is None else (C.c_double * 12)(*m)
        p = lambda t: None if t is None else t.data_ptr()      # noqa: E731
        return lib.mud_volume_joint_hist(p(f), fdt, *fdims, 1.0, 0.0, p(v), vdt, *vdims, 1.0, 0.0, mm, stride, *ranges, bins, p(h), None)

    assert call(h=None) == 1 and b'null' in lib.mud_last_error()
    assert call(f=None) == 1 and call(v=None) == 1 and call(m=None) == 1
    assert call(fdims=(0, 8, 4)) == 1 and call(vdims=(12, 8, -1)) == 1
    assert call(stride=0) == 1 and b'stride' in lib.mud_last_error()
    assert call(stride=-2) == 1
    assert call(bins=1) == 1 and b'bins' in lib.mud_last_error()
    assert call(bins=65) == 1
    assert call(fdt=64) == 1 and b'datatype' in lib.mud_last_error()
    assert call(vdt=3) == 1
    assert call(m=eye[:5] + [nan] + eye[6:]) == 1 and b'finite' in lib.mud_last_error()
    assert call(m=eye[:3] + [inf] + eye[4:]) == 1
    for i in range(4):
        for bad in (nan, inf):
            r = [0.0, 1.0, 0.0, 1.0]
            r[i] = bad
            assert call(ranges=tuple(r)) == 1 and b'finite' in lib.mud_last_error()
    torch.cuda.synchronize()
    assert int(hist.min()) == 5 and int(hist.max()) == 5                           # nothing was launched, nothing cleared
    assert call() == 0                                                             # the library still works afterwards
    torch.cuda.synchronize()
    assert int(hist.sum()) == 12 * 8 * 4 and int(hist[0]) == 12 * 8 * 4            # the overlap of two zero volumes, all in bin (0, 0)


# ---------------------------------------------------------------------------------------------------
# recovery of a known motion
# ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def subject():
    from mudiff_hip import volume_coreg as VC
    t, mask = K.head()
    A = np.eye(4)
    centre = VC.grid_centre(K.HEAD_SHAPE, A)
    M_true = VC.sampling_matrix(A, VC.rigid_world(K.TRUE_PARAMS, centre), A)
    return dict(t=t, mask=mask, A=A, centre=centre, M_true=M_true, fix=K.fixed_contrast(t, mask),
                mov=K.moved(K.moving_contrast(t, mask), M_true, mask=mask))


def test_device_recovery_meets_the_bar_and_agrees_with_the_host_search(subject):
    """Bar: mean displacement error <= 0.25 voxel, max <= 0.5; the device's parameters within 0.05 mm / 0.05 deg of the same powell() on
    the numpy histogram; the two cost surfaces equal except at bin edges (sum |dev - ref| <= 2 n_edge at the truth); and the volume
    resampled through the W found differs from the one resampled through the true motion written into its header by no more than a
    displacement of 0.5 voxel can change a trilinear interpolant: sqrt(3) * 0.5 * the largest step between adjacent voxels."""
    from mudiff_hip import volume_coreg as VC
    from mudiff_hip import volume_regrid as VR
    s = subject
    fixed_raw, moving_raw = VS.raw_volume(s['fix'], affine=s['A']), VS.raw_volume(s['mov'], affine=s['A'])
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        W, rep = VC.coregister(fixed_raw, moving_raw, DEV)
    M = VC.sampling_matrix(s['A'], W, s['A'])
    mean, worst = K.displacement_error(M, s['M_true'], s['mask'])
    ranges = K.ranges_of(s['fix'], s['mov'], 32)
    assert VC.bin_ranges(fixed_raw, moving_raw, 32) == ranges

    def cost_at(params, stride):
        Mp = VC.sampling_matrix(s['A'], VC.rigid_world(params, s['centre']), s['A'])
        return VC.nmi(K.joint_hist(s['fix'], s['mov'], Mp, stride, ranges, 32))

    _, host = VC.finish(cost_at, s['centre'], (4, 2, 1), 32, 20.0, 15.0)
    delta = np.abs(np.array(rep['params']) - np.array(host['params']))
    print('device', rep['params'], (mean, worst), rep['nmi_identity'], rep['nmi_result'], rep['evaluations'], '| host', host['params'],
          host['evaluations'], '| delta', delta)
    assert rep['accepted'] and mean <= K.BAR_MEAN and worst <= K.BAR_MAX
    assert delta[:3].max() <= 0.05 and delta[3:].max() <= 0.05
    want, info = K.joint_hist(s['fix'], s['mov'], s['M_true'], 1, ranges, 32, details=True)
    ne = K.n_edge(info, ranges, 32, float(np.abs(s['mov']).max()), s['mov'].shape)
    got = _device_hist(s['fix'], s['mov'], s['M_true'], 1, ranges, 32)
    print('at the truth: sum|dev - ref|', int(np.abs(got - want).sum()), 'n_edge', ne, 'nmi', VC.nmi(got), VC.nmi(want))
    assert int(np.abs(got - want).sum()) <= 2 * ne and int(got.sum()) == info['counted']
    # regrid_to(world=W) against plain regrid of the same voxels whose header carries the true motion
    by_search = VR.regrid_to(moving_raw, K.HEAD_SHAPE, s['A'], DEV, world=W)
    by_header = VR.regrid_to(VS.raw_volume(s['mov'], affine=np.linalg.inv(VC.rigid_world(K.TRUE_PARAMS, s['centre'])) @ s['A']), K.HEAD_SHAPE, s['A'], DEV)
    assert isinstance(by_search, VR.RegriddedVolume) and isinstance(by_header, VR.RegriddedVolume)
    a, b = by_search.values_float32().astype(np.float64), by_header.values_float32().astype(np.float64)
    step = max(float(np.abs(np.diff(s['mov'].astype(np.float64), axis=ax)).max()) for ax in range(3))
    inner = (slice(4, -4),) * 3                                                    # (away from the field of view's border: zero padding)
    print('regridded inputs: max |search - header|', np.abs(a - b)[inner].max(), 'bound', np.sqrt(3) * K.BAR_MAX * step)
    assert np.abs(a - b)[inner].max() <= np.sqrt(3) * K.BAR_MAX * step
    assert VR.regrid_to(moving_raw, K.HEAD_SHAPE, s['A'], DEV, world=np.eye(4)) is moving_raw      # W = I: today's path


def test_a_moving_volume_that_does_not_overlap_is_left_alone(subject):
    from mudiff_hip import volume_coreg as VC
    far = subject['A'].copy()
    far[0, 3] = 1000.0
    with pytest.warns(RuntimeWarning, match='did not improve'):
        W, rep = VC.coregister(VS.raw_volume(subject['fix'], affine=subject['A']), VS.raw_volume(subject['mov'], affine=far), DEV, strides=(4,))
    assert np.array_equal(W, np.eye(4)) and not rep['accepted'] and rep['nmi_identity'] == 0.0 and rep['nmi_result'] == 0.0


# ---------------------------------------------------------------------------------------------------
# end to end: the tiny model of the other volume tests, one subject whose T2 and T1 moved
# ---------------------------------------------------------------------------------------------------
PARAMS_T1 = (-1.5, 2.0, 0.8, -2.5, 3.0, 1.5)


@pytest.fixture(scope='module')
def runs(tmp_path_factory, subject):
    from mudiff_hip import volume as V
    from mudiff_hip import volume_coreg as VC
    s = subject
    tmp = tmp_path_factory.mktemp('coreg')
    VS.write_tiny_model(tmp)
    M_t1 = VC.sampling_matrix(s['A'], VC.rigid_world(PARAMS_T1, s['centre']), s['A'])
    t1 = K.moved(np.asfortranarray(((500.0 + 300.0 * np.cos(5.0 * s['t'])) * s['mask']).astype(np.float32)), M_t1, seed=13, mask=s['mask'])
    p = {k: str(tmp / f'{k}.nii.gz') for k in ('flair', 't2', 't1')}
    V.write_nifti(p['flair'], s['fix'], s['A'])
    V.write_nifti(p['t2'], s['mov'], s['A'])
    V.write_nifti(p['t1'], t1, s['A'])
    model = VS.model_argv(tmp, 2, 5, '--resize_back', '--input_flair', p['flair'], '--input_t2', p['t2'], '--input_t1', p['t1'])
    jobs = {'coreg_host': ['--coregister'], 'coreg_dev': ['--coregister', '--device_intake'], 'plain_host': [], 'plain_dev': ['--device_intake'],
            'regrid_host': ['--regrid']}
    jobs = {k: model + a + ['--output_dir', str(tmp / k)] for k, a in jobs.items()}
    log = VS.run_plan(tmp, [VS.volume_step(k, argv) for k, argv in jobs.items()], 900)
    return dict(tmp=tmp, log=log, M_t1=M_t1, pred=lambda k: VS.payload(str(tmp / k / 'predicted_t1ce.nii.gz')))


def test_predict_volume_coregister_end_to_end(runs, subject):
    from mudiff_hip import volume_coreg as VC
    s, tmp = subject, runs['tmp']
    for name in ('coreg_host', 'coreg_dev'):
        rep = json.load(open(tmp / name / 'coreg_t1ce.json'))
        assert list(rep) == ['T2', 'T1']                                           # (FLAIR is the first input: the fixed volume)
        for key, truth in (('T2', s['M_true']), ('T1', runs['M_t1'])):
            M = VC.sampling_matrix(s['A'], np.array(rep[key]['W']), s['A'])
            mean, worst = K.displacement_error(M, truth, s['mask'])
            print(name, key, rep[key]['params'], (mean, worst), rep[key]['evaluations'])
            assert rep[key]['accepted'] and mean <= K.BAR_MEAN and worst <= K.BAR_MAX
        assert ' | regrid=T2,T1 | coreg=T2:' in VS.done_line(runs['log'][name]) and 'mm/' in VS.done_line(runs['log'][name]) and VS.done_line(runs['log'][name]).count('deg') == 2
    assert json.load(open(tmp / 'coreg_host' / 'coreg_t1ce.json')) == json.load(open(tmp / 'coreg_dev' / 'coreg_t1ce.json'))
    assert runs['pred']('coreg_host') == runs['pred']('coreg_dev')                 # host file == device file, byte for byte
    assert runs['pred']('coreg_host') != runs['pred']('plain_host')                # and the alignment reached the sampler


def test_without_the_flag_nothing_changes(runs):
    tmp = runs['tmp']
    want = runs['pred']('plain_host')
    assert runs['pred']('plain_dev') == want and runs['pred']('regrid_host') == want       # (the inputs share a grid: --regrid is a no-op)
    for name in ('plain_host', 'plain_dev', 'regrid_host'):
        assert ' | coreg=' not in VS.done_line(runs['log'][name]) and ' | regrid=' not in VS.done_line(runs['log'][name])
        assert not os.path.exists(tmp / name / 'coreg_t1ce.json')
    assert VS.done_line(runs['log']['plain_host']).endswith('| slices=16..20')
