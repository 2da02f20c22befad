"""GPU: --regrid.  mud_volume_regrid against the fp64 numpy restatement (tests/volume_regrid_ref.py): exact
for an identity, an integer shift, a flip and a dyadic scale, within one fp32 ulp for an oblique matrix; every stored datatype; nearest
neighbour on a label volume; the C ABI's argument checks; then `predict_volume --regrid` on inputs that lie on three different grids
against the same run on inputs resampled beforehand, byte for byte, through the host path and --device_intake, and the scoring of a
ground truth and a mask on other grids."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import volume_intake_ref as R
import volume_regrid_ref as G
import volume_support as VS

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
CASES = G.EXACT_CASES + ('oblique',)


def _device_regrid(vol, name, mode='linear', scale=(1.0, 0.0), shapes=()):
    """vol: the stored [SX,SY,SZ] array -> (device result as a host [X,Y,Z] array, M, reference shape)."""
    from mudiff_hip import volume_intake as VI
    from mudiff_hip import volume_regrid as VR
    _, sa, rs, ra = G.case(name, vol.shape, *shapes)
    raw = VS.raw_volume(vol, scale, sa)
    M = VR.grid_matrix(sa, ra)
    slope, inter = (raw.slope, raw.inter) if raw.scaled else (1.0, 0.0)
    out = VR.regrid(VI.upload(raw, DEV), raw.code, vol.shape, slope, inter, M, rs, mode)
    assert out.dtype == torch.float32 and tuple(out.shape) == tuple(rs)[::-1]
    return out.cpu().numpy().transpose(2, 1, 0), M, rs


def _within_one_ulp(got, want, src_max):
    """|dev - ref| <= 2^-23 |ref| + 1e-9 max|src|: both sides round an fp64 sum of 8 terms to fp32 once, and their coordinates differ
    by FMA contraction only (~1e-13 voxels) under a continuous interpolant."""
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    bound = 2.0 ** -23 * np.abs(want.astype(np.float64)) + 1e-9 * src_max
    print('max err', err.max(), 'violations', int((err > bound).sum()), 'of', err.size, '| bit-equal', float((got == want).mean()))
    return bool((err <= bound).all())


@pytest.fixture(scope='module')
def source():
    return R.synthetic(G.SRC_SHAPE, 'noise', 'f4', seed=51)


@pytest.mark.parametrize('name', CASES)
def test_trilinear_is_the_reference(source, name):
    got, M, rs = _device_regrid(source, name)
    want = G.trilinear(source, M, rs)
    if name in G.EXACT_CASES:
        assert np.array_equal(got, want)
    else:
        assert _within_one_ulp(got, want, float(np.abs(source).max()))
        assert np.count_nonzero(got) >= 0.4 * got.size                             # (a stray all-zero output must not pass)


def test_trilinear_degenerate_grids(source):
    flat = np.asfortranarray(source[:, :, 8:9])                                    # a single stored plane
    got, M, rs = _device_regrid(flat, 'dyadic')
    assert np.array_equal(got, G.trilinear(flat, M, rs)) and got.any()
    got, M, rs = _device_regrid(flat, 'oblique')
    assert _within_one_ulp(got, G.trilinear(flat, M, rs), float(np.abs(flat).max())) and got.any()
    got, M, rs = _device_regrid(source, 'outside')                                 # wholly outside the source: zeros
    assert not got.any() and np.array_equal(got, G.trilinear(source, M, rs))


def test_a_weight_of_zero_reads_nothing(source):
    """Identity and integer shift are bit-exact next to a NaN and an inf: the neighbours of weight 0 are not multiplied in."""
    vol = source.copy(order='F')
    vol[10, 5, 3], vol[40, 12, 16] = np.nan, np.inf
    for name in ('identity', 'shift'):
        got, M, rs = _device_regrid(vol, name)
        want = G.trilinear(vol, M, rs)
        assert np.array_equal(got, want, equal_nan=True) and int(np.isnan(got).sum()) == 1 and int(np.isinf(got).sum()) == 1
    got, _, _ = _device_regrid(vol, 'identity')
    assert np.array_equal(got, vol, equal_nan=True)


@pytest.mark.parametrize('dtype,scale', [('u1', (1.0, 0.0)), ('i2', (1.0, 0.0)), ('u2', (1.0, 0.0)), ('i4', (1.0, 0.0)), ('f4', (1.0, 0.0)),
                                         ('i2', (0.0123, -5.5))])
def test_every_stored_datatype(dtype, scale):
    vol = R.synthetic(G.SRC_SHAPE, 'noise', dtype, seed=52)
    values = np.asfortranarray(R.values_float32(vol, *scale))                      # what the pipeline sees of this file
    assert R.is_scaled(*scale) == (scale != (1.0, 0.0))
    got, M, rs = _device_regrid(vol, 'oblique', scale=scale)
    assert _within_one_ulp(got, G.trilinear(values, M, rs), float(np.abs(values).max()))
    assert np.count_nonzero(got) >= 0.4 * got.size
    got, M, rs = _device_regrid(vol, 'flip', scale=scale)
    assert np.array_equal(got, G.trilinear(values, M, rs))


@pytest.mark.parametrize('name', CASES)
def test_nearest_on_a_label_volume(name):
    labels = np.asfortranarray(np.random.default_rng(53).integers(0, 5, G.SRC_SHAPE).astype('u1'))
    got, M, rs = _device_regrid(labels, name, mode='nearest')
    want = G.nearest(labels.astype(np.float32), M, rs)
    assert set(np.unique(got).tolist()) <= {0.0, 1.0, 2.0, 3.0, 4.0}
    if name in G.EXACT_CASES:                                                      # (dyadic: 75 % exact ties, resolved by exact arithmetic)
        assert np.array_equal(got, want)
    else:
        skip = G.near_half_integer(M, rs, 1e-9)
        print('excluded', int(skip.sum()), 'of', skip.size)
        assert skip.mean() <= 1e-3 and np.array_equal(got[~skip], want[~skip])
        assert np.count_nonzero(got) >= 0.4 * got.size


def test_c_abi_rejects_bad_arguments_without_launching():
    import mudiff_hip
    lib = mudiff_hip.load()
    src = torch.zeros(16 * 8 * 4, dtype=torch.int16, device=DEV)
    out = torch.full((4, 8, 16), 5.0, device=DEV)
    eye = [1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0, 0]

    def call(s=src, code=4, dims=(16, 8, 4), m=eye, mode=0, size=(16, 8, 4), o=out):
        mm = None if m is None else (C.c_double * 12)(*m)
        return lib.mud_volume_regrid(None if s is None else s.data_ptr(), code, *dims, 1.0, 0.0, mm, mode, *size, None if o is None else o.data_ptr(),
                                     None)

    assert call(o=None) == 1 and b'null' in lib.mud_last_error()
    assert call(size=(0, 8, 4)) == 1 and b'output size' in lib.mud_last_error()
    assert call(mode=7) == 1 and b'mode' in lib.mud_last_error()
    assert call(m=eye[:5] + [float('nan')] + eye[6:]) == 1 and b'finite' in lib.mud_last_error()
    assert call(m=eye[:3] + [float('inf')] + eye[4:]) == 1
    assert call(s=None) == 1 and call(m=None) == 1 and call(code=64) == 1 and call(dims=(16, 0, 4)) == 1 and call(size=(16, 8, -1)) == 1
    torch.cuda.synchronize()
    assert float(out.min()) == 5.0 and float(out.max()) == 5.0                     # nothing was launched
    assert call() == 0                                                             # the library still works afterwards
    torch.cuda.synchronize()
    assert not out.any()


# ---------------------------------------------------------------------------------------------------
# end to end: the tiny model of the other volume tests, inputs on three grids
# ---------------------------------------------------------------------------------------------------
def _affine(lin, centre_of):
    a = np.eye(4)
    a[:3, :3] = lin
    a[:3, 3] = -np.asarray(lin) @ ((np.array(centre_of) - 1) / 2.0)
    return a


@pytest.fixture(scope='module')
def runs(tmp_path_factory):
    """One child process for every sampling run of this module (the library, the checkpoints and torch are loaded once): the log of
    each run, and the exceptions of the runs that must fail."""
    from mudiff_hip import volume as V
    tmp = tmp_path_factory.mktemp('regrid')
    VS.write_tiny_model(tmp)
    rng = np.random.default_rng(7)
    ref_shape, obl_shape = (16, 16, 9), (18, 14, 11)
    ref_aff = _affine(np.diag([1.0, 1.0, 2.5]), ref_shape)
    obl_aff = _affine(G.oblique_linear() @ np.diag([1.0, 1.0, 2.0]), obl_shape)     # its own field of view, thicker planes, tilted
    shift_aff = ref_aff.copy()
    shift_aff[:3, 3] += ref_aff[:3, :3] @ (1.0, -1.0, 0.0)                          # the same shape, one voxel off in x and y

    def volume(shape, dtype):
        return np.asfortranarray(((100 + 50 * rng.random(shape)) * (rng.random(shape) > 0.2)).astype(dtype))

    p = {k: str(tmp / f'{k}.nii.gz') for k in ('flair', 't2', 't1', 't1ce', 'seg', 't2_pre', 't1_pre', 't1ce_pre', 'seg_pre')}
    V.write_nifti(p['flair'], volume(ref_shape, 'f4'), ref_aff)                     # defines the grid
    R.write_nifti_typed(p['t2'], volume(obl_shape, 'i2'), affine=obl_aff)           # oblique, stored as int16
    R.write_nifti_typed(p['t1'], volume(ref_shape, 'i2'), '<', 0.5, 3.0, affine=shift_aff)
    R.write_nifti_typed(p['t1ce'], volume(obl_shape, 'i2'), affine=obl_aff)         # the ground truth, oblique
    R.write_nifti_typed(p['seg'], np.asfortranarray(((rng.random(ref_shape) < 0.3) * 4).astype('u1')), affine=shift_aff)
    model = VS.model_argv(tmp, 3, 4)
    raw_in = ['--input_flair', p['flair'], '--input_t2', p['t2'], '--input_t1', p['t1']]
    pre_in = ['--input_flair', p['flair'], '--input_t2', p['t2_pre'], '--input_t1', p['t1_pre']]
    raw_ev, pre_ev = ['--gt_volume', p['t1ce'], '--eval_mask', p['seg']], ['--gt_volume', p['t1ce_pre'], '--eval_mask', p['seg_pre']]
    jobs = {                                                                       # name: (argv, must raise)
        'regrid_host': (raw_in + ['--regrid'], False), 'regrid_dev': (raw_in + ['--regrid', '--device_intake'], False),
        'regrid_dev_z': (raw_in + ['--regrid', '--device_intake', '--norm', 'zscore'], False),
        'regrid_host_z': (raw_in + ['--regrid', '--norm', 'zscore'], False),
        'pre_host': (pre_in, False), 'pre_host_z': (pre_in + ['--norm', 'zscore'], False),
        'pre_flag_host': (pre_in + ['--regrid'], False), 'pre_flag_dev': (pre_in + ['--regrid', '--device_intake'], False),
        'noflag_host': (raw_in, True), 'noflag_dev': (raw_in + ['--device_intake'], True),
        'score_regrid': (pre_in + raw_ev + ['--regrid'], False), 'score_pre': (pre_in + pre_ev, False), 'score_noflag': (pre_in + raw_ev, True),
    }
    jobs = {k: (model + a + ['--output_dir', str(tmp / k)], bad) for k, (a, bad) in jobs.items()}
    offline = [VS.regrid_step(p[k], p['flair'], p[k + '_pre'], mode) for k, mode in (('t2', 'linear'), ('t1', 'linear'), ('t1ce', 'linear'), ('seg', 'nearest'))]
    log = VS.run_plan(tmp, offline + [VS.volume_step(k, argv, raises=bad) for k, (argv, bad) in jobs.items()], 900)
    return dict(tmp=tmp, paths=p, log=log, pred=lambda k: VS.payload(str(tmp / k / 'predicted_t1ce.nii.gz')))


def test_regrid_run_writes_the_file_of_the_run_on_resampled_inputs(runs):
    want = runs['pred']('pre_host')
    assert runs['pred']('regrid_host') == want and runs['pred']('regrid_dev') == want
    want_z = runs['pred']('pre_host_z')
    assert runs['pred']('regrid_host_z') == want_z and runs['pred']('regrid_dev_z') == want_z and want_z != want
    for name in ('regrid_host', 'regrid_dev'):
        assert VS.done_line(runs['log'][name]['stdout']).endswith(' | regrid=T2,T1')
    for name in ('regrid_host_z', 'regrid_dev_z'):
        assert VS.done_line(runs['log'][name]['stdout']).endswith(' | norm=zscore | regrid=T2,T1')
    # the inputs really were on other grids: the resampled T1 differs from the stored one although the shapes agree
    from mudiff_hip import volume as V
    t1, t1_pre = V.read_nifti(runs['paths']['t1'])[0], V.read_nifti(runs['paths']['t1_pre'])[0]
    assert t1.shape == t1_pre.shape and not np.array_equal(t1, t1_pre)
    assert np.array_equal(t1_pre[1:, :-1], t1[:-1, 1:]) and not t1_pre[0].any() and not t1_pre[:, -1].any()      # the one-voxel shift, exactly
    assert np.count_nonzero(V.read_nifti(runs['paths']['t2_pre'])[0]) >= 0.4 * 16 * 16 * 9


def test_without_the_flag_nothing_changes(runs):
    p = runs['paths']
    assert runs['log']['noflag_host']['error'] == 'All input volumes must share shape. Got (18, 14, 11) vs (16, 16, 9) for T2'
    assert runs['log']['noflag_dev']['error'] == f"All input volumes must share shape. Got (18, 14, 11) vs (16, 16, 9) for {p['t2']}"
    assert ' | regrid=' not in VS.done_line(runs['log']['pre_host']['stdout'])


def test_the_flag_on_inputs_that_share_a_grid_changes_nothing(runs):
    want = runs['pred']('pre_host')
    assert runs['pred']('pre_flag_host') == want and runs['pred']('pre_flag_dev') == want
    tmp = str(runs['tmp'])
    lines = {k: VS.done_line(runs['log'][k]['stdout']).replace(os.path.join(tmp, k), 'OUT') for k in ('pre_host', 'pre_flag_host', 'pre_flag_dev')}
    assert lines['pre_flag_host'] == lines['pre_host'] and lines['pre_flag_dev'] == lines['pre_host']


def test_scoring_a_ground_truth_and_a_mask_on_other_grids(runs):
    tmp = runs['tmp']
    got, want = (json.load(open(tmp / k / 'metrics_t1ce.json')) for k in ('score_regrid', 'score_pre'))
    assert got == want and got['regions'] == ['slab', 'brain', 'tumor', 'healthy'] and got['metrics']['tumor']['voxels'] > 0
    assert runs['pred']('score_regrid') == runs['pred']('pre_host')                # scoring does not change the prediction
    assert VS.done_line(runs['log']['score_regrid']['stdout']).endswith(' | regrid=gt_volume,eval_mask') and ' | regrid=' not in VS.done_line(runs['log']['score_pre']['stdout'])
    assert runs['log']['score_noflag']['error'].startswith('--gt_volume / --eval_mask: prediction (16, 16, 9) and ground truth (18, 14, 11) '
                                                          'differ in shape')
    assert not os.path.exists(tmp / 'score_noflag' / 'predicted_t1ce.nii.gz')      # refused before any sampling
