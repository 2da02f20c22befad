"""GPU: --reorient (csrc/volume_reorient.hip, mudiff_hip.volume_reorient) against the numpy restatement
(tests/volume_reorient_ref.py).  Every comparison is exact: the kernel moves elements and never interprets them.

All 48 permutations-with-flips at every element width on shapes that are no multiple of the tile in any position, one that is, one with
a unit axis and a single voxel; nothing written out of range; the C ABI's refusals; volume_reorient.reorient on scaled int16, uint16 and
fp32 with non-finite voxels; then `predict_volume --reorient --reorient_back` end to end: the same phantom stored LPS, RAS and sagittally
gives the same condition stacks and the same voxels at the same world positions, and the RAS files without the flag do not."""
import ctypes as C
import itertools
import json
import os
import types

import numpy as np
import pytest
import torch

import volume_intake_ref as I
import volume_reorient_ref as R
import volume_support as VS

pytestmark = pytest.mark.gpu

SHAPES = [(37, 29, 23), (5, 4, 3), (70, 19, 11), (33, 1, 65), (1, 1, 1), (64, 64, 2)]
COMBOS = [(perm, flip) for perm in itertools.permutations(range(3)) for flip in itertools.product((False, True), repeat=3)]
SIGNED = {1: np.int8, 2: np.int16, 4: np.int32, 8: np.int64}
SENTINEL = 0xA5
SAGITTAL = 'PSL'


def _plan(perm, flip, shape):
    from mudiff_hip import volume_reorient as VO
    return VO.ReorientPlan(perm, flip, shape, np.eye(4), '', '')


def _device(vol):
    """An [X, Y, Z] unsigned volume -> its flat device tensor (the signed dtype of the same width: torch has no wide unsigned ones)."""
    flat = np.ascontiguousarray(vol.reshape(-1, order='F'))
    return torch.from_numpy(flat.view(SIGNED[flat.dtype.itemsize])).cuda()


def _host(dev, dtype, shape):
    return dev.cpu().numpy().view(dtype).reshape(shape, order='F')


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(str(v) for v in s))
def test_kernel_all_48_at_every_width(shape):
    from mudiff_hip import ops
    assert len(COMBOS) == 48
    for width in (1, 2, 4, 8):
        vol = R.labelled(shape, width)
        dev = _device(vol)
        for perm, flip in COMBOS:
            p = _plan(perm, flip, shape)
            out = ops.volume_reorient(dev, width, shape, p)
            assert out.dtype == dev.dtype and out.shape == dev.shape
            want = R.apply(vol, perm, flip)
            assert np.array_equal(_host(out, vol.dtype, p.shape), want), (width, perm, flip)
            assert torch.equal(ops.volume_reorient(dev, width, shape, p), out)                          # two runs: the same bits
            assert torch.equal(ops.volume_reorient(out, width, p.shape, p.inverse()), dev), (width, perm, flip)      # and back


def _call(src, width, shape, perm, mask, dst):
    from mudiff_hip import load
    from mudiff_hip import stream_ptr
    return load().mud_volume_reorient(C.c_void_p(src), width, *shape, *perm, mask, C.c_void_p(dst), stream_ptr())


@pytest.mark.parametrize('shape', [(37, 29, 23), (70, 19, 11)], ids=['37x29x23', '70x19x11'])
def test_nothing_is_written_out_of_range(shape):
    """Source and destination sit inside larger buffers full of a sentinel, aligned to their elements only."""
    n = int(np.prod(shape))
    for width in (1, 2, 4, 8):
        vol = R.labelled(shape, width)
        payload = torch.from_numpy(np.ascontiguousarray(vol.reshape(-1, order='F')).view(np.uint8)).cuda()
        a, b = 4096 + width, 4096 + 3 * width
        src = torch.full((a + n * width + 4096,), SENTINEL, dtype=torch.uint8, device='cuda')
        src[a:a + n * width] = payload
        src_before = src.clone()
        for perm, flip in COMBOS:
            dst = torch.full((b + n * width + 4096,), SENTINEL, dtype=torch.uint8, device='cuda')
            mask = sum(1 << o for o, f in enumerate(flip) if f)
            assert _call(src.data_ptr() + a, width, shape, perm, mask, dst.data_ptr() + b) == 0
            assert bool((dst[:b] == SENTINEL).all()) and bool((dst[b + n * width:] == SENTINEL).all()), (width, perm, flip)
            got = dst[b:b + n * width].cpu().numpy().view(vol.dtype).reshape(tuple(shape[q] for q in perm), order='F')
            assert np.array_equal(got, R.apply(vol, perm, flip)), (width, perm, flip)
        assert torch.equal(src, src_before)


def test_cabi_refusals():
    from mudiff_hip import load
    shape, n = (6, 5, 4), 120
    src = torch.arange(n * 8, dtype=torch.uint8, device='cuda')
    dst = torch.full((n * 8,), SENTINEL, dtype=torch.uint8, device='cuda')
    s, d = src.data_ptr(), dst.data_ptr()
    ok = ((0, 1, 2), 0)
    refused = [
        (s, 3, shape, *ok, d), (s, 0, shape, *ok, d), (s, 16, shape, *ok, d), (s, -4, shape, *ok, d),              # the element width
        (s, 4, shape, (0, 0, 1), 0, d), (s, 4, shape, (0, 1, 3), 0, d), (s, 4, shape, (-1, 1, 2), 0, d), (s, 4, shape, (2, 2, 2), 0, d),
        (s, 4, shape, (0, 1, 2), 8, d), (s, 4, shape, (0, 1, 2), -1, d),                                            # the flip mask
        (s, 4, (-6, 5, 4), *ok, d), (s, 4, (6, 5, -4), *ok, d), (s, 4, (-6, -5, 4), *ok, d),                         # a negative extent
        (s, 1, (2048, 2048, 512), *ok, d), (s, 1, (65536, 65536, 1), *ok, d), (s, 1, (1, 1 << 30, 2), (2, 0, 1), 0, d),      # >= 2^31 voxels
        (s, 4, shape, *ok, s), (s, 4, shape, (1, 0, 2), 3, s), (s, 4, shape, *ok, s + 4), (s + 8, 4, shape, *ok, s),      # src == dst, overlap
        (0, 4, shape, *ok, d), (s, 4, shape, *ok, 0), (s + 2, 4, shape, *ok, d), (s, 8, shape, *ok, d + 4),          # null, misaligned
    ]
    for args in refused:
        src_before = src.clone()
        assert _call(*args) != 0, args
        assert load().mud_last_error().decode().startswith('mud_volume_reorient: '), args
        torch.cuda.synchronize()
        assert bool((dst == SENTINEL).all()) and torch.equal(src, src_before), args
    for empty in ((0, 5, 4), (6, 0, 4), (6, 5, 0), (0, 0, 0)):                 # a volume without voxels: nothing launched, success
        for perm in ((0, 1, 2), (2, 0, 1)):
            assert _call(s, 4, empty, perm, 5, d) == 0 and _call(0, 4, empty, perm, 5, 0) == 0
    torch.cuda.synchronize()
    assert bool((dst == SENTINEL).all())
    from mudiff_hip import MudiffHipError, ops
    flat = torch.zeros(n, dtype=torch.int32, device='cuda')
    for bad in (lambda: ops.volume_reorient(flat, 2, shape, _plan((0, 1, 2), (True, False, False), shape)),
                lambda: ops.volume_reorient(flat, 4, (6, 5, 5), _plan((0, 1, 2), (True, False, False), (6, 5, 5))),
                lambda: ops.volume_reorient(flat.cpu(), 4, shape, _plan((0, 1, 2), (True, False, False), shape)),
                lambda: ops.volume_reorient(flat, 4, shape, types.SimpleNamespace(perm=(0, 0, 2), flip=(False,) * 3))):
        with pytest.raises(MudiffHipError):
            bad()
    assert ops.volume_reorient(flat[:0], 4, (0, 5, 4), _plan((1, 0, 2), (False,) * 3, (0, 5, 4))).numel() == 0


# ---------------------------------------------------------------------------------------------------
# volume_reorient.reorient on files
# ---------------------------------------------------------------------------------------------------
def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(f'u{a.dtype.itemsize}')


@pytest.mark.parametrize('kind', ['int16_scaled', 'uint16', 'float32_nonfinite'])
@pytest.mark.parametrize('code', ['RAS', SAGITTAL])
def test_reorient_keeps_the_stored_volume(tmp_path, kind, code):
    from mudiff_hip import volume_intake as VI, volume_reorient as VO
    shape = (37, 29, 23)
    lps_affine = np.array([[-1., 0, 0, 18], [0, -2, 0, 29], [0, 0, 0.5, -4], [0, 0, 0, 1]])
    slope, inter = 0.0, 0.0
    if kind == 'int16_scaled':
        lps, slope, inter = I.synthetic(shape, 'noise', '<i2', seed=3), 0.25, -3.0
    elif kind == 'uint16':
        lps = R.labelled(shape, 2)
        assert int(lps.max()) > 40000
    else:
        lps = I.synthetic(shape, 'noise', '<f4', seed=4)
        lps.view(np.uint32)[3, 4, 5], lps[7, 8, 9], lps[30, 2, 20] = 0x7FC00123, np.inf, -np.inf      # a NaN with a payload, both infinities
    stored, affine = R.stored_as(lps, lps_affine, code)
    raw = VI.read_nifti_raw(I.write_nifti_typed(tmp_path / 'v.nii.gz', stored, slope=slope, inter=inter, affine=affine))
    assert np.array_equal(_bits(raw.data), _bits(stored.reshape(-1, order='F')))
    out, entry = VO.reorient(raw, torch.device('cuda:0'), 'LPS')
    assert isinstance(out, VO.ReorientedVolume) and entry['moved'] and (entry['from'], entry['to']) == (code, 'LPS')
    assert (out.code, out.endian, out.slope, out.inter) == (raw.code, raw.endian, raw.slope, raw.inter) and out.scaled == raw.scaled
    assert out.shape == shape and out.dev.is_cuda and out.dev.dim() == 1 and out.dev.element_size() == lps.dtype.itemsize
    assert out.data.dtype == raw.data.dtype and np.array_equal(_bits(out.data), _bits(lps.reshape(-1, order='F')))      # bit patterns
    p = VO.plan(raw.shape, raw.header.world_affine, 'LPS')
    assert np.array_equal(_bits(out.values_float64()), _bits(R.apply(raw.values_float64(), p.perm, p.flip)))
    assert np.array_equal(out.affine, lps_affine) and np.array_equal(out.header.world_affine, lps_affine) and out.header.shape == shape
    assert out.header._get('2f', 112) == raw.header._get('2f', 112) and out.header._get('h', 70) == raw.header._get('h', 70)
    assert VI.upload(out, torch.device('cuda:0')).data_ptr() == out.dev.data_ptr()                 # handed on as it is
    again, entry = VO.reorient(out, torch.device('cuda:0'), 'LPS')                                # stored LPS already: itself, no launch
    assert again is out and not entry['moved']
    same = VI.read_nifti_raw(I.write_nifti_typed(tmp_path / 'lps.nii.gz', lps, slope=slope, inter=inter, affine=lps_affine))
    assert VO.reorient(same, torch.device('cuda:0'))[0] is same


# ---------------------------------------------------------------------------------------------------
# end to end: the tiny model of the other volume tests on one phantom stored three ways
# ---------------------------------------------------------------------------------------------------
SHAPE = (16, 16, 9)                                  # a slab of 7 planes at --slice_half_range 3: the least the 7 x 7 x 7 SSIM window takes
LPS_AFFINE = np.array([[-1., 0, 0, 8], [0, -1, 0, 9], [0, 0, 1, -3], [0, 0, 0, 1]])


def _phantom(seed):
    rng = np.random.default_rng(seed)
    x, y, z = np.meshgrid(*[np.arange(s) for s in SHAPE], indexing='ij')
    inside = ((x - 6.0) / 5.5) ** 2 + ((y - 9.0) / 4.5) ** 2 + ((z - 4.5) / 4.4) ** 2 < 1          # off-centre: its mirror image differs
    return np.asfortranarray(np.where(inside, rng.integers(50, 1500, SHAPE) + 40 * x + 25 * y, 0).astype('<i2'))


def _read(path):
    from mudiff_hip import volume as V
    vol, affine, _ = V.read_nifti(str(path))
    return np.asarray(vol), np.asarray(affine)


@pytest.fixture(scope='module')
def runs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp('reorient')
    VS.write_tiny_model(tmp)
    vols = {'flair': _phantom(21), 't2': _phantom(22), 't1': _phantom(23), 'gt': _phantom(24)}
    vols['mask'] = np.asfortranarray((vols['gt'] > 1200).astype(np.uint8))
    files = {}
    for code in ('LPS', 'RAS', SAGITTAL):
        for k, vol in vols.items():
            stored, affine = R.stored_as(vol, LPS_AFFINE, code)
            files[code, k] = I.write_nifti_typed(tmp / f'{code}_{k}.nii.gz', stored, affine=affine)
    model = VS.model_argv(tmp, 3, 7)
    inputs = lambda code: ['--input_flair', files[code, 'flair'], '--input_t2', files[code, 't2'], '--input_t1', files[code, 't1']]      # noqa: E731
    ev = lambda code: ['--gt_volume', files[code, 'gt'], '--eval_mask', files[code, 'mask']]      # noqa: E731
    back = ['--reorient', '--reorient_back']
    jobs = {'lps_host': inputs('LPS') + ev('LPS'), 'lps_dev': inputs('LPS') + ['--device_intake'],
            'ras_host': inputs('RAS') + ev('RAS') + back, 'ras_dev': inputs('RAS') + back + ['--device_intake'],
            'sag_host': inputs(SAGITTAL) + back, 'sag_dev': inputs(SAGITTAL) + back + ['--device_intake'],
            'ras_plain': inputs('RAS')}
    jobs = {k: model + a + ['--output_dir', str(tmp / k)] for k, a in jobs.items()}
    log = VS.run_plan(tmp, [VS.volume_step(k, argv, stacks=True) for k, argv in jobs.items()], 600, ignore='RuntimeWarning')
    return dict(tmp=tmp, log=log, stacks={k: VS.load_stacks(tmp, k) for k in jobs}, files=files)


def test_equivariance_end_to_end(runs):
    tmp = runs['tmp']
    lps_pred, lps_affine = _read(tmp / 'lps_host' / 'predicted_t1ce.nii.gz')
    assert lps_pred.shape == SHAPE and np.array_equal(lps_affine, LPS_AFFINE) and float(np.abs(lps_pred).max()) > 0
    assert np.array_equal(lps_pred, _read(tmp / 'lps_dev' / 'predicted_t1ce.nii.gz')[0])
    for kind in ('host', 'dev'):
        want = runs['stacks'][f'lps_{kind}']
        assert len(want) == 3
        for stored, code in (('ras', 'RAS'), ('sag', SAGITTAL)):
            name = f'{stored}_{kind}'
            got = runs['stacks'][name]                                                   # the condition stacks: bit-equal to the LPS run's
            assert all(g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w) for g, w in zip(got, want)), name
            # the prediction: the same voxels at the same world positions, in the input's own storage order
            pred, affine = _read(tmp / name / 'predicted_t1ce.nii.gz')
            want_pred, want_affine = R.stored_as(lps_pred, LPS_AFFINE, code)
            assert pred.shape == want_pred.shape and np.array_equal(pred, want_pred), name
            assert np.array_equal(affine.astype(np.float32), want_affine.astype(np.float32)), name
            assert np.array_equal(affine, _read(runs['files'][code, 'flair'])[1])       # the first input's original affine
            flips = f'FLAIR:{code}>LPS,T2:{code}>LPS,T1:{code}>LPS'
            assert VS.done_line(runs['log'][name]).endswith(f' | reorient={flips}') and f'shape={SHAPE}' in VS.done_line(runs['log'][name])
            entries = json.load(open(tmp / name / 'reorient_t1ce.json'))
            assert list(entries) == ['FLAIR', 'T2', 'T1'] and all(e['moved'] and e['shape_to'] == list(SHAPE) for e in entries.values())
    # the flag does something: the same RAS files without it give another prediction, and nothing of the feature shows
    plain, _ = _read(tmp / 'ras_plain' / 'predicted_t1ce.nii.gz')
    with_flag, _ = _read(tmp / 'ras_host' / 'predicted_t1ce.nii.gz')
    assert plain.shape == with_flag.shape and not np.array_equal(plain, with_flag)
    for name in ('ras_plain', 'lps_dev'):                 # (the lines name the output directory, which lies under this fixture's own)
        assert 'reorient' not in runs['log'][name].replace(str(tmp), 'TMP') and sorted(os.listdir(tmp / name)) == ['predicted_t1ce.nii.gz']


def test_evaluation_inputs_are_reoriented(runs):
    tmp = runs['tmp']
    want = json.load(open(tmp / 'lps_host' / 'metrics_t1ce.json'))
    assert set(want['regions']) >= {'tumor', 'healthy'}
    assert open(tmp / 'ras_host' / 'metrics_t1ce.json').read() == open(tmp / 'lps_host' / 'metrics_t1ce.json').read()      # (a null compares too)
    assert sorted(os.listdir(tmp / 'ras_host')) == ['metrics_t1ce.json', 'predicted_t1ce.nii.gz', 'reorient_t1ce.json']
