"""GPU: the anti-aliasing low-pass of --conform / --antialias (csrc/volume_lowpass.hip, mudiff_hip.volume_conform)
against the numpy restatement (tests/volume_conform_ref.py).

The kernel: every datatype, every set of filtered axes, shapes shorter than the filter, longer than one tile and with unit axes, to one
fp32 ulp (an fp64 fma against a separate multiply and add may move the last rounding and nothing else); its properties; non-finite
voxels; nothing written out of range; the C ABI's refusals.  Then volume_regrid.regrid_to(..., antialias=True) against the restatement
composed with the trilinear restatement, and the stripes of the host test on the device.  Then `predict_volume --conform
--conform_back` end to end on one analytic phantom written three ways, and the same through mudiff_hip.cohort."""
import ctypes as C

import numpy as np
import pytest
import torch

import volume_conform_ref as CR
import volume_intake_ref as I
import volume_regrid_ref as G
import volume_reorient_ref as R
import volume_support as VS

pytestmark = pytest.mark.gpu

SHAPES = [(37, 29, 23), (5, 4, 3), (300, 3, 2), (33, 1, 65), (1, 1, 1), (64, 64, 2)]
W1, W3, W11 = (CR.weights(CR.sigma(f)) for f in (1.25, 2.0, 8.0))          # R = 1, 3, 11
SIGMA_SETS = {'x': [W3, None, None], 'y': [None, W3, None], 'z': [None, None, W3], 'xyz': [W1, W3, W11], 'zyx': [W11, W1, W3],
              'none': [None, None, None]}
KINDS = {'u1': ('<u1', 0.0, 0.0), 'i2_scaled': ('<i2', 0.5, -3.0), 'u2': ('<u2', 0.0, 0.0), 'i4': ('<i4', 0.0, 0.0), 'f4': ('<f4', 0.0, 0.0)}
SIGNED = {'u1': np.uint8, 'i2': np.int16, 'u2': np.int16, 'i4': np.int32, 'f4': np.float32}      # torch has no wide unsigned dtypes
SENTINEL = 0xA5


def _volume(shape, dtype, seed):
    """[X,Y,Z] of `dtype`, F-ordered: noise over the whole range of the type on a smooth ramp, no two neighbours alike."""
    rng = np.random.default_rng(seed)
    if dtype == '<f4':
        v = rng.normal(100.0, 400.0, shape).astype(np.float32)
    else:
        info = np.iinfo(np.dtype(dtype))
        v = rng.integers(info.min, info.max, shape, dtype=np.int64, endpoint=True).astype(dtype)
    return np.asfortranarray(v)


def _device(vol):
    flat = np.ascontiguousarray(vol.reshape(-1, order='F'))
    return torch.from_numpy(flat.view(SIGNED[vol.dtype.kind + str(vol.dtype.itemsize)])).cuda()


def _host(dev, shape):
    return dev.cpu().numpy().reshape(-1).reshape(shape, order='F')


def _within_one_ulp(got, want):
    return bool((np.abs(got.astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.abs(want).astype(np.float32))).all())


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(str(v) for v in s))
def test_kernel_against_the_restatement(shape):
    from mudiff_hip import ops
    for k, (kind, (dtype, slope, inter)) in enumerate(KINDS.items()):
        vol = _volume(shape, dtype, 11 + k)
        values = I.values_float32(vol, slope, inter)
        dev = _device(vol)
        scaling = (slope, inter) if I.is_scaled(slope, inter) else (1.0, 0.0)
        for name, ws in SIGMA_SETS.items():
            out, bad = ops.volume_lowpass(dev, I.CODES[dtype[1:]], shape, *scaling, ws)
            if name == 'none':                           # nothing to filter: nothing launched, the caller keeps the stored voxels
                assert out is None and bad == 0
                continue
            want, _ = CR.lowpass(values, ws)
            got = _host(out, shape)
            assert out.dtype == torch.float32 and tuple(out.shape) == shape[::-1] and bad == 0
            assert _within_one_ulp(got, want), (kind, name, float(np.abs(got - want).max()))
            assert got.min() >= values.min() and got.max() <= values.max(), (kind, name)          # a weighted mean stays inside the range
            again, _ = ops.volume_lowpass(dev, I.CODES[dtype[1:]], shape, *scaling, ws)
            assert torch.equal(again, out), (kind, name)                                           # two runs: the same bits


def test_properties():
    from mudiff_hip import ops
    shape = (37, 29, 23)
    const = np.asfortranarray(np.full(shape, 1237, '<i2'))
    out, bad = ops.volume_lowpass(_device(const), 4, shape, 0.5, -3.0, [W1, W3, W11])
    want = np.float32(1237 * 0.5 - 3.0)
    assert bad == 0 and float(np.abs(_host(out, shape) - want).max()) <= float(np.spacing(want))  # a constant stays constant
    vol = _volume(shape, '<u2', 5)
    vol[8:30, 6:24, 4:20] = 0                            # a zero block wider than R = 3 on every axis
    out, _ = ops.volume_lowpass(_device(vol), 512, shape, 1.0, 0.0, [W3, W3, W3])
    got = _host(out, shape)
    assert np.array_equal(got[11:27, 9:21, 7:17], np.zeros((16, 12, 10), np.float32)) and float(got[10, 15, 10]) > 0
    assert got.min() >= 0 and got.max() <= float(vol.max())


def test_nonfinite_voxels_are_counted_and_read_as_zero():
    from mudiff_hip import ops
    shape = (70, 9, 40)                                  # more than one tile along x and z
    vol = _volume(shape, '<f4', 3)
    bad_at = [(0, 0, 0), (69, 8, 39), (31, 4, 31), (32, 4, 32), (33, 0, 0), (64, 8, 1), (5, 5, 33)]
    for n, at in enumerate(bad_at):
        vol[at] = (np.nan, np.inf, -np.inf)[n % 3]
    for ws in ([W3, None, None], [None, None, W3], [W1, W3, W11]):
        out, bad = ops.volume_lowpass(_device(vol), 16, shape, 1.0, 0.0, ws)
        want, want_bad = CR.lowpass(vol, ws)
        got = _host(out, shape)
        assert bad == want_bad == len(bad_at) and np.isfinite(got).all() and _within_one_ulp(got, want)


def _call(vol, code, shape, scaling, ws, out, scratch, count):
    from mudiff_hip import load, stream_ptr
    args = []
    keep = []
    for w in ws:
        if w is None:
            args += [None, 0]
        elif isinstance(w, tuple):                       # (weights, a radius of the test's choosing)
            keep.append(np.ascontiguousarray(w[0], np.float64))
            args += [keep[-1].ctypes.data_as(C.POINTER(C.c_double)), w[1]]
        else:
            keep.append(np.ascontiguousarray(w, np.float64))
            args += [keep[-1].ctypes.data_as(C.POINTER(C.c_double)), len(w) // 2]
    return load().mud_volume_lowpass(C.c_void_p(vol), code, *shape, *scaling, *args, C.c_void_p(out), C.c_void_p(scratch), C.c_void_p(count),
                                     stream_ptr())


@pytest.mark.parametrize('shape', [(37, 29, 23), (300, 3, 2)], ids=['37x29x23', '300x3x2'])
def test_nothing_is_written_out_of_range(shape):
    """Output and scratch sit inside larger buffers full of a sentinel; the bands on both sides are intact afterwards."""
    n, band = int(np.prod(shape)), 4096
    for dtype in ('<u1', '<i2', '<f4'):
        vol = _volume(shape, dtype, 9)
        width = vol.dtype.itemsize
        src = torch.full((band + n * width + band,), SENTINEL, dtype=torch.uint8, device='cuda')
        src[band:band + n * width] = torch.from_numpy(np.ascontiguousarray(vol.reshape(-1, order='F')).view(np.uint8)).cuda()
        src_before = src.clone()
        for ws in ([W3, None, None], [None, W11, None], [None, None, W3], [W1, W3, W11], [W11, W11, None]):
            out = torch.full((band + 4 * n + band,), SENTINEL, dtype=torch.uint8, device='cuda')
            scratch = torch.full((band + 4 * n + band,), SENTINEL, dtype=torch.uint8, device='cuda')
            count = torch.full((3,), -1, dtype=torch.int32, device='cuda')
            assert _call(src.data_ptr() + band, I.CODES[dtype[1:]], shape, (1.0, 0.0), ws, out.data_ptr() + band, scratch.data_ptr() + band,
                         count.data_ptr() + 4) == 0
            for buf in (out, scratch):
                assert bool((buf[:band] == SENTINEL).all()) and bool((buf[band + 4 * n:] == SENTINEL).all()), (dtype, len(ws))
            assert count.tolist() == [-1, 0, -1]
            got = out[band:band + 4 * n].cpu().numpy().view(np.float32).reshape(shape, order='F')
            assert _within_one_ulp(got, CR.lowpass(I.values_float32(vol), ws)[0])
            if sum(w is not None for w in ws) == 1:      # one pass: the scratch volume is not touched at all
                assert bool((scratch == SENTINEL).all())
        assert torch.equal(src, src_before)


def test_cabi_refusals():
    from mudiff_hip import MudiffHipError, load, ops
    shape, n = (6, 5, 4), 120
    src = torch.arange(n, dtype=torch.float32, device='cuda').view(torch.uint8)          # finite as fp32: the counter ends at 0
    out = torch.full((n * 4 + 64,), SENTINEL, dtype=torch.uint8, device='cuda')
    scratch = torch.full((n * 4 + 64,), SENTINEL, dtype=torch.uint8, device='cuda')
    count = torch.full((2,), -1, dtype=torch.int32, device='cuda')
    s, o, t, c = src.data_ptr(), out.data_ptr(), scratch.data_ptr(), count.data_ptr()
    one, two = [W3, None, None], [W3, W1, None]
    w17 = np.ones(35)
    nan, neg, zero = W3.copy(), W3.copy(), W3.copy()
    nan[1], neg[5], zero[3] = np.nan, -1e-3, 0.0
    inf = W3.copy()
    inf[0] = np.inf
    refused = [
        (s, 16, shape, [(w17, 17), None, None], o, t, c), (s, 16, shape, [None, (W3, -1), None], o, t, c),            # the radius
        (s, 16, shape, [nan, None, None], o, t, c), (s, 16, shape, [None, None, inf], o, t, c), (s, 16, shape, [None, neg, None], o, t, c),
        (s, 16, shape, [None, zero, None], o, t, c),                                                                 # the weights
        (s, 64, shape, one, o, t, c), (s, 0, shape, one, o, t, c), (s, 256, shape, one, o, t, c),                    # the datatype
        (s, 16, (0, 5, 4), one, o, t, c), (s, 16, (6, -5, 4), one, o, t, c), (s, 2, (2048, 2048, 512), one, o, t, c),      # the size
        (0, 16, shape, one, o, t, c), (s, 16, shape, one, 0, t, c), (s, 16, shape, one, o, t, 0), (s, 16, shape, two, o, 0, c),      # null
        (s + 4, 16, shape, one, o, t, c), (s, 16, shape, one, o + 4, t, c), (s, 16, shape, two, o, t + 8, c), (s, 16, shape, one, o, t, c + 2),
        (s, 16, shape, one, s, t, c), (s, 16, shape, one, s + 16, t, c), (s, 16, shape, two, o, o, c), (s, 16, shape, two, o, o + 16, c),
        (s, 16, shape, two, o, s, c),                                                                                # overlaps
    ]
    for args in refused:
        src_before = src.clone()
        assert _call(args[0], args[1], args[2], (1.0, 0.0), *args[3:]) != 0, args
        assert load().mud_last_error().decode().startswith('mud_volume_lowpass: '), args
        torch.cuda.synchronize()
        assert bool((out == SENTINEL).all()) and bool((scratch == SENTINEL).all()) and count.tolist() == [-1, -1] and torch.equal(src, src_before), args
    assert _call(s, 16, shape, (1.0, 0.0), [None, None, None], o, t, c) == 0                        # nothing to filter: nothing launched
    assert _call(s, 16, shape, (1.0, 0.0), one, o, 0, c) == 0                                       # one pass needs no scratch volume
    torch.cuda.synchronize()
    assert bool((scratch == SENTINEL).all()) and count.tolist() == [0, -1] and not bool((out[:n * 4] == SENTINEL).all())
    flat = torch.zeros(n, dtype=torch.float32, device='cuda')
    for bad in (lambda: ops.volume_lowpass(flat, 4, shape, 1.0, 0.0, one), lambda: ops.volume_lowpass(flat, 16, (6, 5, 5), 1.0, 0.0, one),
                lambda: ops.volume_lowpass(flat.cpu(), 16, shape, 1.0, 0.0, one), lambda: ops.volume_lowpass(flat, 3, shape, 1.0, 0.0, one)):
        with pytest.raises(MudiffHipError):
            bad()
    with pytest.raises(ValueError):
        ops.volume_lowpass(flat, 16, shape, 1.0, 0.0, [W3[:-1], None, None])


# ---------------------------------------------------------------------------------------------------
# volume_regrid.regrid_to(..., antialias=True)
# ---------------------------------------------------------------------------------------------------
SRC_SHAPE, REF_SHAPE = (48, 40, 12), (24, 20, 24)
REGRID_BAR = 4 * 1.052e-4                                 # see test_regrid_to_antialiased


def regrid_case(tilt=12.0, spacing=(0.5, 0.5, 2.0)):
    """(48, 40, 12) int16 at (0.5, 0.5, 2) mm, tilted 12 degrees about its own centre, and a (24, 20, 24) 1 mm axis-aligned grid about
    the same centre -> (the stored volume, its affine, the reference shape, the reference affine)."""
    rng = np.random.default_rng(17)
    x, y, z = np.meshgrid(*[np.arange(s, dtype=np.float64) for s in SRC_SHAPE], indexing='ij')
    vol = 900 * np.exp(-(((x - 22) / 14) ** 2 + ((y - 21) / 11) ** 2 + ((z - 5.5) / 4) ** 2)) + rng.normal(0, 60, SRC_SHAPE) + 200
    vol = np.asfortranarray(np.clip(np.rint(vol), 0, 4000).astype('<i2'))
    src = R.affine_of('RAS', SRC_SHAPE, spacing=spacing)
    src[:3, 3] = -src[:3, :3] @ ((np.asarray(SRC_SHAPE) - 1) / 2)          # the grid centre at the world origin
    src = R.rotation(0, tilt) @ src
    ref = R.affine_of('RAS', REF_SHAPE)
    ref[:3, 3] = -ref[:3, :3] @ ((np.asarray(REF_SHAPE) - 1) / 2)
    return vol, src, REF_SHAPE, ref


def test_regrid_to_antialiased():
    """The bar is the restatement's own: on this case the chain with fp32 between the passes (what the kernels do) and the chain with
    fp64 throughout differ by 1.052e-4 at most (measured on the CPU, at values up to 1071: the fp32 roundings, 6.1e-5 each at that size, of
    the two passes and of the result); the device may be 4 times that, 4.208e-4, from the fp32 restatement."""
    from mudiff_hip import volume_regrid as VR
    vol, src, ref_shape, ref = regrid_case()
    device = torch.device('cuda:0')
    M = G.matrix(src, ref)
    f = CR.factors(M)
    assert list(f) == pytest.approx([2.0, 2.0, 0.5])                  # x, y downsampled and filtered; z not
    want = CR.antialiased_trilinear(vol.astype(np.float32), M, ref_shape)
    want64 = CR.antialiased_trilinear(vol.astype(np.float32), M, ref_shape, keep=np.float64)
    own = float(np.abs(want - want64).max())
    print(f'restatement fp32 vs fp64 intermediates: {own:.3e}')
    assert own <= REGRID_BAR / 4
    found = {}
    out = VR.regrid_to(VS.raw_volume(vol, affine=src), ref_shape, ref, device, antialias=True, found=found, name='case')
    got = out.values_float32()
    err = float(np.abs(got - want).max())
    print(f'device vs restatement: {err:.3e}')
    assert err <= REGRID_BAR
    assert found['lowpass'] is True and found['nonfinite'] == 0 and found['antialias']['radii'] == [3, 3, 0]
    plain = VR.regrid_to(VS.raw_volume(vol, affine=src), ref_shape, ref, device)
    assert float(np.abs(plain.values_float32() - got).max()) > 10                                  # the filter does something here
    off = VR.regrid_to(VS.raw_volume(vol, affine=src), ref_shape, ref, device, antialias=False)
    assert torch.equal(off.dev, plain.dev)
    # a pure 12 degree rotation at equal spacing: nothing is filtered, the result is today's bit for bit (linear and cubic)
    vol, src, ref_shape, ref = regrid_case(spacing=(1.0, 1.0, 1.0))
    for mode in ('linear', 'cubic'):
        found = {}
        a = VR.regrid_to(VS.raw_volume(vol, affine=src), ref_shape, ref, device, mode=mode, antialias=True, found=found)
        b = VR.regrid_to(VS.raw_volume(vol, affine=src), ref_shape, ref, device, mode=mode)
        assert torch.equal(a.dev, b.dev) and found['lowpass'] is False and found['antialias']['radii'] == [0, 0, 0]
    # a label volume is never filtered
    a = VR.regrid_to(VS.raw_volume(vol, affine=src * np.array([2.0, 2.0, 2.0, 1.0])), ref_shape, ref, device, mode='nearest', antialias=True)
    b = VR.regrid_to(VS.raw_volume(vol, affine=src * np.array([2.0, 2.0, 2.0, 1.0])), ref_shape, ref, device, mode='nearest')
    assert torch.equal(a.dev, b.dev)


def test_stripes_on_the_device():
    """The host test's stripes: period-2 stripes 0 / 200 at 0.5 mm sampled onto a 1 mm grid give exactly 0 without the filter and stay
    within 13.86 of the mean 100 with it."""
    from mudiff_hip import volume_regrid as VR
    shape = (64, 6, 5)
    vol = np.asfortranarray(CR.stripes(shape).astype('<i2'))
    src, ref, ref_shape = np.diag([0.5, 1.0, 1.0, 1.0]), np.eye(4), (32, 6, 5)
    device = torch.device('cuda:0')
    plain = VR.regrid_to(VS.raw_volume(vol, affine=src), ref_shape, ref, device).values_float32()
    assert np.array_equal(plain, np.zeros(ref_shape, np.float32))
    got = VR.regrid_to(VS.raw_volume(vol, affine=src), ref_shape, ref, device, antialias=True).values_float32()
    assert float(np.abs(got[2:-2] - 100.0).max()) <= 13.86 and float(got[2:-2].min()) > 86.0
    want = G.trilinear(CR.lowpass(vol.astype(np.float32), [W3, None, None])[0], G.matrix(src, ref), ref_shape)
    assert _within_one_ulp(got, want)


# ---------------------------------------------------------------------------------------------------
# end to end: one analytic field, a sum of Gaussian blobs in world millimetres, written three ways
# ---------------------------------------------------------------------------------------------------
GRID_SHAPE, GRID_MM = (24, 24, 16), 2.0
A_AFFINE = R.affine_of('LPS', GRID_SHAPE, (GRID_MM,) * 3, origin=(23.0, 25.0, -15.0))          # (A) the conform grid itself: centre (0, 2, 0) mm
CENTRE = np.array([0.0, 2.0, 0.0])
B_SHAPE, C_SHAPE = (60, 60, 44), (48, 48, 32)
FIELDS = {'flair': ([(-8.0, 6.0, -3.0), (9.0, -3.0, 4.0), (2.0, 12.0, -6.0)], [7.0, 6.0, 8.0], [1000.0, 800.0, 600.0]),
          't2': ([(-6.0, -4.0, 2.0), (7.0, 8.0, -4.0), (0.0, 2.0, 6.0)], [8.0, 6.0, 7.0], [900.0, 1100.0, 500.0]),
          't1': ([(5.0, 5.0, 0.0), (-9.0, 0.0, -5.0), (-1.0, -6.0, 5.0)], [6.0, 7.0, 9.0], [1200.0, 700.0, 650.0]),
          'gt': ([(0.0, 2.0, 0.0), (8.0, 8.0, 3.0), (-7.0, -3.0, -4.0)], [9.0, 6.0, 7.0], [1000.0, 900.0, 700.0])}
SLAB = (5, 11)                                           # --slice_half_range 3 of 16 planes


def _centred(code, shape, spacing, tilt=0.0, shift=(0.0, 0.0, 0.0)):
    a = R.affine_of(code, shape, (spacing,) * 3)
    a[:3, 3] = -a[:3, :3] @ ((np.asarray(shape) - 1) / 2)
    a = R.rotation(0, tilt) @ a
    a[:3, 3] += CENTRE + np.asarray(shift)
    return a.astype(np.float32).astype(np.float64)       # what a header stores


B_AFFINE = _centred('RAS', B_SHAPE, 1.0, tilt=12.0)      # (B) 1 mm, RAS, 12 degrees oblique, a larger field of view
C_AFFINE = _centred('LPS', C_SHAPE, 1.25, shift=(0.3, -0.4, 0.2))      # (C) the later inputs of B on a third grid


def phantom(which, shape, affine):
    return np.asfortranarray(np.rint(CR.blobs(affine, shape, *FIELDS[which])).astype('<i2'))


def geometry(name, which):
    """(shape, affine) of input `which` in the way `name` of writing the phantom."""
    if name == 'A':
        return GRID_SHAPE, A_AFFINE
    if name == 'C' and which in ('t2', 't1'):
        return C_SHAPE, C_AFFINE
    return B_SHAPE, B_AFFINE


def restated_stacks(name):
    """The condition stacks of the way `name` by the restatement alone (CPU): the stored values through the low-pass and the trilinear
    restatement onto the conform grid of the first input, then the pipeline's own host normalisation and slab."""
    from mudiff_hip import volume as V
    first_shape, first_affine = geometry(name, 'flair')
    shape, grid = CR.conform_grid(first_shape, first_affine, GRID_SHAPE, (GRID_MM,) * 3, 'LPS')
    stacks, spans = [], []
    for which in ('flair', 't2', 't1'):
        src_shape, src_affine = geometry(name, which)
        vol = phantom(which, src_shape, src_affine).astype(np.float32)
        if name != 'A':
            vol = CR.antialiased_trilinear(vol, G.matrix(src_affine, grid), shape)
        sel = vol[vol != 0]
        spans.append(float(np.percentile(sel, 99.0) - np.percentile(sel, 1.0)))
        stacks.append(np.stack(V.extract_center_slices(V.normalise_volume(vol), 3)[0], 0))
    return stacks, spans


def _write(path, vol, affine, spacing):
    """I.write_nifti_typed, uncompressed, with pixdim[1..3] set to the spacing (a header that agrees with its affine)."""
    import struct
    I.write_nifti_typed(path, vol, affine=affine)
    with open(path, 'r+b') as f:
        f.seek(80)
        f.write(struct.pack('<3f', spacing, spacing, spacing))
    return str(path)


CONFORM = ['--conform', '--conform_shape', '24', '24', '16', '--conform_spacing', '2']
NESTED = ['--reorient', '--reorient_back'] + CONFORM + ['--conform_back']      # both writers, --reorient_back inside --conform_back


@pytest.fixture(scope='module')
def runs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp('conform')
    VS.write_tiny_model(tmp)
    files = {}
    for name in 'ABC':
        for which in FIELDS:
            shape, affine = geometry(name, which)
            files[name, which] = _write(tmp / f'{name}_{which}.nii', phantom(which, shape, affine), affine, float(np.linalg.norm(affine[:3, 0])))
    model = VS.model_argv(tmp, 3, 7, '--resize_back')
    inputs = lambda n: ['--input_flair', files[n, 'flair'], '--input_t2', files[n, 't2'], '--input_t1', files[n, 't1']]      # noqa: E731
    back = CONFORM + ['--conform_back']
    jobs = {'a_plain': inputs('A'), 'a_conform': inputs('A') + CONFORM, 'b_host': inputs('B') + back + ['--gt_volume', files['B', 'gt']],
            'c_host': inputs('C') + back, 'b_plain': inputs('B'), 'b_dev': inputs('B') + back + ['--device_intake'],
            'c_dev': inputs('C') + back + ['--device_intake'],
            'b_nested': inputs('B') + NESTED + ['--gt_volume', files['B', 'gt']],
            'b_nested_dev': inputs('B') + NESTED + ['--gt_volume', files['B', 'gt'], '--device_intake']}
    jobs = {k: model + a + ['--output_dir', str(tmp / k)] for k, a in jobs.items()}
    manifest = tmp / 'cohort.tsv'
    manifest.write_text('id\tt1\tt1ce\tt2\tflair\n' + ''.join(f's_{n.lower()}\t' + '\t'.join([files[n, 't1'], '', files[n, 't2'], files[n, 'flair']]) + '\n'
                                                              for n in 'BC'))
    scored = tmp / 'cohort_nested.tsv'
    scored.write_text('id\tt1\tt1ce\tt2\tflair\tgt\n' + 's_b\t' + '\t'.join([files['B', 't1'], '', files['B', 't2'], files['B', 'flair'], files['B', 'gt']]) + '\n')
    cohorts = {'cohort': model + back + ['--manifest', str(manifest), '--output_dir', str(tmp / 'cohort')],
               'cohort_nested': model + NESTED + ['--score', '--manifest', str(scored), '--output_dir', str(tmp / 'cohort_nested')]}
    steps = [VS.volume_step(k, argv, stacks=True) for k, argv in jobs.items()] + [VS.cohort_step(k, argv) for k, argv in cohorts.items()]
    log = VS.run_plan(tmp, steps, 600, ignore='all')
    return dict(tmp=tmp, log=log, stacks={k: VS.load_stacks(tmp, k) for k in jobs}, files=files)


def test_conform_end_to_end(runs):
    """The distances of B's and C's condition stacks from A's, by the restatement alone on the CPU (stack units, [-1, 1]; FLAIR / T2 /
    T1): B 0.0267 / 0.0206 / 0.0171, C 0.0267 / 0.0199 / 0.0203; the device may be 1.5 times as far.  The bar against the restatement
    itself is the one of test_regrid_to_antialiased carried through the normalisation: a deviation d of the resampled values (of the same
    size here, up to ~1100) moves a normalised value 2 (v - lo) / (hi - lo) - 1 by 2 d / (hi - lo) directly and, through lo and hi
    (interpolated order statistics of such values: at most d each), by at most 4 d / (hi - lo) more: 6 REGRID_BAR / (hi - lo)."""
    import json
    import os
    from mudiff_hip import volume as V
    tmp = runs['tmp']
    # A: on the conform grid already - no input is resampled and the file is the plain run's, header included
    assert VS.payload(str(tmp / 'a_conform' / 'predicted_t1ce.nii.gz')) == VS.payload(str(tmp / 'a_plain' / 'predicted_t1ce.nii.gz'))
    assert all(np.array_equal(g, w) for g, w in zip(runs['stacks']['a_conform'], runs['stacks']['a_plain']))
    assert VS.done_line(runs['log']['a_conform']).endswith(' | conform=24x24x16@2mm:') and 'conform' not in VS.done_line(runs['log']['a_plain']).replace(str(tmp), 'TMP')
    entries = json.load(open(tmp / 'a_conform' / 'conform_t1ce.json'))
    assert entries['grid'] == '24x24x16@2mm' and all(not e['resampled'] and e['radii'] == [0, 0, 0] for e in entries['inputs'].values())
    assert sorted(os.listdir(tmp / 'a_plain')) == ['predicted_t1ce.nii.gz']
    want_a, _ = restated_stacks('A')
    for g, w in zip(runs['stacks']['a_plain'], want_a):
        assert np.array_equal(g, w)
    # B and C: the restatement's stacks within the bar, and no further from A than 1.5 times the restatement's own distance
    for name, run in (('B', 'b_host'), ('C', 'c_host')):
        want, spans = restated_stacks(name)
        got = runs['stacks'][run]
        for k, (g, w, a, span) in enumerate(zip(got, want, want_a, spans)):
            assert g.shape == w.shape == (7, 24, 24)
            err, own, far = float(np.abs(g - w).max()), float(np.abs(w - a).max()), float(np.abs(g - runs['stacks']['a_plain'][k]).max())
            print(f'{name} input {k}: device vs restatement {err:.3e} (bar {6 * REGRID_BAR / span:.3e}); from A: restatement {own:.4f}, device {far:.4f}')
            assert err <= 6 * REGRID_BAR / span, (name, k, err)
            assert 0.01 < own < 0.03 and far <= 1.5 * own, (name, k, own, far)
        # --conform_back: the first input's own shape, affine and header
        buf, hdr, code = V.open_nifti1(str(tmp / run / 'predicted_t1ce.nii.gz'))
        _, first, _ = V.open_nifti1(runs['files'][name, 'flair'])
        assert code == 16 and hdr.shape == B_SHAPE and np.array_equal(hdr.world_affine, first.world_affine) and np.array_equal(hdr.world_affine, B_AFFINE)
        assert hdr._get('8f', 76) == first._get('8f', 76) and hdr.raw[252:256] == first.raw[252:256]
        pred = V.read_nifti(str(tmp / run / 'predicted_t1ce.nii.gz'))[0]
        assert float(pred.max()) > 0.05 and float(pred.min()) >= -1e-3 and np.isfinite(pred).all()
        rep = json.load(open(tmp / run / 'conform_t1ce.json'))
        assert rep['grid'] == '24x24x16@2mm' and list(rep['inputs']) == ['FLAIR', 'T2', 'T1']
        for which, e in rep['inputs'].items():
            assert set(e) == {'shape_from', 'spacing_from', 'obliquity_deg', 'factors', 'sigmas', 'radii', 'resampled', 'nonfinite'}
            third = name == 'C' and which != 'FLAIR'
            assert e['resampled'] is True and e['nonfinite'] == 0 and e['shape_from'] == list(C_SHAPE if third else B_SHAPE)
            assert e['radii'] == ([2, 2, 2] if third else [3, 3, 3]) and e['factors'] == pytest.approx([1.6] * 3 if third else [2.0] * 3, abs=1e-6)
            assert e['obliquity_deg'] == pytest.approx(0.0 if third else 12.0, abs=1e-4) and e['spacing_from'] == pytest.approx([1.25 if third else 1.0] * 3, abs=1e-6)
    assert VS.done_line(runs['log']['c_host']).endswith(' | conform=24x24x16@2mm:FLAIR,T2,T1 | antialias=on')
    assert VS.done_line(runs['log']['b_host']).endswith(' | regrid=gt_volume | conform=24x24x16@2mm:FLAIR,T2,T1 | antialias=on')      # the ground truth too
    assert 'shape=(24, 24, 16)' in VS.done_line(runs['log']['b_host']) and 'slices=5..11' in VS.done_line(runs['log']['b_host'])
    assert sorted(os.listdir(tmp / 'b_host')) == ['conform_t1ce.json', 'metrics_t1ce.json', 'predicted_t1ce.nii.gz']
    # B without the flag: nothing fails (--resize_back), but the generators see other stacks
    plain = runs['stacks']['b_plain']
    assert plain[0].shape == (7, 60, 60) and 'conform' not in VS.done_line(runs['log']['b_plain']).replace(str(tmp), 'TMP')


def test_cohort_writes_the_single_runs_files(runs):
    tmp = runs['tmp']
    lines = VS.done_lines(runs['log']['cohort'], 2)
    for n, line in zip('bc', lines):
        assert VS.payload(str(tmp / 'cohort' / f's_{n}' / 'predicted_t1ce.nii.gz')) == VS.payload(str(tmp / f'{n}_dev' / 'predicted_t1ce.nii.gz'))
        assert open(tmp / 'cohort' / f's_{n}' / 'conform_t1ce.json').read() == open(tmp / f'{n}_dev' / 'conform_t1ce.json').read()
        assert line.endswith(' | conform=24x24x16@2mm:FLAIR,T2,T1 | antialias=on')


def test_nested_writers_and_evaluation_grid_through_both_entry_points(runs):
    """Subject B (stored RAS, 12 degrees oblique) under --reorient --reorient_back --conform --conform_back with a ground truth: the
    evaluation inputs go reoriented onto the conform grid of the reoriented first input, the prediction is scored there and both writers
    take it back to the first input's own storage grid.  predict_volume (host and device intake) and the cohort with --score write the
    same bytes, the same metrics and the same [done] tail.  24 x 24 x 16 with a slab of 7 planes is the smallest grid the 7 x 7 x 7 SSIM
    window accepts."""
    import json
    from mudiff_hip import volume as V
    tmp = runs['tmp']
    single, cohort = tmp / 'b_nested', tmp / 'cohort_nested' / 's_b'
    tail = lambda line: line.split(' | ', 1)[1]                       # noqa: E731  (what follows the path, which differs)
    want = VS.done_line(runs['log']['b_nested'])
    assert tail(want) == ('shape=(24, 24, 16) | slices=5..11 | regrid=gt_volume | reorient=FLAIR:RAS>LPS,T2:RAS>LPS,T1:RAS>LPS | '
                          'conform=24x24x16@2mm:FLAIR,T2,T1 | antialias=on')
    for other, line in ((tmp / 'b_nested_dev', VS.done_line(runs['log']['b_nested_dev'])), (cohort, VS.done_line(runs['log']['cohort_nested']))):
        assert VS.payload(str(other / 'predicted_t1ce.nii.gz')) == VS.payload(str(single / 'predicted_t1ce.nii.gz'))
        for report in ('metrics_t1ce.json', 'reorient_t1ce.json', 'conform_t1ce.json'):
            assert open(other / report).read() == open(single / report).read(), report
        assert tail(line) == tail(want)
    assert sorted(p.name for p in cohort.iterdir()) == sorted(p.name for p in single.iterdir()) == [
        'conform_t1ce.json', 'metrics_t1ce.json', 'predicted_t1ce.nii.gz', 'reorient_t1ce.json']
    # the written file: the first input's own shape, affine and header
    _, hdr, code = V.open_nifti1(str(single / 'predicted_t1ce.nii.gz'))
    _, first, _ = V.open_nifti1(runs['files']['B', 'flair'])
    assert code == 16 and hdr.shape == B_SHAPE and np.array_equal(hdr.world_affine, first.world_affine) and np.array_equal(hdr.world_affine, B_AFFINE)
    assert hdr._get('8f', 76) == first._get('8f', 76) and hdr.raw[252:256] == first.raw[252:256]
    pred = V.read_nifti(str(single / 'predicted_t1ce.nii.gz'))[0]
    assert float(pred.max()) > 0.05 and np.isfinite(pred).all()
    metrics = json.load(open(single / 'metrics_t1ce.json'))
    assert metrics['regions'] == ['slab', 'brain'] and metrics['metrics']['slab']['voxels'] == 24 * 24 * 7
    row = json.load(open(tmp / 'cohort_nested' / 'cohort_t1ce.json'))['subjects'][0]
    assert row['id'] == 's_b' and row['metrics']['slab']['psnr'] == metrics['metrics']['slab']['psnr']
