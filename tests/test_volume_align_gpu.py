"""GPU: --align.  mud_volume_mirror_moments against the fp64 numpy restatement (tests/volume_align_ref.py): equal
sums where the mirror maps the sample lattice onto voxels, within what the samples on a bin edge can cause for oblique planes; the
kernel's edge cases (K = 1, K across the candidate chunk, a few hundred candidates, strides, bins, every stored datatype, NaN and Inf
voxels, a mirror that leaves the volume, two runs, independence of the other candidates, the C ABI's refusals); the device search
against the same search over the numpy cost; prepare_inputs under --conform --align (one interpolation, onto the turned grid); and
`predict_volume --conform --align` end to end through the host path, --device_intake, --conform_back and --gt_volume."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import volume_align_ref as AR
import volume_coreg_ref as K
import volume_intake_ref as R
import volume_support as VS

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SHAPE = (47, 23, 17)                                     # primes: no stride divides them; 9 workgroups of 2048 sample points at stride 1


def _device_sums(vol, mats, stride, lo, scale, bins, scaling=(1.0, 0.0)):
    """vol: the stored [X,Y,Z] array -> host int64 [K, 6]."""
    from mudiff_hip import volume_align as VA
    from mudiff_hip import volume_intake as VI
    raw = VS.raw_volume(vol, scaling)
    out = VA.mirror_moments(VI.upload(raw, DEV), (raw.code, vol.shape) + raw.scaling, mats, stride, lo, scale, bins)
    assert out.dtype == np.int64 and out.shape == (len(np.asarray(mats).reshape(-1, 12)), 6)
    return out


def _flip(axis, offset, shape=SHAPE):
    """The mirror through an axis-aligned plane: index i along `axis` -> offset - i, exact in fp64."""
    m = np.eye(4)[:3]
    m[axis, axis], m[axis, 3] = -1.0, float(offset)
    return m


def _oblique(shape=SHAPE, poses=((7.0, -5.0, 1.5), (-3.0, 4.0, -0.7), (12.0, 9.0, 0.0))):
    from mudiff_hip import volume_align as VA
    from mudiff_hip.volume_coreg import grid_centre
    A = AR.affine(shape, (1.1, 0.9, 1.3))
    return VA.mirror_matrices(poses, A, grid_centre(shape, A))


@pytest.fixture(scope='module')
def noise():
    return R.synthetic(SHAPE, 'noise', 'f4', seed=71)


# ---------------------------------------------------------------------------------------------------
# sums against the reference
# ---------------------------------------------------------------------------------------------------
def test_exact_lattice_mirrors_match_the_reference_bit_for_bit(noise):
    """A flip plus an integer shift: the plane through the centre, half a voxel off it, whole voxels off it - along every axis; and the
    same matrices as volume_align.mirror_matrices builds them for a unit affine."""
    from mudiff_hip import volume_align as VA
    from mudiff_hip.volume_coreg import grid_centre
    mats = [_flip(0, SHAPE[0] - 1), _flip(0, SHAPE[0]), _flip(0, SHAPE[0] - 2), _flip(0, SHAPE[0] + 3), _flip(0, SHAPE[0] - 7), _flip(1, SHAPE[1] - 1),
            _flip(1, SHAPE[1] + 2), _flip(2, SHAPE[2] - 1), _flip(2, SHAPE[2] - 4)]
    built = VA.mirror_matrices([(0.0, 0.0, 0.0), (0.0, 0.0, 0.5), (0.0, 0.0, -0.5), (0.0, 0.0, 2.0), (0.0, 0.0, -3.0)], np.eye(4), grid_centre(SHAPE, np.eye(4)))
    assert np.array_equal(built, np.stack(mats[:5]))
    for stride in (1, 2, 3):
        for bins in (2, 32, 256):
            lo, scale = AR.bin_range(noise, bins)
            want = AR.moments_of(noise, mats, stride, lo, scale, bins)
            got = _device_sums(noise, mats, stride, lo, scale, bins)
            assert np.array_equal(got, want) and (want[:, 0] > 0).all(), (stride, bins, got, want)
            if bins > 2:
                assert (want[:, 5] > 0).all() and len({tuple(r) for r in want.tolist()}) == len(mats)


def test_oblique_planes_match_the_reference_up_to_the_bin_edges(noise):
    """n, sum a and sum a^2 equal; with ne = the samples within rounding of a bin edge (volume_coreg_ref.n_edge), |d sum b| <= ne,
    |d sum b^2| <= ne (2 bins - 1), |d sum a b| <= ne (bins - 1): one bin up or down per such sample."""
    mats = _oblique()
    for stride in (1, 2, 3):
        for bins in (2, 32, 256):
            lo, scale = AR.bin_range(noise, bins)
            got = _device_sums(noise, mats, stride, lo, scale, bins)
            for k, M in enumerate(mats):
                want, info = AR.moments(noise, M, stride, lo, scale, bins, details=True)
                ne = K.n_edge(info, (lo, scale, lo, scale), bins, float(np.abs(noise).max()), SHAPE)
                d = np.abs(got[k] - want)
                print('stride', stride, 'bins', bins, 'plane', k, 'n', want[0], 'of', info['points'], 'n_edge', ne, '|dev - ref|', d.tolist())
                assert want[0] > 0 and ne <= 1e-3 * want[0]
                assert d[0] == 0 and d[1] == 0 and d[3] == 0
                assert d[2] <= ne and d[4] <= ne * (2 * bins - 1) and d[5] <= ne * (bins - 1)


# ---------------------------------------------------------------------------------------------------
# the kernel's edge cases
# ---------------------------------------------------------------------------------------------------
def _many_exact(count):
    """`count` exact mirrors: flips along x, y, z through planes up to 50 voxels off either way (many leave the volume entirely)."""
    return [_flip(k % 3, SHAPE[k % 3] - 1 + (k // 3 - count // 6)) for k in range(count)]


@pytest.mark.parametrize('count', [1, 17, 301, 2003])
def test_any_number_of_candidates(noise, count):
    """The entry point gives a workgroup ceil(9 tiles x K / 1024) candidates, 16 at most: 1 for K = 1 and 17, 3 for K = 301 (the last
    workgroup has one), 16 for K = 2003 (the last has three)."""
    mats = _many_exact(count)
    lo, scale = AR.bin_range(noise, 32)
    want = AR.moments_of(noise, mats, 1, lo, scale, 32)
    got = _device_sums(noise, mats, 1, lo, scale, 32)
    assert np.array_equal(got, want) and want[:, 0].max() > 0
    if count > 300:
        assert (want[:, 0] == 0).sum() > 50 and (want[:, 0] > 0).sum() > 50


def test_a_candidate_does_not_depend_on_the_others_in_the_launch(noise):
    from mudiff_hip import volume_align as VA
    from mudiff_hip.volume_coreg import grid_centre
    A = AR.affine(SHAPE, (1.1, 0.9, 1.3))
    poses = [(y, r, t) for y in (-9.0, -3.0, 0.0, 4.5, 11.0) for r in (-6.0, -1.0, 2.0, 7.5, 10.0) for t in (-2.0, -0.4, 0.3, 1.1, 2.5)] + [(1.0, 1.0, 1.0)]
    mats = VA.mirror_matrices(poses, A, grid_centre(SHAPE, A))
    assert len(mats) == 126                               # two candidates per workgroup; the single runs and the slice below: one
    lo, scale = AR.bin_range(noise, 32)
    together = _device_sums(noise, mats, 1, lo, scale, 32)
    assert np.array_equal(_device_sums(noise, mats[::-1], 1, lo, scale, 32), together[::-1])
    for k in (0, 15, 16, 125):
        assert np.array_equal(_device_sums(noise, mats[k:k + 1], 1, lo, scale, 32)[0], together[k])
    assert np.array_equal(_device_sums(noise, mats[5:22], 1, lo, scale, 32), together[5:22])
    assert np.array_equal(_device_sums(noise, mats, 1, lo, scale, 32), together)      # and two runs are the same bits


@pytest.mark.parametrize('dtype,scaling', [('u1', (1.0, 0.0)), ('i2', (1.0, 0.0)), ('u2', (1.0, 0.0)), ('i4', (1.0, 0.0)), ('f4', (1.0, 0.0)),
                                           ('i2', (0.0123, -5.5))])
def test_every_stored_datatype(dtype, scaling):
    vol = R.synthetic(SHAPE, 'noise', dtype, seed=72)
    values = np.asfortranarray(R.values_float32(vol, *scaling))
    mats = [_flip(0, SHAPE[0] - 1), _flip(0, SHAPE[0] + 4), _flip(1, SHAPE[1] - 2), _flip(2, SHAPE[2] - 1)]
    lo, scale = AR.bin_range(values, 32)
    want = AR.moments_of(values, mats, 2, lo, scale, 32)
    assert np.array_equal(_device_sums(vol, mats, 2, lo, scale, 32, scaling), want) and (want[:, 0] > 0).all() and (want[:, 5] > 0).all()
    oblique = _oblique()[:1]                              # and an interpolating plane: n, sum a, sum a^2 equal; the rest within the edges
    got = _device_sums(vol, oblique, 1, lo, scale, 32, scaling)[0]
    ref, info = AR.moments(values, oblique[0], 1, lo, scale, 32, details=True)
    ne = K.n_edge(info, (lo, scale, lo, scale), 32, float(np.abs(values).max()), SHAPE)
    d = np.abs(got - ref)
    assert ref[0] > 0 and d[0] == 0 and d[1] == 0 and d[3] == 0 and d[2] <= ne and d[4] <= ne * 63 and d[5] <= ne * 31


def test_nan_and_inf_voxels_are_not_counted(noise):
    vol = noise.copy(order='F')
    mats = [_flip(0, SHAPE[0] - 1), _flip(1, SHAPE[1] - 1)]
    lo, scale = AR.bin_range(vol, 32)
    clean = AR.moments_of(vol, mats, 1, lo, scale, 32)
    vol[10, 5, 3], vol[11, 5, 3], vol[30, 20, 9] = np.nan, np.inf, -np.inf
    assert AR.bin_range(vol, 32) == (lo, scale)
    want = AR.moments_of(vol, mats, 1, lo, scale, 32)
    assert (clean[:, 0] - want[:, 0]).tolist() == [6, 6]   # each bad voxel is missing as a voxel and as a mirror image
    assert np.array_equal(_device_sums(vol, mats, 1, lo, scale, 32), want)
    oblique = _oblique()[:2]                              # a NaN neighbour poisons every trilinear value that reads it
    got, ref = _device_sums(vol, oblique, 1, lo, scale, 32), AR.moments_of(vol, oblique, 1, lo, scale, 32)
    assert np.array_equal(got[:, [0, 1, 3]], ref[:, [0, 1, 3]]) and (ref[:, 0] > 0).all()
    for k, M in enumerate(oblique):                      # sum b, sum b^2, sum a b: within what the samples on a bin edge can cause
        _, info = AR.moments(vol, M, 1, lo, scale, 32, details=True)
        ne = K.n_edge(info, (lo, scale, lo, scale), 32, float(np.abs(noise).max()), SHAPE)
        d = np.abs(got[k] - ref[k])
        assert ne <= 1e-3 * ref[k, 0] and d[2] <= ne and d[4] <= ne * 63 and d[5] <= ne * 31


def test_a_mirror_that_leaves_the_volume_counts_nothing(noise):
    from mudiff_hip import volume_align as VA
    mats = [_flip(0, -5.0), _flip(0, 1000.0), _flip(0, SHAPE[0] - 1)]
    lo, scale = AR.bin_range(noise, 32)
    got = _device_sums(noise, mats, 1, lo, scale, 32)
    assert not got[:2].any() and got[2, 0] == np.prod(SHAPE)
    r = VA.scores(got, VA.sample_points(SHAPE, 1))
    assert r[0] == -np.inf and r[1] == -np.inf and np.isfinite(r[2])


def test_c_abi_rejects_bad_arguments_without_launching():
    import mudiff_hip
    from mudiff_hip import ops
    lib = mudiff_hip.load()
    vol = torch.zeros(16 * 8 * 4, dtype=torch.int16, device=DEV)
    mats = torch.tensor([[-1.0, 0, 0, 15.0, 0, 1.0, 0, 0, 0, 0, 1.0, 0]] * 3, dtype=torch.float64, device=DEV)
    sums = torch.full((3 * 6 + 1,), 5, dtype=torch.int64, device=DEV)
    nan, inf = float('nan'), float('inf')

    def call(v=vol, dt=4, dims=(16, 8, 4), m=mats, k=3, stride=1, lo=0.0, scale=1.0, bins=32, s=sums, m_off=0, s_off=0):
        p = lambda t, off=0: None if t is None else t.data_ptr() + off      # noqa: E731
        return lib.mud_volume_mirror_moments(p(v), dt, *dims, 1.0, 0.0, p(m, m_off), k, stride, lo, scale, bins, p(s, s_off), None)

    assert call(s=None) == 1 and b'null' in lib.mud_last_error()
    assert call(v=None) == 1 and call(m=None) == 1
    assert call(dims=(0, 8, 4)) == 1 and call(dims=(16, 8, -1)) == 1 and call(dims=(2048, 2048, 512)) == 1
    assert call(dt=64) == 1 and b'datatype' in lib.mud_last_error()
    assert call(k=0) == 1 and b'candidates' in lib.mud_last_error()
    assert call(k=-3) == 1
    assert call(stride=0) == 1 and b'stride' in lib.mud_last_error()
    assert call(stride=-2) == 1
    assert call(bins=1) == 1 and b'bins' in lib.mud_last_error()
    assert call(bins=257) == 1
    for bad in (nan, inf):
        assert call(lo=bad) == 1 and b'finite' in lib.mud_last_error()
        assert call(scale=bad) == 1 and b'finite' in lib.mud_last_error()
    assert call(m_off=4) == 1 and b'aligned' in lib.mud_last_error()
    assert call(s_off=4) == 1 and b'aligned' in lib.mud_last_error()
    for bad in (nan, inf):                                # the matrices are device memory: the wrapper refuses them before it uploads them
        m = np.tile(np.eye(4)[:3], (3, 1, 1))
        m[1, 2, 3] = bad
        with pytest.raises(ValueError, match='finite'):
            ops.volume_mirror_moments(vol, 4, (16, 8, 4), 1.0, 0.0, m, 1, 0.0, 1.0, 32)
    with pytest.raises(ValueError, match='at least one'):
        ops.volume_mirror_moments(vol, 4, (16, 8, 4), 1.0, 0.0, np.zeros((0, 3, 4)), 1, 0.0, 1.0, 32)
    torch.cuda.synchronize()
    assert int(sums.min()) == 5 and int(sums.max()) == 5                           # nothing was launched, nothing cleared
    assert call() == 0                                                             # the library still works afterwards
    torch.cuda.synchronize()
    n = 16 * 8 * 4
    assert sums[:18].reshape(3, 6).tolist() == [[n, 0, 0, 0, 0, 0]] * 3 and int(sums[18]) == 5      # two zero volumes: everything in bin 0


# ---------------------------------------------------------------------------------------------------
# the search
# ---------------------------------------------------------------------------------------------------
def _both_searches(pose, A):
    """(device (T, report), host (T, report)) of the same search on the int16 head of `pose` on the grid of A."""
    from mudiff_hip import volume_align as VA
    from mudiff_hip.volume_coreg import grid_centre
    vol = AR.phantom(pose, A=A)
    centre = grid_centre(AR.SHAPE, A)
    dev = VA.estimate(VS.raw_volume(vol, affine=A), DEV, bins=AR.BINS, **AR.SEARCH)
    lo, scale = AR.bin_range(vol.astype(np.float32), AR.BINS)
    host = VA.finish(AR.host_cost(vol, A, centre, lo, scale, AR.BINS), lambda s: VA.sample_points(AR.SHAPE, s), centre, **AR.SEARCH)
    return dev, host


def test_the_device_search_is_the_host_search_on_the_exact_lattice_phantom():
    """An axis-aligned grid and a plane two voxels off its centre: the planted mirror maps voxels onto voxels.  Same parameters."""
    pose = (0.0, 0.0, 3.0)
    (T, dev), (_, host) = _both_searches(pose, AR.affine(oblique=False))
    print('device', {k: v for k, v in dev.items() if k != 'T'}, '| host', {k: v for k, v in host.items() if k != 'T'})
    assert (dev['yaw_deg'], dev['roll_deg'], dev['offset_mm']) == (host['yaw_deg'], host['roll_deg'], host['offset_mm']) == pose
    assert dev['kept'] == host['kept'] == 1 and dev['candidates'] == host['candidates'] == 677 and dev['levels'] == 5
    assert dev['r'] == host['r'] and dev['overlap'] == host['overlap'] and np.array_equal(T, np.array(host['T']))


def test_the_device_search_comes_within_one_final_step_of_the_host_search():
    pose = AR.POSES[0]
    (_, dev), (_, host) = _both_searches(pose, AR.affine())
    d = np.abs(np.array([dev[k] - host[k] for k in ('yaw_deg', 'roll_deg', 'offset_mm')]))
    err = np.abs(np.array([dev[k] for k in ('yaw_deg', 'roll_deg', 'offset_mm')]) - np.array(pose))
    print('device', {k: v for k, v in dev.items() if k != 'T'}, '| host', {k: v for k, v in host.items() if k != 'T'}, '| delta', d, '| error', err)
    assert dev['kept'] == 1 and d[0] <= 0.3125 and d[1] <= 0.3125 and d[2] <= 0.25
    assert err[0] <= 2 * 0.3125 and err[1] <= 2 * 0.3125 and err[2] <= 2 * 0.25
    assert abs(dev['r'] - host['r']) <= 1e-3 and abs(dev['r_identity'] - host['r_identity']) <= 1e-3


def test_the_fallbacks_on_the_device(capsys):
    from mudiff_hip import volume_align as VA
    T, rep = VA.estimate(VS.raw_volume(np.asfortranarray(np.full(AR.SHAPE, 7, np.int16)), affine=AR.affine()), DEV, bins=AR.BINS, **AR.SEARCH)
    assert np.array_equal(T, np.eye(4)) and rep['kept'] == 0 and rep['r'] is None
    T, rep = VA.estimate(VS.raw_volume(AR.phantom((30.0, 0.0, 0.0)), affine=AR.affine()), DEV, bins=AR.BINS, **AR.SEARCH)
    assert np.array_equal(T, np.eye(4)) and rep['kept'] == 0 and abs(rep['yaw_deg']) == 20.0
    assert capsys.readouterr().out.count('[align] warning:') == 2


# ---------------------------------------------------------------------------------------------------
# the pipeline: one tilted subject
# ---------------------------------------------------------------------------------------------------
POSE = AR.POSES[0]
GRID = dict(shape=(32, 30, 26), spacing=(2.25, 2.25, 3.0), target='LPS')
CONFORM = ['--conform', '--conform_shape', '32', '30', '26', '--conform_spacing', '2.25', '2.25', '3']
ALIGN = ['--align', '--align_strides', '2', '1']
A32 = AR.affine().astype(np.float32).astype(np.float64)  # what a header holds


def _contrasts():
    flair = AR.phantom(POSE, A=A32)
    base = flair.astype(np.float64)
    return dict(flair=flair, t2=np.asfortranarray(np.rint(1200.0 - 0.8 * base).astype(np.int16)),
                t1=np.asfortranarray(np.rint(300.0 + 0.5 * base + 2e-4 * base ** 2).astype(np.int16)),
                gt=np.asfortranarray((0.7 * base + 50.0).astype(np.float32)))


@pytest.fixture(scope='module')
def prepared():
    from mudiff_hip import volume_prepare as VP
    vols = _contrasts()
    named = [(name.upper(), VS.raw_volume(vols[name], affine=A32)) for name in ('flair', 't2', 't1')]
    plain = VP.IntakeOptions(conform=dict(GRID), antialias=True)
    options = plain._replace(align=dict(AR.SEARCH, bins=AR.BINS, min_overlap=0.5))
    return dict(named=named, aligned=VP.prepare_inputs(named, options, DEV), conformed=VP.prepare_inputs(named, plain, DEV))


def test_prepare_inputs_resamples_every_input_once_onto_the_turned_grid(prepared):
    from mudiff_hip import volume_align as VA
    from mudiff_hip import volume_conform as VCF
    from mudiff_hip import volume_regrid as VR
    from mudiff_hip.volume_coreg import grid_centre
    vols, ref, report = prepared['aligned']
    (name, rep), = report.align
    T = np.array(rep['T'])
    shape, conform_affine = VCF.conform_grid(AR.SHAPE, A32, **GRID)
    err = np.abs(np.array([rep['yaw_deg'], rep['roll_deg'], rep['offset_mm']]) - np.array(POSE))
    print('found', rep['yaw_deg'], rep['roll_deg'], rep['offset_mm'], 'errors', err, 'r', rep['r'], 'r_identity', rep['r_identity'])
    assert name == 'FLAIR' and rep['kept'] == 1 and err[0] <= 0.625 and err[1] <= 0.625 and err[2] <= 0.5
    assert np.array_equal(T, VA.pose_world((rep['yaw_deg'], rep['roll_deg'], rep['offset_mm']), grid_centre(AR.SHAPE, A32)))
    assert ref[0] == shape == GRID['shape'] and np.array_equal(ref[1], T @ conform_affine)
    assert np.allclose(ref[2].world_affine, T @ conform_affine, rtol=0, atol=1e-5) and ref[2].shape == shape
    for (_, raw), vol in zip(prepared['named'], vols):   # one interpolation: the direct resampling of the raw input onto that grid
        direct = VR.regrid_to(raw, shape, T @ conform_affine, DEV, antialias=True)
        assert isinstance(vol, VR.RegriddedVolume) and vol.shape == shape and np.array_equal(vol.affine, T @ conform_affine)
        assert np.array_equal(vol.values_float32(), direct.values_float32()) and float(np.abs(direct.values_float32()).max()) > 100
    assert report.suffix().endswith(f" | align=FLAIR:{rep['yaw_deg']:.2f}/{rep['roll_deg']:.2f}deg/{rep['offset_mm']:.2f}mm")
    assert [n for n, _ in report.conform] == ['FLAIR', 'T2', 'T1'] and prepared['conformed'][2].align == []
    assert np.array_equal(prepared['conformed'][1][1], conform_affine) and ' | align=' not in prepared['conformed'][2].suffix()


@pytest.mark.parametrize('reorient', [False, True])
def test_the_evaluation_inputs_land_on_the_turned_grid_and_the_plane_is_estimated_once(prepared, monkeypatch, reorient):
    """evaluation_inputs under --align: the ground truth comes back bit-equal to its direct resampling onto T @ conform_affine, not onto
    the plain conform grid; found['align'] carries the estimate, and prepare_inputs(align=found['align']) estimates nothing again, runs
    none of --reorient / --foreground on the first input again and returns what it returns on its own."""
    from mudiff_hip import volume_align as VA
    from mudiff_hip import volume_conform as VCF
    from mudiff_hip import volume_foreground as VF
    from mudiff_hip import volume_prepare as VP
    from mudiff_hip import volume_regrid as VR
    from mudiff_hip import volume_reorient as VO
    named = prepared['named']
    gt_raw = VS.raw_volume(_contrasts()['gt'], affine=A32)
    options = VP.IntakeOptions(conform=dict(GRID), antialias=True, align=dict(AR.SEARCH, bins=AR.BINS, min_overlap=0.5),
                               reorient=dict(target='LPS') if reorient else None, foreground=VF.options_from(_ns(foreground=True))['foreground'])
    gt_stored = VO.reorient(gt_raw, DEV, **options.reorient)[0] if reorient else gt_raw      # (an evaluation input is reoriented by its own affine first)
    calls = dict(estimate=0, reorient=0, foreground=0)

    def counted(module, name, key):
        inner = getattr(module, name)

        def wrapper(*a, **k):
            calls[key] += 1
            return inner(*a, **k)
        monkeypatch.setattr(module, name, wrapper)

    counted(VA, 'estimate', 'estimate')
    counted(VO, 'reorient', 'reorient')
    counted(VF, 'foreground', 'foreground')
    alone_vols, alone_ref, alone_report = VP.prepare_inputs(named, options, DEV)
    assert calls == dict(estimate=1, reorient=3 * reorient, foreground=3)
    for k in calls:
        calls[k] = 0
    (gt, label), resampled, found = VP.evaluation_inputs(named[0][1], gt_raw, None, options, DEV, names=('flair', 'gt'), wording=str)
    assert calls['estimate'] == 1 and calls['foreground'] == 1 and calls['reorient'] >= int(reorient)      # (the ground truth is reoriented too)
    align = found['align']
    assert isinstance(align, VP.Alignment) and label is None and resampled == ['gt_volume']
    assert np.array_equal(align.T, np.array(alone_report.align[0][1]['T'])) and align.report == alone_report.align[0][1] and align.report['kept'] == 1
    first_world = VR.world_affine_of(align.first.affine, align.first.header)
    shape, conform_affine = VCF.conform_grid(align.first.shape, first_world, **GRID)
    turned = align.T @ conform_affine
    assert np.array_equal(turned, alone_ref[1]) and not np.allclose(turned, conform_affine, atol=1e-3)
    on_turned = VR.regrid_to(gt_stored, shape, turned, DEV, antialias=True).values_float32()
    on_plain = VR.regrid_to(gt_stored, shape, conform_affine, DEV, antialias=True).values_float32()
    assert gt.shape == shape and np.array_equal(gt, on_turned.astype(np.float64))
    assert float(np.abs(on_turned.astype(np.float64) - on_plain).max()) > 50.0 and not np.array_equal(gt, on_plain.astype(np.float64))
    for k in calls:
        calls[k] = 0
    vols, ref, report = VP.prepare_inputs(named, options, DEV, align=align)
    assert calls == dict(estimate=0, reorient=2 * reorient, foreground=2)   # the later inputs only
    assert np.array_equal(ref[1], alone_ref[1]) and ref[0] == alone_ref[0]
    for a, b in zip(vols, alone_vols):
        assert np.array_equal(a.values_float32(), b.values_float32())
    assert report.align == alone_report.align and report.suffix() == alone_report.suffix()
    assert [n for n, _ in report.reorient] == [n for n, _ in alone_report.reorient] == (['FLAIR', 'T2', 'T1'] if reorient else [])
    assert [e[:2] for e in report.foreground] == [e[:2] for e in alone_report.foreground] and [e[0] for e in report.foreground] == ['FLAIR', 'T2', 'T1']
    assert json.dumps([e for _, e in report.reorient], default=str) == json.dumps([e for _, e in alone_report.reorient], default=str)
    # given the estimate, evaluation_inputs does not estimate either
    again = VP.evaluation_inputs(named[0][1], gt_raw, None, options, DEV, names=('flair', 'gt'), wording=str, align=align)
    assert calls['estimate'] == 0 and again[2]['align'] is align and np.array_equal(again[0][0], gt)


def _ns(**kw):
    import argparse
    return argparse.Namespace(**kw)


SYMMETRY_MARGIN = 0.01


def test_the_conformed_first_input_is_symmetric_about_its_centre_column(prepared):
    """Pearson r of the conformed FLAIR with its own left-right flip against the reported r (of 32 bins on the native grid, over the
    overlap).  SYMMETRY_MARGIN: on the numpy restatement (trilinear onto the grid turned by the host search's plane, no low-pass) the
    flip correlation is 0.9990 against a reported 0.9975, 0.0015 above it, and half a degree of yaw costs r about 0.0002 on this head;
    0.01 leaves room for the low-pass and for the device's plane, one final step away at most.  The --conform-only grid gives 0.61 there (0.636 on the device, behind the low-pass)."""
    rep = prepared['aligned'][2].align[0][1]
    aligned = AR.flip_correlation(prepared['aligned'][0][0].values_float32())
    conformed = AR.flip_correlation(prepared['conformed'][0][0].values_float32())
    print('flip correlation: aligned', aligned, 'conform only', conformed, 'reported r', rep['r'])
    assert aligned >= rep['r'] - SYMMETRY_MARGIN and aligned > conformed


# ---------------------------------------------------------------------------------------------------
# end to end: the tiny model of the other volume tests
# ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def runs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp('align')
    VS.write_tiny_model(tmp)
    vols = _contrasts()
    p = {k: R.write_nifti_typed(tmp / f'{k}.nii', v, affine=A32) for k, v in vols.items()}
    model = VS.model_argv(tmp, 3, 7, '--resize_back', '--input_flair', p['flair'], '--input_t2', p['t2'], '--input_t1', p['t1'])
    on = CONFORM + ALIGN
    jobs = {'host': on, 'dev': on + ['--device_intake'], 'back': on + ['--conform_back'], 'gt': on + ['--gt_volume', p['gt']], 'conform': CONFORM}
    steps = [VS.volume_step(k, model + a + ['--output_dir', str(tmp / k)]) for k, a in jobs.items()]
    manifest = tmp / 'cohort.tsv'
    manifest.write_text('id\tt1\tt1ce\tt2\tflair\ns_a\t' + '\t'.join([p['t1'], '', p['t2'], p['flair']]) + '\n')
    steps.append(VS.cohort_step('cohort', model[:model.index('--input_flair')] + on + ['--manifest', str(manifest), '--output_dir', str(tmp / 'cohort')]))
    log = VS.run_plan(tmp, steps, 600, ignore='all')
    return dict(tmp=tmp, log=log, files=p, pred=lambda k: VS.payload(str(tmp / k / 'predicted_t1ce.nii.gz')))


def test_predict_volume_align_end_to_end(runs):
    from mudiff_hip import volume as V
    from mudiff_hip import volume_conform as VCF
    tmp = runs['tmp']
    rep = json.load(open(tmp / 'host' / 'align_t1ce.json'))
    assert list(rep) == ['FLAIR'] and rep['FLAIR']['kept'] == 1
    found = rep['FLAIR']
    err = np.abs(np.array([found['yaw_deg'], found['roll_deg'], found['offset_mm']]) - np.array(POSE))
    assert err[0] <= 0.625 and err[1] <= 0.625 and err[2] <= 0.5
    assert set(found) >= {'yaw_deg', 'roll_deg', 'offset_mm', 'r', 'r_identity', 'overlap', 'candidates', 'levels', 'kept'}
    suffix = f" | align=FLAIR:{found['yaw_deg']:.2f}/{found['roll_deg']:.2f}deg/{found['offset_mm']:.2f}mm"
    for name in ('host', 'dev', 'back', 'gt'):
        assert json.load(open(tmp / name / 'align_t1ce.json')) == rep
        assert VS.done_line(runs['log'][name]).endswith(' | conform=32x30x26@2.25x2.25x3mm:FLAIR,T2,T1 | antialias=on' + suffix)
    assert runs['pred']('host') == runs['pred']('dev')                             # host file == device file, byte for byte
    assert runs['pred']('host') != runs['pred']('conform')                         # and the turned grid reached the sampler
    # the written sform is T @ conform_affine, to fp32
    shape, conform_affine = VCF.conform_grid(AR.SHAPE, A32, **GRID)
    want = (np.array(found['T']) @ conform_affine).astype(np.float32)
    for name in ('host', 'dev', 'gt'):
        _, hdr, code = V.open_nifti1(str(tmp / name / 'predicted_t1ce.nii.gz'))
        assert code == 16 and hdr.shape == shape and np.array_equal(hdr.world_affine.astype(np.float32), want)
    _, hdr, _ = V.open_nifti1(str(tmp / 'conform' / 'predicted_t1ce.nii.gz'))
    assert np.array_equal(hdr.world_affine.astype(np.float32), conform_affine.astype(np.float32))
    assert not os.path.exists(tmp / 'conform' / 'align_t1ce.json') and ' | align=' not in VS.done_line(runs['log']['conform'])
    # --conform_back: the prediction on the first input's own grid
    _, hdr, code = V.open_nifti1(str(tmp / 'back' / 'predicted_t1ce.nii.gz'))
    _, first, _ = V.open_nifti1(runs['files']['flair'])
    assert code == 16 and hdr.shape == AR.SHAPE and np.array_equal(hdr.world_affine, first.world_affine) and np.array_equal(hdr.world_affine, A32)
    back = V.read_nifti(str(tmp / 'back' / 'predicted_t1ce.nii.gz'))[0]
    assert np.isfinite(back).all() and float(back.max()) > 0.05
    # --gt_volume: scored on the turned grid (the same prediction, the ground truth resampled onto it, one estimate)
    assert runs['pred']('gt') == runs['pred']('host') and ' | regrid=gt_volume | ' in VS.done_line(runs['log']['gt'])
    assert runs['log']['gt'].count('[align]') == 0
    metrics = json.load(open(tmp / 'gt' / 'metrics_t1ce.json'))
    assert metrics['metrics']['slab']['voxels'] == 32 * 30 * 7
    # the cohort takes the flags from the same place
    assert json.load(open(tmp / 'cohort' / 's_a' / 'align_t1ce.json')) == rep
    assert suffix in VS.done_line(runs['log']['cohort'])
    assert VS.payload(str(tmp / 'cohort' / 's_a' / 'predicted_t1ce.nii.gz')) == runs['pred']('host')


def test_volume_and_cohort_estimate_once_and_score_on_the_turned_grid(runs, monkeypatch, tmp_path):
    """predict_volume and cohort.run with a ground truth, the sampling stubbed out: volume_align.estimate runs once per subject (the
    evaluation inputs' estimate is handed to prepare_inputs), and the ground truth that reaches the scoring is its direct resampling
    onto the grid the prediction has, T @ conform_affine."""
    from mudiff_hip import cohort as Co
    from mudiff_hip import volume as V
    from mudiff_hip import volume_align as VA
    from mudiff_hip import volume_conform as VCF
    from mudiff_hip import volume_intake as VI
    from mudiff_hip import volume_regrid as VR
    tmp, p = runs['tmp'], runs['files']
    T = np.array(json.load(open(tmp / 'host' / 'align_t1ce.json'))['FLAIR']['T'])
    shape, conform_affine = VCF.conform_grid(AR.SHAPE, A32, **GRID)
    turned = T @ conform_affine
    want = VR.regrid_to(VI.read_nifti_raw(p['gt']), shape, turned, DEV, antialias=True).values_float32().astype(np.float64)
    plain = VR.regrid_to(VI.read_nifti_raw(p['gt']), shape, conform_affine, DEV, antialias=True).values_float32().astype(np.float64)
    assert float(np.abs(want - plain).max()) > 50.0
    calls, seen = [], []
    estimate = VA.estimate
    monkeypatch.setattr(VA, 'estimate', lambda *a, **k: (calls.append(1), estimate(*a, **k))[1])
    monkeypatch.setattr(V, 'predict_from_conditions', lambda args, plan, evaluation, g1, g2, dev, stacks, ref, **kw: seen.append((evaluation, ref)))
    model = VS.model_argv(tmp, 3, 7, '--resize_back')
    inputs = ['--input_flair', p['flair'], '--input_t2', p['t2'], '--input_t1', p['t1']]
    for intake in ([], ['--device_intake']):
        V.predict_volume(V.build_argparser(model + inputs + CONFORM + ALIGN + intake + ['--gt_volume', p['gt'], '--output_dir', str(tmp_path / 'v')]))
    assert len(calls) == 2 and len(seen) == 2                                      # one estimate per run
    for (gt, label), ref in seen:
        assert label is None and ref[0] == shape and np.array_equal(ref[1], turned) and np.array_equal(gt, want)
    # the cohort: its own loop, the same hand-over
    manifest = tmp_path / 'scored.tsv'
    manifest.write_text('id\tt1\tt1ce\tt2\tflair\tgt\ns_a\t' + '\t'.join([p['t1'], '', p['t2'], p['flair'], p['gt']]) + '\n')
    args = Co.build_argparser(model + CONFORM + ALIGN + ['--score', '--manifest', str(manifest), '--output_dir', str(tmp_path / 'c')])
    del calls[:], seen[:]

    def stub(sargs, plan, evaluation, conds, ref, write, calibrate, timing):
        seen.append((evaluation, ref))
        raise ValueError('stop here')

    failures = Co.run(args, Co.read_manifest(args.manifest), predict=stub)[1]
    assert failures == [('s_a', 'ValueError: stop here')] and len(calls) == 1 and len(seen) == 1
    (gt, label), ref = seen[0]
    assert label is None and np.array_equal(ref[1], turned) and np.array_equal(gt, want)
