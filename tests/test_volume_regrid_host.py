"""CPU: the host side of --regrid: NiftiHeader.world_affine (sform / qform / pixdim), grid_matrix, same_grid,
the flag on the three command lines, and the numpy reference of the kernel (tests/volume_regrid_ref.py) against scipy where it imports."""
import struct

import numpy as np
import pytest

import volume_intake_ref as R
import volume_regrid_ref as G


# ---------------------------------------------------------------------------------------------------
# world_affine
# ---------------------------------------------------------------------------------------------------
def _header(sform=None, qform=None, pixdim=(1.0, 0.9, 1.1, 3.0)):
    """A little-endian NIfTI-1 header: sform = 3 x 4 rows or None; qform = (b, c, d, qoffset xyz) or None; pixdim[0..3]."""
    from mudiff_hip.volume import NiftiHeader
    raw = bytearray(348)
    struct.pack_into('<i', raw, 0, 348)
    struct.pack_into('<8h', raw, 40, 3, 5, 4, 3, 1, 1, 1, 1)
    struct.pack_into('<8f', raw, 76, *pixdim, 1.0, 1.0, 1.0, 1.0)
    if qform is not None:
        struct.pack_into('<h', raw, 252, 1)
        struct.pack_into('<6f', raw, 256, *qform)
    if sform is not None:
        struct.pack_into('<h', raw, 254, 2)
        for r in range(3):
            struct.pack_into('<4f', raw, 280 + 16 * r, *sform[r])
    raw[344:348] = b'n+1\0'
    return NiftiHeader(raw, '<')


def _quaternion_affine(b, c, d, offset, pix, qfac):
    """The NIfTI-1 standard's own formula (nifti1.h, METHOD 2)."""
    a = np.sqrt(max(0.0, 1.0 - (b * b + c * c + d * d)))
    rot = np.array([[a * a + b * b - c * c - d * d, 2 * b * c - 2 * a * d, 2 * b * d + 2 * a * c],
                    [2 * b * c + 2 * a * d, a * a + c * c - b * b - d * d, 2 * c * d - 2 * a * b],
                    [2 * b * d - 2 * a * c, 2 * c * d + 2 * a * b, a * a + d * d - c * c - b * b]])
    out = np.eye(4)
    out[:3, :3] = rot @ np.diag([pix[0], pix[1], pix[2] * qfac])
    out[:3, 3] = offset
    return out


SFORM = [(2.0, 0.0, 0.0, -7.0), (0.0, 0.0, -1.5, 4.0), (0.0, 3.0, 0.0, 9.5)]
QFORM = (0.0, 0.0, float(np.sin(0.2)), -11.5, 20.25, 3.0)           # a rotation about z by 0.4 rad


def test_world_affine_reads_a_qform_only_header():
    h = _header(qform=QFORM, pixdim=(-1.0, 0.9, 1.1, 3.0))
    want = _quaternion_affine(0.0, 0.0, np.sin(0.2), (-11.5, 20.25, 3.0), (0.9, 1.1, 3.0), -1.0)
    assert np.abs(h.world_affine - want).max() <= 1e-6
    c, s = np.cos(0.4), np.sin(0.4)                      # and what that formula means: Rz(0.4) . diag(pixdim), the third axis reversed
    assert np.abs(h.world_affine[:3, :3] - np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]]) @ np.diag([0.9, 1.1, -3.0])).max() <= 1e-6
    assert np.array_equal(h.affine, np.diag([np.float32(0.9), np.float32(1.1), 3.0, 1.0]))        # `affine` is what it was
    h0 = _header(qform=QFORM, pixdim=(0.0, 0.9, 1.1, 3.0))                                       # qfac 0 reads as +1
    assert np.abs(h0.world_affine - _quaternion_affine(0.0, 0.0, np.sin(0.2), (-11.5, 20.25, 3.0), (0.9, 1.1, 3.0), 1.0)).max() <= 1e-6


def test_world_affine_prefers_sform_and_falls_back_to_pixdim():
    both = _header(sform=SFORM, qform=QFORM)
    want = np.array(SFORM + [(0.0, 0.0, 0.0, 1.0)])
    assert np.array_equal(both.world_affine, want) and np.array_equal(both.affine, want)
    neither = _header()
    diag = np.diag([np.float32(0.9), np.float32(1.1), 3.0, 1.0]).astype(np.float64)
    assert np.array_equal(neither.world_affine, diag) and np.array_equal(neither.affine, diag)
    assert neither.world_affine.dtype == np.float64 and both.world_affine.shape == (4, 4)


# ---------------------------------------------------------------------------------------------------
# grid_matrix / same_grid / regrid_to on a volume that needs nothing
# ---------------------------------------------------------------------------------------------------
def test_grid_matrix_composes_shift_and_scale():
    from mudiff_hip import volume_regrid as VR
    eye = np.eye(4)
    shift = np.eye(4)
    shift[:3, 3] = (3.0, -2.0, 1.0)
    assert np.array_equal(VR.grid_matrix(eye, shift), shift)                       # reference voxel i is source voxel i + 3
    assert np.array_equal(VR.grid_matrix(shift, eye)[:3, 3], (-3.0, 2.0, -1.0))
    src = np.diag([1.0, 2.0, 1.0, 1.0])
    ref = np.diag([2.0, 1.0, 0.5, 1.0])
    ref[:3, 3] = (1.0, -1.0, 0.5)
    m = VR.grid_matrix(src, ref)
    assert m.dtype == np.float64 and np.array_equal(m[:3, :3], np.diag([2.0, 0.5, 0.5])) and np.array_equal(m[:, 3], (1.0, -0.5, 0.5, 1.0))
    _, sa, _, ra = G.case('oblique')
    m = VR.grid_matrix(sa, ra)
    centre_ref, centre_src = (np.array(G.REF_SHAPE) - 1) / 2.0, (np.array(G.SRC_SHAPE) - 1) / 2.0
    assert np.abs(m[:3, :3] @ centre_ref + m[:3, 3] - centre_src).max() < 1e-12     # the centres coincide
    assert np.abs(m - G.matrix(sa, ra)).max() < 1e-14


def test_grid_matrix_refuses_singular_and_non_finite_affines():
    from mudiff_hip import volume_regrid as VR
    flat = np.diag([1.0, 1.0, 0.0, 1.0])
    dependent = np.eye(4)
    dependent[:3, :3] = [[1.0, 2.0, 3.0], [2.0, 4.0, 6.0], [0.0, 1.0, 0.0]]
    nan = np.eye(4)
    nan[1, 3] = np.nan
    for bad in (flat, dependent, nan, np.zeros((4, 4)), np.eye(3)):
        with pytest.raises(ValueError):
            VR.grid_matrix(bad, np.eye(4))
        with pytest.raises(ValueError):
            VR.grid_matrix(np.eye(4), bad)


def test_same_grid_is_exact_in_float32(tmp_path):
    from mudiff_hip import volume as V
    from mudiff_hip import volume_intake as VI
    from mudiff_hip import volume_regrid as VR
    _, aff, _, _ = G.case('oblique')                                               # entries that float32 has to round
    vol = np.zeros((6, 5, 4), np.float32)
    p = str(tmp_path / 'v.nii.gz')
    V.write_nifti(p, vol, aff)
    raw = VI.read_nifti_raw(p)
    back = VR.world_affine_of(raw.affine, raw.header)
    assert not np.array_equal(back, aff) and VR.same_grid(vol.shape, aff, raw.shape, back)
    moved = aff.copy()
    moved[0, 3] += 1e-3                                                            # a 1e-3 mm offset is another grid
    assert not VR.same_grid(vol.shape, aff, vol.shape, moved)
    assert not VR.same_grid(vol.shape, aff, (6, 5, 5), aff)
    # a volume already on the reference grid is returned untouched: no upload, no launch (there is no device here to launch on)
    assert VR.regrid_to(raw, vol.shape, aff, device=None) is raw


# ---------------------------------------------------------------------------------------------------
# the command lines
# ---------------------------------------------------------------------------------------------------
def test_the_flag_is_on_all_three_command_lines_and_off_by_default():
    from mudiff_hip import cohort, volume, volume_metrics
    base = ['--target_modality', 'T1CE', '--output_dir', 'o', '--exp', 'e']
    assert volume.build_argparser(base).regrid is False and volume.build_argparser(base + ['--regrid']).regrid is True
    assert cohort.build_argparser(base + ['--manifest', 'm.tsv']).regrid is False
    assert cohort.build_argparser(base + ['--manifest', 'm.tsv', '--regrid']).regrid is True
    scoring = ['--pred', 'p.nii.gz', '--gt', 'g.nii.gz']
    assert volume_metrics.build_parser().parse_args(scoring).regrid is False
    assert volume_metrics.build_parser().parse_args(scoring + ['--regrid']).regrid is True
    assert volume.regrid_suffix([]) == '' and volume.regrid_suffix(None) == '' and volume.regrid_suffix(['T2', 'gt_volume']) == ' | regrid=T2,gt_volume'


# ---------------------------------------------------------------------------------------------------
# the reference itself
# ---------------------------------------------------------------------------------------------------
def test_reference_basics():
    src = R.synthetic(G.SRC_SHAPE, 'noise', 'f4', seed=41)
    for name in ('identity', 'shift', 'flip'):
        ss, sa, rs, ra = G.case(name)
        got, near = G.trilinear(src, G.matrix(sa, ra), rs), G.nearest(src, G.matrix(sa, ra), rs)
        assert np.array_equal(got, near)                                           # integer coordinates: both pick stored voxels
    assert np.array_equal(G.trilinear(src, G.matrix(*G.case('identity')[1::2]), G.SRC_SHAPE), src)
    ss, sa, rs, ra = G.case('shift')
    got = G.trilinear(src, G.matrix(sa, ra), rs)
    assert np.array_equal(got[:67, 2:, :16], src[3:, :16, 1:]) and not got[67:].any() and not got[:, :2].any() and not got[:, :, 16:].any()
    ss, sa, rs, ra = G.case('flip')
    assert np.array_equal(G.trilinear(src, G.matrix(sa, ra), rs)[:70, :18, :17], src[::-1, ::-1][:, :18])
    ss, sa, rs, ra = G.case('outside')
    assert not G.trilinear(src, G.matrix(sa, ra), rs).any() and not G.nearest(src, G.matrix(sa, ra), rs).any()
    ss, sa, rs, ra = G.case('oblique')
    assert np.count_nonzero(G.trilinear(src, G.matrix(sa, ra), rs)) >= 0.4 * np.prod(rs)
    assert not G.near_half_integer(G.matrix(sa, ra), rs).any()
    ss, sa, rs, ra = G.case('dyadic')
    assert G.near_half_integer(G.matrix(sa, ra), rs).mean() == 0.75                # exact ties: resolved by exact arithmetic


@pytest.mark.parametrize('name', ['oblique', 'dyadic'])
def test_reference_agrees_with_scipy(name):
    ndimage = pytest.importorskip('scipy.ndimage')
    src = R.synthetic(G.SRC_SHAPE, 'noise', 'f4', seed=42)
    ss, sa, rs, ra = G.case(name)
    M = G.matrix(sa, ra)
    want = ndimage.affine_transform(src.astype(np.float64), M[:3, :3], offset=M[:3, 3], output_shape=rs, order=1, mode='grid-constant', cval=0.0)
    got = G.trilinear(src, M, rs)
    err = np.abs(got.astype(np.float64) - want).max() / np.abs(src).max()
    print(name, 'max |reference - scipy| / max|src| =', err)
    assert err <= 1e-6
