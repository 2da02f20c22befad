"""CPU: the host side of --reorient (mudiff_hip.volume_reorient) against its numpy restatement
(tests/volume_reorient_ref.py): orientation codes and obliquity, the 48 x 48 plans and their affines, the header, the flags, the place of
the stage in prepare_inputs and the write-back wrapper.  Every comparison is an equality unless an affine is oblique."""
import itertools
import json
import struct

import numpy as np
import pytest

import volume_reorient_ref as R
from volume_support import raw_volume

BASE = ['--target_modality', 'T1CE', '--output_dir', 'o', '--exp', 'e']
SAGITTAL, CORONAL = 'PSL', 'LSP'                    # storage axes of a sagittal / a coronal acquisition


def _cases():
    shape = (5, 4, 3)
    return {'brats': R.BRATS, 'identity': np.eye(4), 'sagittal': R.affine_of(SAGITTAL, shape, origin=(3.0, -2.0, 7.5)),
            'coronal': R.affine_of(CORONAL, shape), 'anisotropic': R.affine_of('RAS', shape, spacing=(0.5, 0.5, 5.0)),
            'anisotropic_sagittal': R.affine_of(SAGITTAL, shape, spacing=(0.5, 5.0, 0.5))}


WANT = {'brats': 'LPS', 'identity': 'RAS', 'sagittal': SAGITTAL, 'coronal': CORONAL, 'anisotropic': 'RAS', 'anisotropic_sagittal': SAGITTAL}


def test_axcodes_and_obliquity():
    from mudiff_hip import volume_reorient as VO
    assert len(VO.TARGETS) == 48 and sorted(VO.TARGETS) == sorted(R.CODES)
    for name, a in _cases().items():
        assert VO.axcodes(a) == VO.axcodes(a[:3, :3]) == R.axcodes(a) == WANT[name], name
        assert VO.obliquity_deg(a) == 0.0
        for axis in range(3):                        # 12 degrees about a world axis: the codes stay, two voxel axes are tilted by 12
            tilted = R.rotation(axis, 12.0) @ a
            assert VO.axcodes(tilted) == R.axcodes(tilted) == WANT[name], (name, axis)
            assert abs(VO.obliquity_deg(tilted) - 12.0) <= 1e-9
    for bad in (np.zeros((4, 4)), np.diag([1.0, 1.0, 0.0, 1.0]), np.array([[1.0, 1, 0, 0], [1, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]])):
        with pytest.raises(ValueError, match='singular'):
            VO.axcodes(bad)
    nan = np.eye(4)
    nan[0, 0] = np.nan
    with pytest.raises(ValueError, match='finite'):
        VO.axcodes(nan)


def _indices(shape):
    return np.stack(np.meshgrid(*[np.arange(s) for s in shape], indexing='ij'), -1).reshape(-1, 3)


@pytest.mark.parametrize('oblique', [False, True])
def test_all_48_x_48_plans(oblique):
    from mudiff_hip import volume_reorient as VO
    shape = (5, 4, 3)
    vol = R.labelled(shape, 4)
    src_idx = np.arange(60).reshape(shape, order='F')                  # the linear source index of every voxel
    for source, target in itertools.product(R.CODES, R.CODES):
        a = R.affine_of(source, shape, spacing=(1.0, 2.0, 0.5), origin=(-7.0, 11.0, 3.0))      # integer-valued in fp64 terms: dyadic
        if oblique:
            a = R.rotation(1, 12.0) @ a
        p = VO.plan(shape, a, target)
        assert (p.source, p.target) == (source, target) and p.identity == (source == target)
        assert p.shape == tuple(shape[q] for q in p.perm)
        assert VO.axcodes(p.affine) == target
        moved = R.apply(vol, p.perm, p.flip)
        assert moved.shape == p.shape and np.array_equal(np.asarray(VO.apply_host(vol, p)), moved)
        # every voxel keeps its world position: p.affine @ (i, 1) == a @ (source index, 1)
        where = R.apply(src_idx, p.perm, p.flip)
        i = _indices(p.shape)
        j = np.stack(np.unravel_index(where.reshape(-1), shape, order='F'), -1)
        got = np.c_[i, np.ones(len(i))] @ p.affine.T
        want = np.c_[j, np.ones(len(j))] @ a.T
        if oblique:
            assert np.abs(got - want).max() <= 1e-9
        else:
            assert np.array_equal(got, want)
        assert np.array_equal(np.c_[i, np.ones(len(i))] @ p.matrix.T, np.c_[j, np.ones(len(j))])
        # composed with its inverse: the identity
        back = p.inverse()
        assert np.array_equal(R.apply(moved, back.perm, back.flip), vol) and back.shape == shape
        assert np.array_equal(back.matrix @ p.matrix, np.eye(4)) and np.array_equal(p.matrix @ back.matrix, np.eye(4))
        assert np.array_equal(back.affine, a) and (back.source, back.target) == (target, source)
    for bad in ('LLS', 'RA', 'XYZ', 'LPSI', ''):
        with pytest.raises(ValueError, match='reorient_to'):
            VO.plan(shape, np.eye(4), bad)
    with pytest.raises(ValueError, match='3D'):
        VO.plan((4, 4), np.eye(4))


def _header(shape, pixdim, sform=None, qform=None, slope=0.25, inter=-3.0):
    from mudiff_hip.volume import NiftiHeader
    raw = bytearray(348)
    struct.pack_into('<i', raw, 0, 348)
    struct.pack_into('<8h', raw, 40, 3, *shape, 1, 1, 1, 1)
    struct.pack_into('<h', raw, 70, 4)
    struct.pack_into('<h', raw, 72, 16)
    struct.pack_into('<8f', raw, 76, *pixdim)
    struct.pack_into('<f', raw, 108, 352.0)
    struct.pack_into('<2f', raw, 112, slope, inter)
    raw[148:148 + 11] = b'description'
    if sform is not None:
        struct.pack_into('<h', raw, 254, 2)
        for r in range(3):
            struct.pack_into('<4f', raw, 280 + 16 * r, *[float(v) for v in sform[r]])
    if qform is not None:
        struct.pack_into('<h', raw, 252, 1)
        struct.pack_into('<3f', raw, 256, *qform[0])
        struct.pack_into('<3f', raw, 268, *qform[1])
    raw[344:348] = b'n+1\0'
    return NiftiHeader(bytes(raw), '<')


def test_reoriented_header():
    from mudiff_hip import volume_reorient as VO
    shape, pix = (5, 4, 3), (1.0, 0.5, 2.0, 5.0, 1.0, 1.0, 1.0, 1.0)
    a = R.affine_of('RAS', shape, spacing=pix[1:4], origin=(1.0, 2.0, 3.0))
    hdr = _header(shape, pix, sform=a, qform=((0.1, 0.2, 0.3), (9.0, 9.0, 9.0)))
    p = VO.plan(shape, hdr.world_affine, SAGITTAL)
    out = VO.reoriented_header(hdr, p)
    assert out.shape == p.shape == (4, 3, 5)
    assert out._get('8f', 76) == (1.0, 2.0, 5.0, 0.5, 1.0, 1.0, 1.0, 1.0)
    assert out._get('h', 252)[0] == 0 and out._get('h', 254)[0] == 2          # no qform; the sform code is kept when it was set
    assert np.array_equal(out.world_affine, p.affine.astype(np.float32).astype(np.float64)) and np.array_equal(out.affine, out.world_affine)
    changed = [k for k in range(348) if out.raw[k] != hdr.raw[k]]
    assert all(42 <= k < 48 or 80 <= k < 92 or 252 <= k < 254 or 280 <= k < 328 for k in changed), changed
    assert out._get('h', 70)[0] == 4 and out._get('2f', 112) == (0.25, -3.0) and out.raw[148:159] == b'description'
    assert VO.reoriented_header(None, p) is None and hdr.raw == _header(shape, pix, sform=a, qform=((0.1, 0.2, 0.3), (9.0, 9.0, 9.0))).raw
    # geometry only in the qform (a rotation by 90 degrees about z, qfac = -1): the corners stay where they were
    s = float(np.sqrt(0.5))
    q = _header(shape, (-1.0, 0.5, 2.0, 5.0, 1.0, 1.0, 1.0, 1.0), qform=((0.0, 0.0, s), (10.0, -20.0, 30.0)))
    assert q._get('h', 254)[0] == 0
    world = q.world_affine
    for target in ('LPS', 'RAS', SAGITTAL):
        p = VO.plan(shape, world, target)
        out = VO.reoriented_header(q, p)
        assert out._get('h', 252)[0] == 0 and out._get('h', 254)[0] == 1 and VO.axcodes(out.world_affine) == target
        for corner in itertools.product(*[(0, s_ - 1) for s_ in p.shape]):
            i = np.array(corner + (1,), np.float64)
            want = world @ (p.matrix @ i)
            assert np.abs(out.world_affine @ i - want).max() <= 1e-6 * max(1.0, np.abs(want).max())      # fp32 rounding of the sform


def test_flags_and_options():
    from mudiff_hip import cohort, volume as V
    from mudiff_hip.volume_prepare import IntakeOptions
    args = V.build_argparser(BASE)
    assert (args.reorient, args.reorient_to, args.reorient_back) == (False, 'LPS', False)
    assert IntakeOptions.from_args(args).reorient is None and IntakeOptions().reorient is None
    assert IntakeOptions._fields[-1] == 'denoise' and IntakeOptions._fields[:5] == ('norm', 'regrid', 'coreg', 'bias', 'half_range')
    assert IntakeOptions.from_args(V.build_argparser(BASE + ['--reorient'])).reorient == dict(target='LPS')
    assert IntakeOptions.from_args(V.build_argparser(BASE + ['--reorient', '--reorient_to', 'ras'])).reorient == dict(target='RAS')
    import argparse
    assert IntakeOptions.from_args(argparse.Namespace(reorient=True)).reorient == dict(target='LPS')      # the defaults live in from_args
    assert IntakeOptions.from_args(argparse.Namespace()).reorient is None
    for bad in ('LLS', 'RA', 'XYZ'):
        with pytest.raises(ValueError, match='reorient_to'):
            IntakeOptions.from_args(argparse.Namespace(reorient=True, reorient_to=bad))
        with pytest.raises(SystemExit):
            V.build_argparser(BASE + ['--reorient', '--reorient_to', bad])
    with pytest.raises(SystemExit):
        V.build_argparser(BASE + ['--reorient_back'])
    assert V.build_argparser(BASE + ['--reorient', '--reorient_back']).reorient_back
    assert cohort.build_argparser(BASE + ['--manifest', 'm.tsv', '--reorient', '--reorient_to', 'PSL']).reorient_to == 'PSL'
    assert 'untuned' in V.make_parser().format_help()


def test_suffix_and_reports(tmp_path):
    from mudiff_hip import volume_reorient as VO
    from mudiff_hip.volume_prepare import IntakeReport
    moved = VO.plan((5, 4, 3), np.eye(4), 'LPS').entry()
    same = VO.plan((5, 4, 3), R.BRATS, 'LPS').entry()
    assert moved == {'from': 'RAS', 'to': 'LPS', 'perm': [0, 1, 2], 'flip': [True, True, False], 'shape_from': [5, 4, 3], 'shape_to': [5, 4, 3],
                     'obliquity_deg': 0.0, 'moved': True}
    assert same['moved'] is False and same['from'] == same['to'] == 'LPS'
    sag = VO.plan((5, 4, 3), R.affine_of(SAGITTAL, (5, 4, 3)), 'LPS').entry()
    assert (sag['perm'], sag['flip'], sag['shape_to']) == ([2, 0, 1], [False, False, False], [3, 5, 4])
    entries = [('T1', moved), ('T2', same), ('FLAIR', sag)]
    assert VO.reorient_suffix(entries) == ' | reorient=T1:RAS>LPS,T2:same,FLAIR:PSL>LPS' and VO.reorient_suffix([]) == ''
    report = IntakeReport()
    assert report.suffix() == ''
    report.reorient += entries
    assert report.suffix() == ' | reorient=T1:RAS>LPS,T2:same,FLAIR:PSL>LPS'
    report.write(str(tmp_path), 'T1CE', np.eye(4), None)
    assert [f.name for f in tmp_path.iterdir()] == ['reorient_t1ce.json']
    assert json.load(open(tmp_path / 'reorient_t1ce.json')) == {'T1': moved, 'T2': same, 'FLAIR': sag}


def _raw(vol, affine):
    return raw_volume(np.asarray(vol, np.int16), affine=np.asarray(affine, np.float64))


def _host_reorient(raw, device, target='LPS'):
    """volume_reorient.reorient with the device's permutation replaced by the restatement's."""
    from mudiff_hip import volume_reorient as VO
    p = VO.plan(raw.shape, raw.affine, target)
    if p.identity:
        return raw, p.entry()
    out = _raw(R.apply(raw.values_float64(), p.perm, p.flip), p.affine)
    return out, p.entry()


def test_prepare_inputs_reorients_first(monkeypatch, capsys):
    from mudiff_hip import volume_denoise as VD, volume_prepare as VP, volume_reorient as VO
    shape = (6, 5, 8)
    lps = R.labelled(shape, 2).astype(np.int16)
    order = []
    monkeypatch.setattr(VO, 'reorient', lambda raw, device, **kw: (order.append(('reorient', raw.shape, kw)), _host_reorient(raw, device, **kw))[1])
    monkeypatch.setattr(VD, 'denoise', lambda raw, device, **kw: (order.append(('denoise', raw.shape)), (raw, dict(sigma=0.0)))[1])
    named = [('FLAIR', _raw(*R.stored_as(lps, R.BRATS, SAGITTAL))), ('T2', _raw(lps, R.BRATS)), ('T1', _raw(*R.stored_as(lps, R.BRATS, 'RAS')))]
    options = VP.IntakeOptions(half_range=2, reorient=dict(target='LPS'), denoise=dict(VD.DEFAULTS))
    prepared, ref, report = VP.prepare_inputs(named, options, 'cpu')
    assert [o[0] for o in order] == ['reorient'] * 3 + ['denoise'] * 3                         # stage 0, before --denoise
    assert [o[1] for o in order] == [(5, 8, 6), shape, shape] + [shape] * 3 and order[0][2] == dict(target='LPS')
    assert ref[0] == shape and np.array_equal(ref[1], R.BRATS) and ref[3:] == (2, 6)           # the slab of the reoriented first input
    assert prepared[1] is named[1][1]                                                          # stored LPS already: untouched
    for vol in prepared:
        assert np.array_equal(vol.values_float64(), lps)
    assert report.suffix() == ' | denoise=FLAIR,T2,T1 | reorient=FLAIR:PSL>LPS,T2:same,T1:RAS>LPS'
    assert capsys.readouterr().out == ''
    # the shape check sees reoriented shapes: these three differ as stored and agree once reoriented ...
    assert len({raw.shape for _, raw in named}) == 2
    with pytest.raises(ValueError, match='share shape'):
        VP.prepare_inputs(named, VP.IntakeOptions(half_range=2), 'cpu')
    # ... and the other way round
    odd = [('FLAIR', _raw(np.zeros((5, 8, 6)), R.affine_of(SAGITTAL, (5, 8, 6)))), ('T2', _raw(np.zeros((5, 8, 6)), R.BRATS))]
    with pytest.raises(ValueError, match=r'share shape. Got \(5, 8, 6\) vs \(6, 5, 8\) for T2'):
        VP.prepare_inputs(odd, VP.IntakeOptions(half_range=2, reorient=dict(target='LPS')), 'cpu')
    # an oblique input is warned about, once per input, and still permuted
    tilted = [('T1', _raw(lps, R.rotation(0, 12.0) @ R.BRATS))]
    VP.prepare_inputs(tilted, VP.IntakeOptions(half_range=2, reorient=dict(target='RAS')), 'cpu')
    out = capsys.readouterr().out.splitlines()
    assert len(out) == 1 and out[0].startswith('[reorient] warning: T1:') and '12.0 degrees' in out[0]
    assert VO.OBLIQUE_WARN_DEG == 10.0


def test_write_back_returns_the_stored_order():
    from mudiff_hip import volume_reorient as VO
    shape = (6, 5, 8)
    lps = R.labelled(shape, 4).astype(np.float32)
    for code in ('RAS', SAGITTAL, CORONAL, 'LPS'):
        stored, affine = R.stored_as(lps, R.BRATS, code)
        first = _raw(np.zeros(stored.shape), affine)
        ref, p = VO.reference_of(first, 'LPS')
        assert ref[0] == shape and np.array_equal(ref[1], R.BRATS) and ref[2] is None and p.identity == (code == 'LPS')
        first.header = 'the original header'
        assert np.array_equal(R.apply(stored, p.perm, p.flip), lps)
        calls = []
        write = VO.write_back(lambda *a: calls.append(a), first, target='LPS')
        write('p.nii.gz', lps, ref[1], ref[2])                                    # the prediction arrives on the reoriented grid
        (path, vol, aff, hdr), = calls
        assert path == 'p.nii.gz' and np.array_equal(vol, stored) and vol.shape == stored.shape
        assert aff is first.affine and hdr == 'the original header'
        assert np.asarray(vol).tobytes(order='F') == stored.tobytes(order='F')    # what write_nifti serialises
