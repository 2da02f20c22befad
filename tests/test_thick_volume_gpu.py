"""GPU: --known_thick end to end on the tiny model (mudiff_hip.thick through mudiff_hip.volume and mudiff_hip.cohort; DESIGN.md section
5.27): 16 x 16 x 13 phantoms, S = 16, L = 3, G = 1 (slabs 0..2, 4..6, 8..10 and a cut one at 12), every run in one child process under
MUD_DETERMINISTIC=1 (tests/volume_support.py)."""
import json
import os

import numpy as np
import pytest

import thick_ref as R
import volume_support as VS

pytestmark = pytest.mark.gpu
S, Z, L, G = 16, 13, 3, 1
TH = ['--known_thick', str(L), '--thick_gap', str(G), '--thick_profile', 'gauss']
SLABS = [(0, 2), (4, 6), (8, 10), (12, 12)]


def _phantom(shape, i):
    x, y, z = np.meshgrid(*(np.arange(float(n)) for n in shape), indexing='ij')
    return (120 + 60 * np.sin(x / (3 + i) + 0.3 * z) * np.cos(y / (4.5 - i) - 0.2 * z) + 4 * z).astype(np.float32)


@pytest.fixture(scope='module')
def runs(tmp_path_factory):
    from mudiff_hip import volume as V
    tmp = tmp_path_factory.mktemp('thick')
    VS.write_tiny_model(tmp)
    p = {k: str(tmp / f'{k}.nii.gz') for k in ('flair', 't2', 't1', 'K')}
    for i, k in enumerate(p):
        V.write_nifti(p[k], _phantom((16, 16, Z), i), np.eye(4))
    inputs = ['--input_flair', p['flair'], '--input_t2', p['t2'], '--input_t1', p['t1']]
    known = inputs + ['--known_volume', p['K']]
    jobs = {'plain': (6, 7, inputs, {}), 'plain_old': (6, 7, inputs, dict(strip=['known_thick', 'thick_'])),
            'th': (6, 7, known + TH, {}), 'th_dev': (6, 7, known + TH + ['--device_intake'], {}), 'th_b4': (6, 4, known + TH, {}),
            'th_hr5': (5, 7, known + TH, {}), 'drop': (6, 7, known + TH + ['--known_drop_slices', '5:5'], {}),
            'ens': (6, 7, known + TH + ['--num_samples', '2'], {}), 'ens_b4': (6, 4, known + TH + ['--num_samples', '2'], {}),
            'interp': (6, 7, known + TH + ['--thick_interp', '--gt_volume', p['K'], '--through_plane'], {}),
            'small': (6, 2, known + TH, dict(raises=True))}
    steps = [VS.volume_step(k, VS.model_argv(tmp, hr, b) + a + ['--output_dir', str(tmp / k)], **o) for k, (hr, b, a, o) in jobs.items()]
    manifest = tmp / 'cohort.tsv'
    manifest.write_text('id\tt1\tt1ce\tt2\tflair\tknown\ns0\t' + '\t'.join([p['t1'], '', p['t2'], p['flair'], p['K']]) + '\n')
    steps.append(VS.cohort_step('cohort', VS.model_argv(tmp, 6, 7) + TH + ['--manifest', str(manifest), '--output_dir', str(tmp / 'cohort')]))
    log = VS.run_plan(tmp, steps, 900, ignore='RuntimeWarning')
    vol = lambda path: V.read_nifti(str(path))[0]             # noqa: E731
    return dict(tmp=tmp, log=log, p=p, vol=vol, pred=lambda k, suffix='': vol(tmp / k / f'predicted_t1ce{suffix}.nii.gz'),
                bytes=lambda k, suffix='': VS.payload(str(tmp / k / f'predicted_t1ce{suffix}.nii.gz')),
                report=lambda k: json.load(open(tmp / k / 'thick_t1ce.json')))


def _residuals_under_the_rule(rep):
    """Every measured slab: |A x - y| <= 3 (L + 4) 2^-24 (|A |x_new|| + |y|) in L2 over the slab's pixels: the constraint's chain
    (thick_ref.bound_residual), the check's own weighted sum of a result that is at most x_new's size and the residual's, and y's."""
    worst = 0.0
    for s in rep['slabs']:
        assert (s['residual'] is None) == (not s['measured'])
        if s['measured']:
            assert s['y_norm'] > 0 and 0 <= s['residual'] * s['y_norm'] <= 3 * (L + 4) * R.EPS * (s['x_norm'] + s['y_norm']), s
            worst = max(worst, s['residual'])
    return worst


def test_report_and_residuals(runs):
    rep = runs['report']('th')
    w32 = R.profile(L, 'gauss').astype(np.float32)
    assert (rep['L'], rep['gap'], rep['offset'], rep['profile'], rep['image_size'], rep['slab'], rep['resample']) == (L, G, 0, 'gauss', S, [0, Z - 1], 1)
    assert rep['weights'] == [float(v) for v in w32] and rep['sum_w2'] == float((w32.astype(np.float64) ** 2).sum())
    assert [(s['first'], s['last'], s['measured']) for s in rep['slabs']] == [(a, b, b - a + 1 == L) for a, b in SLABS] and rep['measured_slabs'] == 3
    worst = _residuals_under_the_rule(rep)
    print(f'worst residual {worst:.3e}')
    assert rep['max_residual'] == worst
    pred, plain = runs['pred']('th'), runs['pred']('plain')
    assert pred.shape == (16, 16, Z) and np.isfinite(pred).all() and (pred != plain).any()
    assert VS.done_line(runs['log']['th']).endswith(f' | thick={L}+{G} gauss (3/4 slabs)')
    assert sorted(os.listdir(runs['tmp'] / 'th')) == ['predicted_t1ce.nii.gz', 'thick_t1ce.json']
    # away from the clip, the written slab averages are those of K (the [0,1] map is affine)
    from mudiff_hip import volume as V
    k01 = 0.5 * np.asarray(V.normalise_volume(np.asarray(runs['vol'](runs['p']['K']), np.float64)), np.float32).astype(np.float64) + 0.5
    for a, b in SLABS[:3]:
        got, want = (pred[:, :, a:b + 1].astype(np.float64) * w32).sum(2), (k01[:, :, a:b + 1] * w32).sum(2)
        inside = ((pred[:, :, a:b + 1] > 0) & (pred[:, :, a:b + 1] < 1)).all(2)
        assert inside.any() and np.abs(got - want)[inside].max() <= 1e-5


def test_intake_batch_size_and_cohort_give_the_same_bytes(runs):
    assert runs['bytes']('th') == runs['bytes']('th_dev')
    assert runs['bytes']('th') == runs['bytes']('th_b4')
    assert runs['bytes']('th') == VS.payload(str(runs['tmp'] / 'cohort' / 's0' / 'predicted_t1ce.nii.gz'))
    assert json.load(open(runs['tmp'] / 'cohort' / 's0' / 'thick_t1ce.json')) == runs['report']('th') == runs['report']('th_b4')
    assert VS.done_line(runs['log']['cohort']).endswith(VS.done_line(runs['log']['th']).split(' | slices=')[1])
    small = runs['log']['small']                              # a slab of 3 thin slices does not fit a batch of 2
    assert '--batch_size 2 ' in small['error']


def test_the_slabs_belong_to_the_volume_not_to_the_sampled_range(runs):
    """--slice_half_range 5 samples slices 1..11: slab 0..2 is cut and sampled freely, the others are where they were (the draws are
    keyed by the slice's index in the sampled range, so the bytes are another run's)."""
    rep = runs['report']('th_hr5')
    assert rep['slab'] == [1, 11] and [(s['first'], s['last'], s['measured']) for s in rep['slabs']] == [(0, 2, False), (4, 6, True), (8, 10, True), (12, 12, False)]
    _residuals_under_the_rule(rep)
    assert VS.done_line(runs['log']['th_hr5']).endswith(f' | thick={L}+{G} gauss (2/4 slabs)')


def test_without_the_flags_nothing_changes(runs):
    """The run without the flags writes the bytes the commit before them wrote (recorded: tests/golden/thick_parent_payloads.json), a
    namespace as the parser left it before these flags existed gives the same, and those runs write nothing new."""
    import hashlib
    from conftest import REPO
    with open(os.path.join(REPO, 'tests', 'golden', 'thick_parent_payloads.json')) as f:
        recorded = json.load(f)
    assert hashlib.sha256(runs['bytes']('plain')).hexdigest() == recorded['plain']
    assert runs['bytes']('plain') == runs['bytes']('plain_old')
    assert ' | thick=' not in VS.done_line(runs['log']['plain']) and sorted(os.listdir(runs['tmp'] / 'plain')) == ['predicted_t1ce.nii.gz']


def test_a_dropped_slice_frees_its_whole_slab(runs):
    rep = runs['report']('drop')
    assert [s['measured'] for s in rep['slabs']] == [True, False, True, False] and rep['drop_slices'] == [[5, 5]] and rep['measured_slabs'] == 2
    assert rep['slabs'][1]['residual'] is None
    _residuals_under_the_rule(rep)
    drop, th = runs['pred']('drop'), runs['pred']('th')
    assert all((drop[:, :, z] != th[:, :, z]).any() for z in (4, 5, 6))          # the whole slab is sampled freely ...
    keep = [0, 1, 2, 3, 7, 8, 9, 10, 11, 12]
    assert np.array_equal(drop[:, :, keep], th[:, :, keep])                       # ... and no other slice notices


def test_ensemble(runs):
    tmp = runs['tmp']
    assert sorted(os.listdir(tmp / 'ens')) == ['predicted_t1ce.nii.gz', 'predicted_t1ce_std.nii.gz', 'thick_t1ce.json']
    mean, std = runs['pred']('ens'), runs['pred']('ens', '_std')
    assert np.isfinite(mean).all() and np.isfinite(std).all() and std.any()
    rep = runs['report']('ens')
    assert rep['measured_slabs'] == 3
    _residuals_under_the_rule(rep)                             # the largest over both samples
    assert f' | 2 samples per slice | thick={L}+{G} gauss (3/4 slabs)' in VS.done_line(runs['log']['ens'])
    for suffix in ('', '_std'):                                # a (slab, sample) group travels whole whatever the batch size
        assert runs['bytes']('ens', suffix) == runs['bytes']('ens_b4', suffix)
    assert runs['report']('ens_b4') == rep


def test_the_interpolated_baseline(runs):
    tmp = runs['tmp']
    assert sorted(os.listdir(tmp / 'interp')) == ['metrics_t1ce.json', 'metrics_thick_interp_t1ce.json', 'predicted_t1ce.nii.gz', 'thick_interp_t1ce.nii.gz',
                                                  'thick_t1ce.json', 'through_plane_t1ce.json', 'through_plane_thick_interp_t1ce.json']
    assert runs['bytes']('interp') == runs['bytes']('th')
    got = runs['vol'](tmp / 'interp' / 'thick_interp_t1ce.nii.gz')
    from mudiff_hip import volume as V
    k = np.moveaxis(np.asarray(V.normalise_volume(np.asarray(runs['vol'](runs['p']['K']), np.float64)), np.float32).astype(np.float64), 2, 0)
    w32 = R.profile(L, 'gauss').astype(np.float32)
    starts = [a for a, b in SLABS[:3]]
    y = R.average(k, [list(range(a, a + L)) for a in starts], w32)
    want = np.clip(0.5 * R.interpolate(y, starts, L, Z) + 0.5, 0, 1)
    assert np.abs(np.moveaxis(got, 2, 0) - want).max() <= 1e-5
    both = [json.load(open(tmp / 'interp' / f)) for f in ('metrics_t1ce.json', 'metrics_thick_interp_t1ce.json')]
    assert both[0].keys() == both[1].keys()
    both = [json.load(open(tmp / 'interp' / f)) for f in ('through_plane_t1ce.json', 'through_plane_thick_interp_t1ce.json')]
    assert both[0].keys() == both[1].keys()
    assert '[thick-interp] ' in runs['log']['interp']


def test_with_the_flags_the_bytes_are_those_of_the_separate_code_paths(runs):
    """The three modes share one constraint path (mudiff_hip.constraints): the runs with the flags write the bytes, and report the
    residuals, that the commit before it wrote (recorded there: tests/golden/constraint_parent_payloads.json)."""
    import hashlib
    from conftest import REPO
    with open(os.path.join(REPO, 'tests', 'golden', 'constraint_parent_payloads.json')) as f:
        recorded = json.load(f)['thick']
    for job, suffix in (('th', ''), ('ens', ''), ('ens', '_std')):
        got = VS.payload(str(runs['tmp'] / job / f'predicted_t1ce{suffix}.nii.gz'))
        assert hashlib.sha256(got).hexdigest() == recorded[job + suffix], job + suffix
    for job in ('th', 'ens'):
        assert runs['report'](job)['max_residual'] == recorded[job + '_max_residual'], job
