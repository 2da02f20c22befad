"""Host: every refusal of the flag parsers of the known-target modes, word for word (known_region, kspace, thick, multislice and
thick_volume: options_from).  One row per `raise` of those functions and of the range parsers they call, and rows with two faults at
once, which pin the order of the checks: the order decides which message a doubly bad command line gets.  DESIGN.md section 5.24a."""
import argparse
import importlib

import pytest

KV = dict(known_volume='k.nii.gz')
KS = dict(KV, known_kspace='equispaced')
TH = dict(KV, known_thick=3)
MS = dict(KV, known_multislice='equispaced', multislice_thick=3)
TV = dict(known_thick_volume='y.nii.gz')
PATTERNS = "('equispaced', 'random', 'lowres', 'file')"
PROFILES = "('box', 'gauss')"
TV_WHY = ': Y is the measurement itself, on its own grid (--known_volume and the modes on it measure a thin target retrospectively)'
MS_WHY = ' (it is both at once: its own --multislice_* flags say how thick and how accelerated)'

REFUSALS = [
    # --known_volume
    ('known_region', dict(known_mask='m.nii.gz'), '--known_mask needs --known_volume'),
    ('known_region', dict(known_drop_slices=['1:2']), '--known_drop_slices needs --known_volume'),
    ('known_region', dict(known_resample=2), '--known_resample needs --known_volume'),
    ('known_region', dict(KV, known_resample=0), '--known_resample must be an integer >= 1, got 0'),
    ('known_region', dict(KV, known_resample=1.5), '--known_resample must be an integer >= 1, got 1.5'),
    ('known_region', dict(KV, seed=-1), '--known_volume needs a --seed in [0, 2^64) (its draws are keyed)'),
    ('known_region', dict(KV, seed=1 << 64), '--known_volume needs a --seed in [0, 2^64) (its draws are keyed)'),
    ('known_region', dict(KV, known_drop_slices=['3:1']), "--known_drop_slices takes ranges A:B of slices with 0 <= A <= B, got '3:1'"),
    ('known_region', dict(KV, known_drop_slices=['a:b']), "--known_drop_slices takes ranges A:B of slices with 0 <= A <= B, got 'a:b'"),
    ('known_region', dict(KV, known_drop_slices=['4']), "--known_drop_slices takes ranges A:B of slices with 0 <= A <= B, got '4'"),
    # two faults: the first dependent flag named, the value before the seed, the seed before the ranges
    ('known_region', dict(known_mask='m.nii.gz', known_drop_slices=['1:2']), '--known_mask needs --known_volume'),
    ('known_region', dict(KV, known_resample=0, seed=-1), '--known_resample must be an integer >= 1, got 0'),
    ('known_region', dict(KV, seed=-1, known_drop_slices=['3:1']), '--known_volume needs a --seed in [0, 2^64) (its draws are keyed)'),

    # --known_kspace
    ('kspace', dict(kspace_accel=2), '--kspace_accel needs --known_kspace'),
    ('kspace', dict(kspace_center=0.1), '--kspace_center needs --known_kspace'),
    ('kspace', dict(kspace_axis=1), '--kspace_axis needs --known_kspace'),
    ('kspace', dict(kspace_mask_file='m.npy'), '--kspace_mask_file needs --known_kspace'),
    ('kspace', dict(kspace_zero_filled=True), '--kspace_zero_filled needs --known_kspace'),
    ('kspace', dict(KV, known_kspace='spiral'), f"--known_kspace must be one of {PATTERNS}, got 'spiral'"),
    ('kspace', dict(known_kspace='equispaced'), '--known_kspace needs --known_volume'),
    ('kspace', dict(KS, known_mask='m.nii.gz'), '--known_kspace cannot be combined with --known_mask (a voxel mask has no meaning in k-space; '
                                                 'use --known_drop_slices for slices that were not measured)'),
    ('kspace', dict(KS, image_size=96), '--known_kspace needs an --image_size that is a power of two in [16, 512], got 96'),
    ('kspace', dict(KS, kspace_accel=0), '--kspace_accel must be an integer >= 1, got 0'),
    ('kspace', dict(KS, kspace_accel=2.5), '--kspace_accel must be an integer >= 1, got 2.5'),
    ('kspace', dict(KS, kspace_center=1.5), '--kspace_center must lie in [0, 1], got 1.5'),
    ('kspace', dict(KS, kspace_mask_file='m.npy'), '--kspace_mask_file goes with --known_kspace file, and that pattern needs it'),
    ('kspace', dict(KV, known_kspace='file'), '--kspace_mask_file goes with --known_kspace file, and that pattern needs it'),
    ('kspace', dict(KS, seed=-1), '--known_kspace needs a --seed in [0, 2^64) (its draws are keyed)'),
    # two faults
    ('kspace', dict(known_kspace='equispaced', known_mask='m.nii.gz'), '--known_kspace needs --known_volume'),
    ('kspace', dict(KS, kspace_accel=0, kspace_center=1.5), '--kspace_accel must be an integer >= 1, got 0'),
    ('kspace', dict(KS, known_mask='m.nii.gz', image_size=96), '--known_kspace cannot be combined with --known_mask (a voxel mask has no meaning '
                                                                'in k-space; use --known_drop_slices for slices that were not measured)'),
    ('kspace', dict(KS, image_size=96, kspace_accel=0), '--known_kspace needs an --image_size that is a power of two in [16, 512], got 96'),
    ('kspace', dict(KS, kspace_center=-0.5, kspace_mask_file='m.npy'), '--kspace_center must lie in [0, 1], got -0.5'),
    ('kspace', dict(KS, kspace_mask_file='m.npy', seed=-1), '--kspace_mask_file goes with --known_kspace file, and that pattern needs it'),
    ('kspace', dict(known_kspace='spiral', kspace_accel=0), f"--known_kspace must be one of {PATTERNS}, got 'spiral'"),

    # --known_thick
    ('thick', dict(thick_gap=1), '--thick_gap needs --known_thick'),
    ('thick', dict(thick_offset=1), '--thick_offset needs --known_thick'),
    ('thick', dict(thick_profile='gauss'), '--thick_profile needs --known_thick'),
    ('thick', dict(thick_interp=True), '--thick_interp needs --known_thick'),
    ('thick', dict(KV, known_thick=0), '--known_thick must be an integer in [1, 16] (thin slices per slab), got 0'),
    ('thick', dict(KV, known_thick=17), '--known_thick must be an integer in [1, 16] (thin slices per slab), got 17'),
    ('thick', dict(KV, known_thick=2.5), '--known_thick must be an integer in [1, 16] (thin slices per slab), got 2.5'),
    ('thick', dict(known_thick=3), '--known_thick needs --known_volume'),
    ('thick', dict(TH, known_kspace='equispaced'), '--known_thick cannot be combined with --known_kspace (in-plane undersampling of thick slices '
                                                   'is out of scope)'),
    ('thick', dict(TH, known_mask='m.nii.gz'), '--known_thick cannot be combined with --known_mask (a thick slice is measured whole; use '
                                               '--known_drop_slices for thick slices that were not acquired)'),
    ('thick', dict(TH, thick_gap=-1), '--thick_gap must be an integer >= 0, got -1'),
    ('thick', dict(TH, thick_offset=-2), '--thick_offset must be an integer >= 0, got -2'),
    ('thick', dict(TH, thick_offset=0.5), '--thick_offset must be an integer >= 0, got 0.5'),
    ('thick', dict(TH, thick_profile='sinc'), f"--thick_profile must be one of {PROFILES}, got 'sinc'"),
    ('thick', dict(TH, seed=1 << 64), '--known_thick needs a --seed in [0, 2^64) (its draws are keyed)'),
    # two faults
    ('thick', dict(KV, known_thick=0, thick_gap=-1), '--known_thick must be an integer in [1, 16] (thin slices per slab), got 0'),
    ('thick', dict(known_thick=0), '--known_thick must be an integer in [1, 16] (thin slices per slab), got 0'),
    ('thick', dict(known_thick=3, known_mask='m.nii.gz'), '--known_thick needs --known_volume'),
    ('thick', dict(known_thick=3, thick_gap=-1), '--known_thick needs --known_volume'),
    ('thick', dict(TH, known_kspace='equispaced', known_mask='m.nii.gz'), '--known_thick cannot be combined with --known_kspace (in-plane '
                                                                          'undersampling of thick slices is out of scope)'),
    ('thick', dict(TH, known_mask='m.nii.gz', thick_gap=-1), '--known_thick cannot be combined with --known_mask (a thick slice is measured '
                                                             'whole; use --known_drop_slices for thick slices that were not acquired)'),
    ('thick', dict(TH, thick_gap=-1, thick_offset=-2), '--thick_gap must be an integer >= 0, got -1'),
    ('thick', dict(TH, thick_offset=-2, thick_profile='sinc'), '--thick_offset must be an integer >= 0, got -2'),
    ('thick', dict(TH, thick_profile='sinc', seed=-1), f"--thick_profile must be one of {PROFILES}, got 'sinc'"),

    # --known_multislice
    ('multislice', dict(multislice_thick=3), '--multislice_thick needs --known_multislice'),
    ('multislice', dict(multislice_gap=1), '--multislice_gap needs --known_multislice'),
    ('multislice', dict(multislice_offset=1), '--multislice_offset needs --known_multislice'),
    ('multislice', dict(multislice_profile='box'), '--multislice_profile needs --known_multislice'),
    ('multislice', dict(multislice_accel=2), '--multislice_accel needs --known_multislice'),
    ('multislice', dict(multislice_center=0.1), '--multislice_center needs --known_multislice'),
    ('multislice', dict(multislice_axis=0), '--multislice_axis needs --known_multislice'),
    ('multislice', dict(multislice_mask_file='m.npy'), '--multislice_mask_file needs --known_multislice'),
    ('multislice', dict(multislice_baseline=True), '--multislice_baseline needs --known_multislice'),
    ('multislice', dict(MS, known_multislice='spiral'), f"--known_multislice must be one of {PATTERNS}, got 'spiral'"),
    ('multislice', dict(known_multislice='equispaced', multislice_thick=3), '--known_multislice needs --known_volume'),
    ('multislice', dict(MS, known_mask='m.nii.gz'), '--known_multislice cannot be combined with --known_mask (a thick slice is measured in '
                                                    'k-space; use --known_drop_slices for thick slices that were not acquired)'),
    ('multislice', dict(MS, known_kspace='random'), '--known_multislice cannot be combined with --known_kspace' + MS_WHY),
    ('multislice', dict(MS, known_thick=3), '--known_multislice cannot be combined with --known_thick' + MS_WHY),
    ('multislice', dict(KV, known_multislice='equispaced'), '--known_multislice needs --multislice_thick L (thin slices per thick slice)'),
    ('multislice', dict(MS, multislice_thick=0), '--multislice_thick must be an integer in [1, 16] (thin slices per slab), got 0'),
    ('multislice', dict(MS, multislice_thick=17), '--multislice_thick must be an integer in [1, 16] (thin slices per slab), got 17'),
    ('multislice', dict(MS, image_size=100), '--known_multislice needs an --image_size that is a power of two in [16, 512], got 100'),
    ('multislice', dict(MS, multislice_gap=-1), '--multislice_gap must be an integer >= 0, got -1'),
    ('multislice', dict(MS, multislice_gap=1.5), '--multislice_gap must be an integer >= 0, got 1.5'),
    ('multislice', dict(MS, multislice_offset=-1), '--multislice_offset must be an integer >= 0, got -1'),
    ('multislice', dict(MS, multislice_profile='sinc'), f"--multislice_profile must be one of {PROFILES}, got 'sinc'"),
    ('multislice', dict(MS, multislice_accel=0), '--multislice_accel must be an integer >= 1, got 0'),
    ('multislice', dict(MS, multislice_center=2), '--multislice_center must lie in [0, 1], got 2.0'),
    ('multislice', dict(MS, multislice_axis=2), '--multislice_axis must be 0 or 1, got 2'),
    ('multislice', dict(MS, multislice_mask_file='m.npy'), '--multislice_mask_file goes with --known_multislice file, and that pattern needs it'),
    ('multislice', dict(MS, known_multislice='file'), '--multislice_mask_file goes with --known_multislice file, and that pattern needs it'),
    ('multislice', dict(MS, seed=-1), '--known_multislice needs a --seed in [0, 2^64) (its draws and its mask are keyed)'),
    # two faults
    ('multislice', dict(MS, multislice_thick=0, multislice_gap=-1), '--multislice_thick must be an integer in [1, 16] (thin slices per slab), got 0'),
    ('multislice', dict(known_multislice='equispaced', multislice_thick=3, known_mask='m.nii.gz'), '--known_multislice needs --known_volume'),
    ('multislice', dict(MS, multislice_accel=0, multislice_center=2), '--multislice_accel must be an integer >= 1, got 0'),
    ('multislice', dict(known_multislice='spiral'), f"--known_multislice must be one of {PATTERNS}, got 'spiral'"),
    ('multislice', dict(MS, known_mask='m.nii.gz', known_kspace='random'), '--known_multislice cannot be combined with --known_mask (a thick slice '
                                                                           'is measured in k-space; use --known_drop_slices for thick slices '
                                                                           'that were not acquired)'),
    ('multislice', dict(MS, known_kspace='random', known_thick=3), '--known_multislice cannot be combined with --known_kspace' + MS_WHY),
    ('multislice', dict(KV, known_multislice='equispaced', known_thick=3), '--known_multislice cannot be combined with --known_thick' + MS_WHY),
    ('multislice', dict(KV, known_multislice='equispaced', image_size=100), '--known_multislice needs --multislice_thick L (thin slices per thick '
                                                                            'slice)'),
    ('multislice', dict(MS, multislice_thick=0, image_size=100), '--multislice_thick must be an integer in [1, 16] (thin slices per slab), got 0'),
    ('multislice', dict(MS, image_size=100, multislice_gap=-1), '--known_multislice needs an --image_size that is a power of two in [16, 512], '
                                                                'got 100'),
    ('multislice', dict(MS, multislice_gap=-1, multislice_offset=-1), '--multislice_gap must be an integer >= 0, got -1'),
    ('multislice', dict(MS, multislice_offset=-1, multislice_profile='sinc'), '--multislice_offset must be an integer >= 0, got -1'),
    ('multislice', dict(MS, multislice_profile='sinc', multislice_accel=0), f"--multislice_profile must be one of {PROFILES}, got 'sinc'"),
    ('multislice', dict(MS, multislice_center=2, multislice_axis=2), '--multislice_center must lie in [0, 1], got 2.0'),
    ('multislice', dict(MS, multislice_axis=2, multislice_mask_file='m.npy'), '--multislice_axis must be 0 or 1, got 2'),
    ('multislice', dict(MS, multislice_mask_file='m.npy', seed=-1), '--multislice_mask_file goes with --known_multislice file, and that pattern '
                                                                    'needs it'),

    # --known_thick_volume
    ('thick_volume', dict(thick_volume_thickness_mm=5.0), '--thick_volume_thickness_mm needs --known_thick_volume'),
    ('thick_volume', dict(thick_volume_profile='box'), '--thick_volume_profile needs --known_thick_volume'),
    ('thick_volume', dict(thick_volume_drop=['1:2']), '--thick_volume_drop needs --known_thick_volume'),
    ('thick_volume', dict(thick_volume_baseline=True), '--thick_volume_baseline needs --known_thick_volume'),
    ('thick_volume', dict(TV, known_volume='k.nii.gz'), '--known_thick_volume cannot be combined with --known_volume' + TV_WHY),
    ('thick_volume', dict(TV, known_kspace='random'), '--known_thick_volume cannot be combined with --known_kspace' + TV_WHY),
    ('thick_volume', dict(TV, known_thick=3), '--known_thick_volume cannot be combined with --known_thick' + TV_WHY),
    ('thick_volume', dict(TV, known_multislice='random'), '--known_thick_volume cannot be combined with --known_multislice' + TV_WHY),
    ('thick_volume', dict(TV, known_mask='m.nii.gz'), '--known_thick_volume cannot be combined with --known_mask' + TV_WHY),
    ('thick_volume', dict(TV, known_drop_slices=['1:2']), '--known_thick_volume cannot be combined with --known_drop_slices' + TV_WHY),
    ('thick_volume', dict(known_thick_volume='manifest'), "--known_thick_volume manifest needs a cohort (--manifest): it takes each subject's file "
                                                          'from the `known` column'),
    ('thick_volume', dict(TV, thick_volume_thickness_mm=0.0), '--thick_volume_thickness_mm must be a positive number of millimetres, got 0.0'),
    ('thick_volume', dict(TV, thick_volume_thickness_mm=float('inf')), '--thick_volume_thickness_mm must be a positive number of millimetres, got inf'),
    ('thick_volume', dict(TV, thick_volume_profile='sinc'), f"--thick_volume_profile must be one of {PROFILES}, got 'sinc'"),
    ('thick_volume', dict(TV, known_resample=0), '--known_resample must be an integer >= 1, got 0'),
    ('thick_volume', dict(TV, seed=-1), '--known_thick_volume needs a --seed in [0, 2^64) (its draws are keyed)'),
    ('thick_volume', dict(TV, thick_volume_drop=['2:1']), "--thick_volume_drop takes ranges A:B of thick slices with 0 <= A <= B, got '2:1'"),
    ('thick_volume', dict(TV, thick_volume_drop=['x']), "--thick_volume_drop takes ranges A:B of thick slices with 0 <= A <= B, got 'x'"),
    # two faults
    ('thick_volume', dict(TV, known_volume='k.nii.gz', known_mask='m.nii.gz'), '--known_thick_volume cannot be combined with --known_volume' + TV_WHY),
    ('thick_volume', dict(known_thick_volume='manifest', known_thick=3), '--known_thick_volume cannot be combined with --known_thick' + TV_WHY),
    ('thick_volume', dict(known_thick_volume='manifest', thick_volume_thickness_mm=-1.0), "--known_thick_volume manifest needs a cohort "
                                                                                          "(--manifest): it takes each subject's file from the "
                                                                                          '`known` column'),
    ('thick_volume', dict(TV, thick_volume_thickness_mm=-1.0, thick_volume_profile='sinc'), '--thick_volume_thickness_mm must be a positive number '
                                                                                            'of millimetres, got -1.0'),
    ('thick_volume', dict(TV, thick_volume_profile='sinc', known_resample=0), f"--thick_volume_profile must be one of {PROFILES}, got 'sinc'"),
    ('thick_volume', dict(TV, known_resample=0, seed=-1), '--known_resample must be an integer >= 1, got 0'),
    ('thick_volume', dict(TV, seed=-1, thick_volume_drop=['2:1']), '--known_thick_volume needs a --seed in [0, 2^64) (its draws are keyed)'),
]


@pytest.mark.parametrize('module,fields,message', REFUSALS, ids=[f'{m}-{i}' for i, (m, _, _) in enumerate(REFUSALS)])
def test_the_refusal_keeps_its_words_and_its_place(module, fields, message):
    options_from = importlib.import_module('mudiff_hip.' + module).options_from
    with pytest.raises(ValueError) as e:
        options_from(argparse.Namespace(**fields))
    assert str(e.value) == message


ACCEPTED = [
    # a cohort needs no --known_volume: its K is the manifest's `known` column
    ('kspace', dict(known_kspace='lowres', manifest='m.csv'), dict(pattern='lowres', accel=4, center=0.08, axis=0, mask_file=None, zero_filled=False)),
    ('thick', dict(known_thick=4, brats_root='/data'), dict(L=4, gap=0, offset=0, profile='box', interp=False)),
    ('multislice', dict(known_multislice='random', multislice_thick=2, manifest='m.csv'),
     dict(pattern='random', L=2, gap=0, offset=0, profile='box', accel=4, center=0.08, axis=0, mask_file=None, baseline=False)),
    ('known_region', dict(known_mask='m.nii.gz', manifest='m.csv'), None),
    ('known_region', dict(known_resample=3, known_thick_volume='y.nii.gz'), None),
    ('thick_volume', dict(known_thick_volume='manifest', manifest='m.csv', known_resample=None),
     dict(volume='manifest', thickness=None, profile='box', drop=[], baseline=False, resample=1)),
    # every value given, at the edge of what is taken
    ('kspace', dict(KV, known_kspace='file', kspace_mask_file='m.npy', kspace_accel=1, kspace_center=1, kspace_axis=1, kspace_zero_filled=True,
                    image_size=512, seed=(1 << 64) - 1), dict(pattern='file', accel=1, center=1.0, axis=1, mask_file='m.npy', zero_filled=True)),
    ('thick', dict(KV, known_thick=16, thick_gap=0, thick_offset=7, thick_profile='gauss', thick_interp=True, seed=0),
     dict(L=16, gap=0, offset=7, profile='gauss', interp=True)),
    ('multislice', dict(KV, known_multislice='file', multislice_thick=1, multislice_gap=2, multislice_offset=3, multislice_profile='gauss',
                        multislice_accel=1, multislice_center=0, multislice_axis=1, multislice_mask_file='m.npy', multislice_baseline=True,
                        image_size=16),
     dict(pattern='file', L=1, gap=2, offset=3, profile='gauss', accel=1, center=0.0, axis=1, mask_file='m.npy', baseline=True)),
    ('known_region', dict(KV, known_mask='m.nii.gz', known_drop_slices=['0:0', '4:9'], known_resample=2),
     dict(volume='k.nii.gz', mask='m.nii.gz', drop=[(0, 0), (4, 9)], resample=2)),
    ('thick_volume', dict(TV, thick_volume_thickness_mm=5, thick_volume_profile='gauss', thick_volume_drop=['1:1'], thick_volume_baseline=True,
                          known_resample=2), dict(volume='y.nii.gz', thickness=5.0, profile='gauss', drop=[(1, 1)], baseline=True, resample=2)),
]


@pytest.mark.parametrize('module,fields,want', ACCEPTED, ids=[f'{m}-{i}' for i, (m, _, _) in enumerate(ACCEPTED)])
def test_what_is_taken_stays_taken(module, fields, want):
    got = importlib.import_module('mudiff_hip.' + module).options_from(argparse.Namespace(**fields))
    assert got == want and (want is None or list(got) == list(want))
