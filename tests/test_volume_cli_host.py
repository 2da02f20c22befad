"""Host: the volume pipeline's command line, whose input-stage flags live in the stage modules (volume_prepare.STAGES: each module's
add_flags and options_from).  The order of the options, that a default is the same whether it comes from the parser or from a namespace
that lacks the flag, and that every stage's refusals still leave through the parser's error."""
import argparse

import pytest

MINIMAL = ['--target_modality', 'T1CE', '--output_dir', 'o', '--exp', 'e']
SWITCHES = ['regrid', 'coregister', 'bias_correct', 'denoise', 'foreground', 'brain_extract', 'reorient', 'conform']

OPTIONS = '''
-h --help --input_t1ce --input_t1 --input_t2 --input_flair --target_modality --output_dir --exp --output_path --slice_half_range --image_size --seed
--num_channels --num_channels_dae --n_mlp --ch_mult --num_res_blocks --attn_resolutions --dropout --resamp_with_conv --conditional --fir --fir_kernel
--skip_rescale --resblock_type --progressive --progressive_input --progressive_combine --embedding_type --fourier_scale --not_use_tanh --centered --nz
--z_emb_dim --t_emb_dim --num_timesteps --use_geometric --beta_min --beta_max --use_bf16 --gpu_chose --batch_size --resize_back --num_samples
--gt_volume --eval_mask --device_intake --norm --regrid --regrid_interp --coregister --coregister_strides --coregister_max_mm --coregister_max_deg
--bias_correct --bias_shrink --bias_levels --bias_iters --bias_tol --bias_bins --bias_fwhm --bias_wiener --bias_field_out --denoise --denoise_sigma
--denoise_search --denoise_patch --denoise_beta --denoise_rician --foreground --foreground_bins --foreground_open --foreground_keep_holes
--foreground_mask_out --brain_extract --brain_from --brain_erode_mm --brain_dilate_mm --brain_bins --brain_keep_holes --brain_mask_out --reorient
--reorient_to --reorient_back --conform --conform_shape --conform_spacing --conform_to --conform_back --antialias --calibrate --calibrate_threshold
--prec_plan
'''.split()
COHORT_OPTIONS = ['--manifest', '--brats_root', '--subjects', '--score', '--io_threads']


def _options(parser):
    return [o for action in parser._actions for o in action.option_strings]


def test_parser_order(monkeypatch):
    from mudiff_hip import cohort, volume as V
    p = V.make_parser()
    assert len(p._actions) == 93 and _options(p) == OPTIONS
    seen = []
    finish = V.finish_args
    monkeypatch.setattr(V, 'finish_args', lambda parser, args: (seen.append(parser), finish(parser, args))[1])
    cohort.build_argparser(MINIMAL + ['--manifest', 'm.tsv'])
    assert _options(seen[0]) == OPTIONS + COHORT_OPTIONS


def test_defaults_agree():
    """Every default is written once: a namespace that only carries the eight switches gives the options the parser's defaults give."""
    from mudiff_hip import volume as V
    from mudiff_hip.volume_prepare import IntakeOptions
    bare = IntakeOptions.from_args(argparse.Namespace(**{s: True for s in SWITCHES}))
    parsed = IntakeOptions.from_args(V.build_argparser(MINIMAL + ['--' + s for s in SWITCHES]))
    assert bare == parsed
    assert None not in (parsed.coreg, parsed.bias, parsed.denoise, parsed.foreground, parsed.brain, parsed.reorient, parsed.conform) and parsed.regrid
    assert IntakeOptions.from_args(V.build_argparser(MINIMAL)) == IntakeOptions()
    assert IntakeOptions.from_args(argparse.Namespace()) == IntakeOptions()


# per stage: a bad value, and where the stage has one the flag that needs the stage's switch -> the flag the message names
REFUSALS = [
    (['--regrid', '--regrid_interp', 'sinc'], 'regrid_interp'),
    (['--coregister', '--coregister_strides', '0'], 'coregister_strides'),
    (['--bias_correct', '--bias_levels', '6'], 'bias_levels'), (['--bias_field_out'], 'bias_field_out'),
    (['--denoise', '--denoise_search', '6'], 'denoise_search'),
    (['--foreground', '--foreground_bins', '15'], 'foreground_bins'),
    (['--brain_extract', '--brain_dilate_mm', '4'], 'brain_dilate_mm'),
    (['--reorient', '--reorient_to', 'LLS'], 'reorient_to'), (['--reorient_back'], 'reorient_back'),
    (['--conform', '--conform_shape', '24', '0', '16'], 'conform_shape'), (['--conform_back'], 'conform_back'),
    (['--conform', '--conform_to', 'RAS', '--reorient', '--reorient_to', 'LPS'], 'conform_to'),          # the one cross-stage check
]


@pytest.mark.parametrize('bad, word', REFUSALS, ids=[w for _, w in REFUSALS])
def test_refusals_leave_through_the_parser(bad, word, capsys):
    from mudiff_hip import cohort, volume as V
    for build in (lambda: V.build_argparser(MINIMAL + bad), lambda: cohort.build_argparser(MINIMAL + ['--manifest', 'm.tsv'] + bad)):
        with pytest.raises(SystemExit) as e:
            build()
        assert e.value.code == 2 and word in capsys.readouterr().err
