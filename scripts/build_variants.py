"""Builds experiment variants of libmudiff_hip.so (conv_mfma.hip compiled with extra flags) for in-process A/B runs
(scripts/ab_conv.py).  Output: mu-diff_amd/mudiff_hip/variants/lib_<name>.so (git-ignored).  A variant reports its flags through
mud_build_flags(), and mudiff_hip.load() refuses it unless MUDIFF_ALLOW_VARIANT=1.
    python scripts/build_variants.py name1:-DSOME_KNOB=1 name2:"-DA=1 -DB=2" ...
The compiler, the object list and every unit's flags are csrc/Makefile's (its print-* targets): a variant is the shipped library with
one object replaced.  Experiments that no longer ship live in scripts/experiments, which is on the include path:
    python scripts/build_variants.py ws:-DMUD_EXPERIMENT_WS          # conv_ws.inc, the warp-specialised 3x3 kernel
(`name:@path/to/edited_conv_mfma.hip[:flags]` compiles that file instead of csrc/conv_mfma.hip.)"""
import os, subprocess, sys, tempfile
from concurrent.futures import ThreadPoolExecutor
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'mu-diff_amd', 'csrc')
EXPERIMENTS = os.path.join(ROOT, 'scripts', 'experiments')
OUT = os.path.join(ROOT, 'mu-diff_amd', 'mudiff_hip', 'variants')
UNIT = 'conv_mfma'


def from_makefile(what):
    return subprocess.check_output(['make', '-C', CSRC, '-s', '--no-print-directory', 'print-' + what], text=True).split()


os.makedirs(OUT, exist_ok=True)
subprocess.check_call(['make', '-C', CSRC, '-j8'], stdout=subprocess.DEVNULL)
HIPCC, = from_makefile('hipcc')
ARCH = [f for f in from_makefile('flags-' + UNIT) if f.startswith('--offload-arch=')]
objs = [os.path.join(CSRC, o) for o in from_makefile('objs') if o not in (UNIT + '.o', 'api.o')]
TMPDIR = tempfile.TemporaryDirectory(prefix='mud_variants_')        # the variants' own objects: removed when the script ends
TMP = TMPDIR.name


def build(spec):
    name, _, flags = spec.partition(':')
    src = os.path.join(CSRC, UNIT + '.hip')
    if flags.startswith('@'):
        path, _, flags = flags[1:].partition(':')
        src = os.path.abspath(path)
    obj, api = os.path.join(TMP, f'conv_{name}.o'), os.path.join(TMP, f'api_{name}.o')
    subprocess.check_call([HIPCC, *from_makefile('flags-' + UNIT), '-Wno-pass-failed', f'-I{CSRC}', f'-I{EXPERIMENTS}', *flags.split(), '-c', src, '-o', obj])
    tag = (os.path.basename(src) + ' ' + flags).strip().replace('"', '')
    subprocess.check_call([HIPCC, *from_makefile('flags-api'), f'-DMUD_BUILD_FLAGS="{name}: {tag}"', '-c', os.path.join(CSRC, 'api.cpp'), '-o', api])
    lib = os.path.join(OUT, f'lib_{name}.so')
    subprocess.check_call([HIPCC, *ARCH, '-shared', '-fPIC', *objs, api, obj, '-o', lib])
    return lib


with ThreadPoolExecutor(4) as ex:
    for lib in ex.map(build, sys.argv[1:]):
        print('built', lib)
