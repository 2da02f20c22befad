"""Register / spill / LDS / occupancy table of every kernel of one unit (default: every k_conv_mfma instantiation), from hipcc's
kernel-resource-usage remarks (no GPU needed), compiled with the flags csrc/Makefile gives that unit:
    python scripts/kernel_resources.py [file.hip] [extra hipcc flags]"""
import re, subprocess, sys, os, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'mu-diff_amd', 'csrc')
src = sys.argv[1] if len(sys.argv) > 1 else os.path.join(CSRC, 'conv_mfma.hip')


def from_makefile(what):
    return subprocess.check_output(['make', '-C', CSRC, '-s', '--no-print-directory', 'print-' + what], text=True).split()


unit = os.path.splitext(os.path.basename(src))[0]
with tempfile.TemporaryDirectory(prefix='mud_kres_') as tmp:      # the object is not wanted, only the remarks
    p = subprocess.run([*from_makefile('hipcc'), *from_makefile('flags-' + unit), '-Wno-pass-failed', f'-I{CSRC}', '-Rpass-analysis=kernel-resource-usage',
                        *sys.argv[2:], '-c', src, '-o', os.path.join(tmp, unit + '.o')], stderr=subprocess.PIPE, text=True)
t = p.stderr
if p.returncode:
    sys.exit(t[-3000:])
for b in re.split(r'remark: Function Name: ', t)[1:]:
    name = b.split()[0].strip()
    g = lambda k: re.search(k + r': (\d+)', b).group(1)       # noqa: E731
    m = re.search(r'k_conv_mfmaILi(\d)ELi(\d)ELi(\d)ELi(\d)ELi(\d)ELb(\d)ELi(\d)E', name)
    tag = ('KS%s MT%s WM%s WN%s PRO%s DUAL%s PREC%s' % m.groups()) if m else name[:48]
    print('%-48s VGPR %4s AGPR %4s spill %4s scratch %5s occ %s LDS %s' % (tag, g(' VGPRs'), g('AGPRs'), g('VGPRs Spill'), g(r'ScratchSize \[bytes/lane\]'),
                                                                         g(r'Occupancy \[waves/SIMD\]'), g(r'LDS Size \[bytes/block\]')))
