"""Record tests/golden/constraint_kernel_parent_bits.json: the SHA-256 of every output of the `parent_bit_cases()` generators of the
modules tests/parent_bits.py lists, computed on a build of the commit BEFORE the constraint and keyed-draw kernels moved onto
csrc/keyed_rows.h.  Needs a GPU.  Build that commit's csrc/ with its own Makefile in a scratch copy and point the loader at it:

    MUDIFF_HIP_LIB=<scratch>/mu-diff_amd/mudiff_hip/libmudiff_hip.so MUDIFF_ALLOW_VARIANT=1 \\
        python tests/golden/make_constraint_kernel_bits.py --commit <hash of that commit>

Every generator runs twice; an output whose digest differs between the two runs is reported and left out (the kernels are fixed
functions of their inputs, so none is expected).  --check compares the library in use against the fixture and writes nothing."""
import argparse
import importlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
REPO = os.path.dirname(TESTS)
sys.path[:0] = [TESTS, REPO, os.path.join(REPO, 'mu-diff_amd')]

import parent_bits as P      # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--commit', help='hash of the commit the library in use was built from')
    ap.add_argument('--out', default=P.FIXTURE)
    ap.add_argument('--check', action='store_true', help='compare with the fixture, write nothing')
    a = ap.parse_args()
    import mudiff_hip
    print('library:', mudiff_hip.lib_path())
    mudiff_hip.load()
    if a.check:
        for name in P.MODULES:
            P.check(name, importlib.import_module(name).parent_bit_cases())
        return
    if not a.commit:
        ap.error('--commit is required to record')
    out, unstable = {}, []
    for name in P.MODULES:
        cases = importlib.import_module(name).parent_bit_cases
        first, second = P.digests(cases()), P.digests(cases())
        unstable += [f'{name}: {n}' for n in first if first[n] != second[n]]
        out[name] = {n: d for n, d in first.items() if d == second[n]}
        print(f'{name}: {len(out[name])} outputs')
    print('digests that differ between two runs of the same library:', unstable or 'none')
    with open(a.out, 'w') as f:
        json.dump(dict(commit=a.commit, unstable=unstable, digests=out), f, indent=0, sort_keys=True)
        f.write('\n')
    print('wrote', a.out, os.path.getsize(a.out), 'bytes')


if __name__ == '__main__':
    main()
