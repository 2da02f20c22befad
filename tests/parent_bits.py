"""The bits of the constraint and keyed-draw kernels, recorded on the commit before they moved onto csrc/keyed_rows.h
(tests/golden/constraint_kernel_parent_bits.json, written by tests/golden/make_constraint_kernel_bits.py).  Every module in MODULES has
a generator `parent_bit_cases()` of (name, tensor) pairs, built from its own case functions, and one test that hands it to `check`; the
recorder runs the same generators, so the two cannot drift.  A test never writes the fixture."""
import hashlib
import json
import os

import torch

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'constraint_kernel_parent_bits.json')
MODULES = ('test_known_region_gpu', 'test_kspace_gpu', 'test_thick_gpu', 'test_ensemble_gpu', 'test_slice_coupling_gpu', 'test_gpu_parity')
NTAB = 5
ROW_LENS = (1, 3, 4, 5, 8, 4099)       # a ragged quad alone, one whole quad, a whole quad and a tail, two whole quads, a long odd row
ROWS = (1, 5, 37)


def level_t(rows, toff):
    """Row levels whose first two entries make both clamps act: 0 (toff -1 -> below the table) and NTAB - 1 (toff +1 -> past it); a
    single row takes the end toff pushes it over."""
    if rows == 1:
        return torch.tensor([NTAB - 1 if toff > 0 else 0])
    return torch.tensor([(0, NTAB - 1, 2, 1, 3)[r % 5] for r in range(rows)])


def off_by_one_float(t):
    """A contiguous copy of t that starts 4 bytes off a 16-byte boundary: the [1:] view of a flat buffer."""
    buf = torch.empty(t.numel() + 1, device=t.device, dtype=t.dtype)
    assert buf.data_ptr() % 16 == 0
    v = buf[1:].view(t.shape)
    v.copy_(t)
    return v


def digest(t):
    t = torch.view_as_real(t) if t.is_complex() else t
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def digests(cases):
    out = {}
    for name, t in cases:
        assert name not in out, name
        out[name] = digest(t)
    return out


def check(module, cases):
    with open(FIXTURE) as f:
        recorded = json.load(f)['digests'][module]
    got = digests(cases)
    assert sorted(got) == sorted(recorded), sorted(set(got) ^ set(recorded))
    differ = [n for n in got if got[n] != recorded[n]]
    print(f'{module}: {len(got)} outputs, {len(differ)} differ from the parent commit')
    assert not differ, differ
