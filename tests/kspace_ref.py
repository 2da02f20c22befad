"""fp64 numpy restatement of the k-space path (csrc/kspace.hip, mudiff_hip.kspace): the unitary transform, the
measurement y = M_eff * F(k), the data-consistency step of mud_kspace_constrain and the mask builders.  Nothing here imports the
package."""
import numpy as np


def fft2(x, inverse=False):
    """Unitary 2D DFT of [..., S, S] in fp64 / complex128, DC at [0, 0]."""
    x = np.asarray(x)
    x = x.astype(np.complex128 if np.iscomplexobj(x) else np.float64)
    return np.fft.ifft2(x, norm='ortho') if inverse else np.fft.fft2(x, norm='ortho')


def rule(S):
    """The relative L2 error a radix FFT of an S x S slice may have in fp32 with correctly rounded twiddles: 8 * log2(S^2) * 2^-24
    (Higham, Accuracy and Stability of Numerical Algorithms, ch. 24, constant rounded up)."""
    return 8.0 * np.log2(float(S) ** 2) * 2.0 ** -24


def symmetrise(mask):
    """M_eff[u, v] = M[u, v] | M[-u mod S, -v mod S]."""
    m = np.asarray(mask) != 0
    S = m.shape[-1]
    idx = (-np.arange(S)) % S
    return (m | m[..., idx, :][..., :, idx]).astype(np.uint8)


def measure(k, mask):
    """y = mask * F(k) for real k [rows, S, S] and a 0/1 mask [1 or rows, S, S]."""
    return np.where(np.asarray(mask) != 0, fft2(k), 0.0)


def constrain(x_new, y, mask, eta, t, toff, a_tab, s_tab, clean):
    """out = x_new - Re F^H[ mask ? F(x_new - s * eta) - a * y : 0 ] per slice, c = clamp(t + toff, 0, ntab - 1); clean: s = 0, a = 1.
    All in fp64 from the fp32 operands."""
    x_new = np.asarray(x_new, np.float64)
    rows = x_new.shape[0]
    if clean:
        a, s = np.ones(rows), np.zeros(rows)
        d = x_new
    else:
        c = np.clip(np.asarray(t, np.int64) + int(toff), 0, len(a_tab) - 1)
        a, s = np.asarray(a_tab, np.float64)[c], np.asarray(s_tab, np.float64)[c]
        d = x_new - s[:, None, None] * np.asarray(eta, np.float64)
    r = np.where(np.asarray(mask) != 0, fft2(d) - a[:, None, None] * np.asarray(y, np.complex128), 0.0)
    return x_new - fft2(r, inverse=True).real


# ---- mask builders (centred line patterns as fastMRI draws them, then an ifftshift into the kernel's order) ----------------------------
def center_lines(S, fraction):
    n = int(round(S * float(fraction)))
    lines = np.zeros(S, bool)
    pad = (S - n + 1) // 2
    lines[pad:pad + n] = True
    return lines


def lines_of(mask, axis):
    """The measured phase-encode lines of a line mask in kernel order, centred again: bool [S]."""
    m = np.fft.fftshift(np.asarray(mask) != 0)
    full = m.all(axis=1 - axis)
    assert np.array_equal(m, np.broadcast_to(full[:, None] if axis == 0 else full[None, :], m.shape)), 'not a line mask'
    return full
