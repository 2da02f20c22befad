"""numpy restatement of --unring: removal of truncation (Gibbs) ringing by local sub-voxel shifts (Kellner et al.
2016), as the definition in DESIGN.md states it - not as the kernels compute it.  Everything is fp64 by default; dtype=np.float32 rounds
the tables and every intermediate to fp32 and is the yardstick for the rounding error an fp32 implementation may show (its sums run in
numpy's order, not the device's: it is no bit-for-bit model).

    shifts(N)                       s_0 = 0, s_j = +j/K (1 <= j <= N), s_j = -(j - N)/K (N < j <= 2N), K = 2N + 1
    shift_table(n, N)               D[j, r]: the real circulant that samples a band-limited n-line at l + s_j
    unring_lines(x, N, a, b)        U along the last axis of x[..., n] -> (out, jmap, TV[K, ..., n])
    split(vol, axes)                Ix, Iy = the directional filter pair of every slice, Ix + Iy = I as computed
    unring(vol, axes, N, a, b)      the whole stage on values [X, Y, Z] -> dict(out, ix, iy, jx, jy, tvx, tvy, nonfinite)
"""
import numpy as np

DEFAULTS = dict(axes=(0, 1), shifts=20, window=(1, 3))


def shifts(N):
    K = 2 * N + 1
    return np.array([0.0] + [j / K for j in range(1, N + 1)] + [-(j - N) / K for j in range(N + 1, 2 * N + 1)])


def signed_frequencies(n):
    """The signed frequencies of an n-point transform in np.fft's order; n/2 (not -n/2) for the Nyquist bin of an even n."""
    k = np.fft.fftfreq(n, 1.0 / n).round().astype(np.int64)
    return np.where(2 * k == -n, n // 2, k)


def shift_table(n, N, dtype=np.float64):
    """D[j, r] = (1/n) sum_k phi_{s_j}(k) exp(2 pi i k r / n): phi_s(k) = exp(2 pi i s k / n) for |k| < n/2, cos(pi s) at k = n/2."""
    k = signed_frequencies(n)
    D = np.empty((2 * N + 1, n))
    for j, s in enumerate(shifts(N)):
        phi = np.exp(2j * np.pi * s * k / n)
        if n % 2 == 0:
            phi[n // 2] = np.cos(np.pi * s)
        D[j] = np.fft.ifft(phi).real
    return D.astype(dtype)


def circulant(d):
    """C[l, m] = d[(l - m) mod n]: y = C @ x is the circular convolution of x with d."""
    n = d.shape[0]
    l, m = np.meshgrid(np.arange(n), np.arange(n), indexing='ij')
    return d[(l - m) % n]


def unring_lines(x, N=20, a=1, b=3, dtype=np.float64, sign=1.0):
    """U of the definition along the last axis -> (out, jmap int8, TV [2N + 1, ...]).  sign=-1 re-interpolates the wrong way (the check
    that tells a sign slip)."""
    x = np.asarray(x, dtype)
    n = x.shape[-1]
    assert 2 * b + 2 <= n and 1 <= a <= b
    D = shift_table(n, N, dtype)
    TV, cands = np.empty((2 * N + 1,) + x.shape, dtype), np.empty((2 * N + 1,) + x.shape, dtype)
    for j, s in enumerate(shifts(N)):
        y = x if j == 0 else (x @ circulant(D[j]).T).astype(dtype)
        d = np.abs(y - np.roll(y, 1, -1))                              # d[l] = |y[l] - y[l-1]|
        tvl, tvr = np.zeros_like(y), np.zeros_like(y)
        for t in range(a, b + 1):
            tvl = (tvl + np.roll(d, t, -1)).astype(dtype)              # d[l - t]
            tvr = (tvr + np.roll(d, -(t + 1), -1)).astype(dtype)       # d[l + t + 1]
        TV[j] = np.minimum(tvl, tvr)
        if j == 0:
            cands[0] = x
            continue
        s = dtype(s * sign)
        toward = np.roll(y, 1, -1) if s > 0 else np.roll(y, -1, -1)    # a0 = y[l-1] for s > 0, a2 = y[l+1] for s < 0
        cands[j] = (y + (abs(s) * (toward - y)).astype(dtype)).astype(dtype)
    jmap = choose(TV)
    return np.take_along_axis(cands, jmap[None].astype(np.int64), 0)[0], jmap, TV


def choose(TV):
    """j*: the first j, scanning upwards with a strict <, of the smallest TV[j]: a tie keeps the earlier shift, an all-equal score j = 0."""
    TV = np.asarray(TV)
    best, jmap = TV[0].copy(), np.zeros(TV.shape[1:], np.int8)
    for j in range(1, TV.shape[0]):
        better = TV[j] < best
        best, jmap = np.where(better, TV[j], best), np.where(better, np.int8(j), jmap)
    return jmap


def direction_filter(nx, ny):
    """Gx[kx, ky] = cy / (cx + cy), cx = 1 + cos(2 pi kx / nx), cy = 1 + cos(2 pi ky / ny); 1/2 at the one bin where both are 0."""
    cx = 1.0 + np.cos(2 * np.pi * np.arange(nx) / nx)[:, None]
    cy = 1.0 + np.cos(2 * np.pi * np.arange(ny) / ny)[None, :]
    corner = nx % 2 == 0 and ny % 2 == 0
    den = cx + cy
    if corner:
        den[nx // 2, ny // 2] = 1.0
    G = cy / den
    if corner:
        G[nx // 2, ny // 2] = 0.5
    return G


def _dft_matrix(n, dtype):
    kl = (np.arange(n)[:, None] * np.arange(n)[None, :]) % n
    return np.exp(-2j * np.pi * kl / n).astype(np.complex64 if dtype == np.float32 else np.complex128)


def split(vol, axes=(0, 1), dtype=np.float64):
    """-> (Ix, Iy): Ix = every slice circularly filtered by Gx along (axes[0], axes[1]), Iy = I - Ix."""
    vol = np.asarray(vol, dtype)
    ax, ay = axes
    nx, ny = vol.shape[ax], vol.shape[ay]
    G = direction_filter(nx, ny)
    moved = np.moveaxis(vol, (ax, ay), (0, 1))
    if dtype == np.float32:                                            # dense fp32 transforms, as an fp32 implementation has them
        Wx, Wy = _dft_matrix(nx, dtype), _dft_matrix(ny, dtype)
        F = np.einsum('kx,xy...->ky...', Wx, moved.astype(np.complex64)).astype(np.complex64)
        F = np.einsum('qy,ky...->kq...', Wy, F).astype(np.complex64)
        F = (F * G.astype(np.float32).reshape(G.shape + (1,) * (moved.ndim - 2))).astype(np.complex64)
        F = np.einsum('yq,kq...->ky...', Wy.conj(), F).astype(np.complex64)
        ix = (np.einsum('xk,ky...->xy...', Wx.conj(), F).real / np.float32(nx * ny)).astype(np.float32)
    else:
        F = np.fft.fftn(moved, axes=(0, 1))
        ix = np.fft.ifftn(F * G.reshape(G.shape + (1,) * (moved.ndim - 2)), axes=(0, 1)).real
    ix = np.ascontiguousarray(np.moveaxis(ix, (0, 1), (ax, ay))).astype(dtype)
    return ix, (vol - ix).astype(dtype)


def unring(values, axes=(0, 1), shifts=20, window=(1, 3), dtype=np.float64, sign=1.0):
    """The stage on the values [X, Y, Z] of a volume (non-finite ones read as 0 and counted) -> dict: out, ix, iy, the maps jx, jy of the
    chosen shifts and tvx, tvy [2N + 1, X, Y, Z]."""
    values = np.asarray(values)
    bad = ~np.isfinite(values)
    vol = np.where(bad, 0, values).astype(dtype)
    ax, ay = axes
    ix, iy = split(vol, axes, dtype)
    a, b = window
    ux, jx, tvx = unring_lines(np.moveaxis(ix, ax, -1), shifts, a, b, dtype, sign)
    uy, jy, tvy = unring_lines(np.moveaxis(iy, ay, -1), shifts, a, b, dtype, sign)
    back = lambda v, axis: np.moveaxis(v, -1, axis if v.ndim == 3 else axis + 1)      # noqa: E731
    out = (back(ux, ax) + back(uy, ay)).astype(dtype)
    return dict(out=out, ix=ix, iy=iy, jx=back(jx, ax), jy=back(jy, ay), tvx=back(tvx, ax), tvy=back(tvy, ay), nonfinite=int(bad.sum()))


def counters(jmap, N):
    """(voxels with j* != 0, sum of |shift| in units of 1 / (2N + 1)) as the device counts them."""
    j = np.asarray(jmap).astype(np.int64)
    return int((j != 0).sum()), int(np.where(j > N, j - N, j).sum())


# ---------------------------------------------------------------------------------------------------
# the phantom of the recovery test: random ellipses rendered at 8x, truncated in k-space
# ---------------------------------------------------------------------------------------------------
def phantom(n, seed=0, over=8, ellipses=6):
    """-> (ringing n x n image: the over-sampled image's central n x n block of k-space transformed back; the box-averaged truth; mask of
    the pixels more than one pixel away from every edge of the truth)."""
    rng = np.random.default_rng(seed)
    m = n * over
    u = (np.arange(m) + 0.5) / m - 0.5
    xx, yy = np.meshgrid(u, u, indexing='ij')
    hi = np.zeros((m, m))
    for _ in range(ellipses):
        cx, cy = rng.uniform(-0.2, 0.2, 2)
        ra, rb = rng.uniform(0.08, 0.28, 2)
        th = rng.uniform(0, np.pi)
        xr, yr = (xx - cx) * np.cos(th) + (yy - cy) * np.sin(th), -(xx - cx) * np.sin(th) + (yy - cy) * np.cos(th)
        hi[(xr / ra) ** 2 + (yr / rb) ** 2 <= 1.0] += rng.uniform(0.2, 1.0)
    truth = hi.reshape(n, over, n, over).mean((1, 3))
    F = np.fft.fftshift(np.fft.fft2(hi))
    c = m // 2
    # the centre of the box average is half a fine pixel off the fine grid's origin: shift by (over - 1) / 2 fine pixels
    k = np.arange(-(n // 2), n - n // 2)
    ramp = np.exp(2j * np.pi * k * ((over - 1) / 2.0) / m)
    crop = F[c - n // 2:c - n // 2 + n, c - n // 2:c - n // 2 + n] * ramp[:, None] * ramp[None, :]
    ringing = np.fft.ifft2(np.fft.ifftshift(crop)).real / (over * over)
    edge = np.zeros((n, n), bool)
    for axis in (0, 1):
        step = np.abs(truth - np.roll(truth, 1, axis)) > 1e-9
        edge |= step | np.roll(step, -1, axis)
    near = edge.copy()
    for dx in (-1, 0, 1):
        for dy in (-1, 0, 1):
            near |= np.roll(np.roll(edge, dx, 0), dy, 1)
    return ringing, truth, ~near


def rms(a, b, mask):
    return float(np.sqrt(np.mean((a[mask] - b[mask]) ** 2)))


def cumsum_noise(shape, axes, seed):
    """The GPU tests' input: seeded standard-normal noise cumulated along the in-plane axes, fp64 [X, Y, Z]."""
    v = np.random.default_rng(seed).standard_normal(shape)
    for axis in axes:
        v = np.cumsum(v, axis)
    return v
