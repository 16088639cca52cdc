"""fp64 NumPy references and the case lists of the reconstruction-metric tests (ops.pair_error, ops.ssim).

ref_ssim is a direct taps x taps window sum (121 terms at 11 taps), not separable: it shares no structure with
the kernel, which runs a horizontal and a vertical pass.  ref_pair_error sums exactly (math.fsum).  All inputs
are fp32 with |x| <= 1, data_range 2."""
import math

import numpy as np

DATA_RANGE = 2.0
C1 = (0.01 * DATA_RANGE) ** 2
C2 = (0.03 * DATA_RANGE) ** 2
SSIM_TOL = 1e-10        # derivation: tests/test_gpu_recon_metrics.py
PE_CHUNK = 4096         # csrc/recon.hip: elements of one image per workgroup of the chunk kernel
PE_TRIP = 1024          # ... of which the 256 threads take 4 each per trip


def gaussian_window(taps=11, sigma=1.5):
    w = np.exp(-((np.arange(taps) - taps // 2) ** 2) / (2.0 * sigma * sigma))
    return w / w.sum()


def uniform_window(taps):
    return np.full(taps, 1.0 / taps)


def ref_ssim(a, b, win, c1=C1, c2=C2, dtype=np.float64):
    """Per-image mean SSIM of (N,C,H,W) arrays over the valid positions.  dtype=np.float32 is the mutant that
    keeps the window moments in fp32: it must FAIL the GPU tolerance where the moments cancel."""
    a, b = np.asarray(a, dtype), np.asarray(b, dtype)
    win = np.asarray(win, np.float64)
    taps = len(win)
    N, C, H, W = a.shape
    oh, ow = H - taps + 1, W - taps + 1
    mx, my, xx, yy, xy = (np.zeros((N, C, oh, ow), dtype) for _ in range(5))
    for dy in range(taps):
        for dx in range(taps):
            w = dtype(win[dy] * win[dx])
            x, y = a[:, :, dy:dy + oh, dx:dx + ow], b[:, :, dy:dy + oh, dx:dx + ow]
            mx += w * x
            my += w * y
            xx += w * (x * x)
            yy += w * (y * y)
            xy += w * (x * y)
    c1, c2 = dtype(c1), dtype(c2)
    m = ((2 * mx * my + c1) * (2 * (xy - mx * my) + c2)) / \
        ((mx * mx + my * my + c1) * ((xx - mx * mx) + (yy - my * my) + c2))
    return m.astype(np.float64).reshape(N, -1).mean(axis=1)


def ref_ssim_separable(a, b, win, c1=C1, c2=C2):
    """The same formula with a horizontal and a vertical fp64 pass: a second ordering of the sums."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    taps = len(win)
    N, C, H, W = a.shape
    oh, ow = H - taps + 1, W - taps + 1

    def blur(v):
        h = sum(win[k] * v[:, :, :, k:k + ow] for k in range(taps))
        return sum(win[k] * h[:, :, k:k + oh, :] for k in range(taps))

    mx, my, xx, yy, xy = blur(a), blur(b), blur(a * a), blur(b * b), blur(a * b)
    m = ((2 * mx * my + c1) * (2 * (xy - mx * my) + c2)) / \
        ((mx * mx + my * my + c1) * ((xx - mx * mx) + (yy - my * my) + c2))
    return m.reshape(N, -1).mean(axis=1)


def ref_pair_error(a, b):
    """(N,3) fp64 {sum d^2, sum |d|, max |d|} per image; each term rounded once, the sums exact."""
    a = np.asarray(a, np.float64).reshape(len(a), -1)
    b = np.asarray(b, np.float64).reshape(len(b), -1)
    out = np.empty((len(a), 3))
    for n in range(len(a)):
        d = a[n] - b[n]
        ad = np.abs(d)
        out[n] = (math.fsum(d * d), math.fsum(ad), ad.max()) if np.isfinite(d).all() else \
            ((d * d).sum(), ad.sum(), ad.max())
    return out


def pair_error_close(got, want, E):
    """The two sums within E 2^-52 relative (non-negative terms, each rounded once), the maximum equal."""
    got, want = np.asarray(got), np.asarray(want)
    ok = np.abs(got[:, :2] - want[:, :2]) <= E * 2.0 ** -52 * np.abs(want[:, :2])
    return bool(ok.all()) and np.array_equal(got[:, 2], want[:, 2])


# ("negated", x against -x, flips the sign of the mean term and of the structure term at once: its scores are
#  positive, about 0.7; "anticorrelated" is the family whose scores are negative)
FAMILIES = ("noise", "negated", "anticorrelated", "near_constant", "constants", "identical")


def make_pair(family, shape, seed):
    """Two fp32 arrays of `shape`, |x| <= 1."""
    rng = np.random.default_rng(seed)
    if family == "noise":
        x = np.tanh(rng.standard_normal(shape))
        y = np.clip(x + 0.1 * rng.standard_normal(shape), -1.0, 1.0)
    elif family == "negated":
        x = np.tanh(rng.standard_normal(shape))
        y = -x
    elif family == "anticorrelated":          # the same mean, the structure inverted: negative scores
        g = np.tanh(rng.standard_normal(shape))
        x, y = 0.5 + 0.4 * g, 0.5 - 0.4 * g
    elif family == "near_constant":
        x = 0.9 + 0.001 * rng.uniform(-1.0, 1.0, shape)
        y = 0.9 + 0.001 * rng.uniform(-1.0, 1.0, shape)
    elif family == "constants":
        x, y = np.full(shape, 0.25), np.full(shape, -0.5)
    elif family == "identical":
        x = np.tanh(rng.standard_normal(shape))
        y = x.copy()
    else:
        raise KeyError(family)
    return x.astype(np.float32), y.astype(np.float32)


# (C, H, W): one output; one row of outputs; one output past a 16-tile in each direction; ragged; four full tiles
SSIM_SHAPES = ((1, 11, 11), (1, 11, 40), (3, 26, 27), (3, 27, 26), (3, 43, 59), (4, 64, 64))
SSIM_BATCHES = (1, 3)
SSIM_UNIFORM_CASE = (2, 3, 26, 23, 7)      # N, C, H, W, taps: uniform weights


def one_pixel_positions(H, W, taps=11):
    """Pixels whose change must show: the image's corners, and the pixels under the first and the last output of
    the last (partial) 16 x 16 tile of outputs."""
    oh, ow = H - taps + 1, W - taps + 1
    ty, tx = 16 * ((oh - 1) // 16), 16 * ((ow - 1) // 16)
    return sorted({(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (oh - 1, ow - 1), (ty, tx), (oh - 1, tx),
                   (ty, ow - 1), (ty + taps - 1, tx + taps - 1)})


def _edges(*at):
    return [e + d for e in at for d in (-1, 0, 1)]


# elements per image: small and wave-sized, then one below, at and above every edge of the kernel's partition --
# a thread's 4, a trip of 1,024, the chunk of 4,096 and its multiples
PAIR_SIZES = sorted({1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1027, *_edges(PE_TRIP, 2 * PE_TRIP, 3 * PE_TRIP,
                                                                            PE_CHUNK, 2 * PE_CHUNK, 3 * PE_CHUNK)})
PAIR_BATCHES = (1, 2, 5)
