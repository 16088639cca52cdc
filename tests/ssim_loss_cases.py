"""fp64 NumPy reference of the SSIM gradient (ops.ssim_bwd, QF.ssim_index) and the case lists of its tests.

ref_ssim_grad scatters every valid position's three derivative maps over the taps x taps pixels of its window, one
(i, j) offset at a time: a direct sum that shares no structure with the kernel, which gathers per pixel in a
horizontal and a vertical pass.  It also returns the magnitude sum the tolerance is stated in,
    mag(q) = |g[n]| / (C oh ow) * sum_ij w_i w_j (|P| + 2 |x(q) Q| + |y(q) R|)(q - (i,j)).
The keyword arguments of ref_ssim_grad are the MUTANTS tests/test_ssim_loss_host.py shows the tolerance to reject.

Tolerance, per element (the issue's): |da - dx_ref| <= 2^-23 |dx_ref| + 1e-9 mag.  The first term is the one fp32
rounding of the result with an ulp of slack, the second the fp64 roundings of two summation orders through
1 / (B1 B2) (two fp64 orderings were measured <= 3.5e-12 mag apart)."""
import functools

import numpy as np

import recon_metric_cases as R

ASYM_WINDOW = (0.05, 0.1, 0.15, 0.3, 0.4)
REL, MAG = 2.0 ** -23, 1e-9


def window(name):
    return {"gauss11": R.gaussian_window(), "uniform7": R.uniform_window(7), "asym5": np.array(ASYM_WINDOW),
            "one": np.array([1.0]), "gauss15": R.gaussian_window(15, 2.0)}[name]


def ref_maps(x, y, win, c1=R.C1, c2=R.C2, dtype=np.float64):
    """(S, P, Q, R), each (N,C,oh,ow) fp64: the score of every valid position and its derivatives with respect to
    sum w x, sum w x^2 and sum w x y.  dtype=np.float32 keeps the five window moments in fp32 (a mutant)."""
    x, y = np.asarray(x, dtype), np.asarray(y, dtype)
    win = np.asarray(win, np.float64)
    taps = len(win)
    N, C, H, W = x.shape
    oh, ow = H - taps + 1, W - taps + 1
    mx, my, xx, yy, xy = (np.zeros((N, C, oh, ow), dtype) for _ in range(5))
    for i in range(taps):
        for j in range(taps):
            w = dtype(win[i] * win[j])
            u, v = x[:, :, i:i + oh, j:j + ow], y[:, :, i:i + oh, j:j + ow]
            mx += w * u
            my += w * v
            xx += w * (u * u)
            yy += w * (v * v)
            xy += w * (u * v)
    mx, my, xx, yy, xy = (m.astype(np.float64) for m in (mx, my, xx, yy, xy))
    if dtype is np.float32:      # the subtractions of the fp32 formula round too
        f = np.float32
        vx, vy, cov = (f(xx) - f(mx) * f(mx)).astype(np.float64), (f(yy) - f(my) * f(my)).astype(np.float64), \
            (f(xy) - f(mx) * f(my)).astype(np.float64)
    else:
        vx, vy, cov = xx - mx * mx, yy - my * my, xy - mx * my
    a1, a2 = 2 * mx * my + c1, 2 * cov + c2
    b1, b2 = mx * mx + my * my + c1, vx + vy + c2
    s = a1 * a2 / (b1 * b2)
    p = 2 * my * (a2 - a1) / (b1 * b2) - 2 * mx * s * (1 / b1 - 1 / b2)
    return s, p, -s / b2, 2 * a1 / (b1 * b2)


def ref_ssim_grad(x, y, win, g, c1=R.C1, c2=R.C2, moments=np.float64, maps=np.float64, flipped=False,
                  drop_last_row=False, g_per_batch=False):
    """(dx, mag), both (N,C,H,W) fp64: the gradient of sum_n g[n] ssim(x, y)[n] with respect to x, and the
    magnitude sum of its terms.  The keywords are mutants: fp32 moments, maps rounded to fp32, the window applied
    flipped in the backward, the last row of valid positions dropped, one g for the whole batch."""
    win = np.asarray(win, np.float64)
    taps = len(win)
    x64, y64 = np.asarray(x, np.float64), np.asarray(y, np.float64)
    N, C, H, W = x64.shape
    oh, ow = H - taps + 1, W - taps + 1
    _, p, q, r = ref_maps(x, y, win, c1, c2, moments)
    if maps is np.float32:
        p, q, r = (m.astype(np.float32).astype(np.float64) for m in (p, q, r))
    if drop_last_row:
        p, q, r = (m.copy() for m in (p, q, r))
        for m in (p, q, r):
            m[:, :, oh - 1, :] = 0.0
    wb = win[::-1] if flipped else win
    dx, mag = np.zeros((N, C, H, W)), np.zeros((N, C, H, W))
    for i in range(taps):
        for j in range(taps):
            w = wb[i] * wb[j]
            u, v = x64[:, :, i:i + oh, j:j + ow], y64[:, :, i:i + oh, j:j + ow]
            dx[:, :, i:i + oh, j:j + ow] += w * (p + 2 * u * q + v * r)
            mag[:, :, i:i + oh, j:j + ow] += w * (np.abs(p) + 2 * np.abs(u * q) + np.abs(v * r))
    g = np.asarray(g, np.float64)
    if g_per_batch:
        g = np.full(N, g.mean())
    scale = (g / (C * oh * ow)).reshape(N, 1, 1, 1)
    return dx * scale, mag * np.abs(scale)


def excess(da, dx, mag):
    """How far each element is from the reference in units of mag, after the fp32-rounding allowance:
    (|da - dx| - 2^-23 |dx|) / mag, at least 0; the tolerance holds where this is <= 1e-9.  Elements whose mag is
    0 (g[n] = 0) must be exact: inf where they are not."""
    da, dx, mag = (np.asarray(v, np.float64) for v in (da, dx, mag))
    over = np.maximum(np.abs(da - dx) - REL * np.abs(dx), 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.where(mag > 0, over / mag, np.where(over > 0, np.inf, 0.0))
    return np.where(np.isnan(da) | np.isnan(dx), np.inf, e)


def within(da, dx, mag):
    return bool((excess(da, dx, mag) <= MAG).all())


# (C, H, W) under the 11-tap Gaussian: one valid position; one row of them; an input tile edge and one pixel past
# it; an output tile edge (16 positions) and one past it, each way; one past two input tiles; ragged
BWD_SHAPES = ((1, 11, 11), (1, 11, 40), (1, 16, 17), (3, 26, 27), (3, 27, 26), (2, 32, 33), (3, 43, 59))
BWD_BATCHES = (1, 3)
# name -> (window name, N, C, H, W): 7 uniform taps; the asymmetric window (correlation order shows); a single tap
# (the maps pass straight through); 15 taps at one row of positions (the largest halo)
WINDOW_CASES = {"uniform7": ("uniform7", *R.SSIM_UNIFORM_CASE[:4]), "asym5": ("asym5", 2, 2, 20, 37),
                "one": ("one", 2, 3, 17, 18), "gauss15": ("gauss15", 2, 1, 15, 31)}
G_VALUES = (-0.75, 3.0, 1e-3, -40.0, 0.3)      # mixed signs and magnitudes; the first N of them


def g_for(N):
    return np.array(G_VALUES[:N], np.float64)


@functools.lru_cache(maxsize=None)
def case(family, wname, N, C, H, W):
    """(x, y, g, dx, mag) of one test case, computed once and shared read-only between the tests that use it."""
    seed = 1000 + 97 * R.FAMILIES.index(family) + 13 * N + C + 7 * H + 3 * W
    x, y = R.make_pair(family, (N, C, H, W), seed=seed)
    g = g_for(N)
    dx, mag = ref_ssim_grad(x, y, window(wname), g)
    for v in (x, y, g, dx, mag):
        v.setflags(write=False)
    return x, y, g, dx, mag


def torch_ssim(pred, target, win, c1=R.C1, c2=R.C2):
    """(N,) mean SSIM in torch (the dtype of pred), differentiable: the window moments through conv2d with groups."""
    import torch
    import torch.nn.functional as F
    C = pred.shape[1]
    w1 = torch.as_tensor(np.asarray(win, np.float64), dtype=pred.dtype)
    k = (w1[:, None] * w1[None, :])[None, None].repeat(C, 1, 1, 1)

    def blur(v):
        return F.conv2d(v, k, groups=C)

    mx, my = blur(pred), blur(target)
    xx, yy, xy = blur(pred * pred), blur(target * target), blur(pred * target)
    s = ((2 * mx * my + c1) * (2 * (xy - mx * my) + c2)) / ((mx * mx + my * my + c1) * ((xx - mx * mx) + (yy - my * my) + c2))
    return s.flatten(1).mean(1)
