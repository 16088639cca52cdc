"""Generation evaluation (additive; the reference has none): the Frechet distance between two sample sets, with the
autoencoder's latent -- what the cascade models -- as the feature space instead of an Inception network.

A sample's feature vector is its latent, or its decoded image, mean-pooled over pool x pool blocks (ops.pool_features,
fp64).  Per set the count, the sum and the Gram matrix of the features, taken about one shift shared by all sets,
stay on the device in fp64 (ops.moments_add: fp64 MFMA, one fixed order, no atomics) and are read back once, in
result().  Means, covariances and the distance itself are host arithmetic in fp64 NumPy.

THE NUMBER IS NOT FID.  It is comparable only between runs that share the autoencoder (and, in image space, the
decoder), the pool and the space; the results carry a note saying so."""
import numpy as np
import torch

from . import ops

TILE = 16       # moments_add maintains the upper triangle of TILE x TILE tiles of the Gram matrix
MAX_DIM = 1024
NOTE = ("Frechet distance between pooled autoencoder features -- NOT FID: no Inception network is involved, and "
        "values are comparable only between runs that share the autoencoder, the feature pool and the space.")


def mirror_triangle(gram):
    """The full symmetric matrix from one whose upper triangle of TILE x TILE tiles (diagonal tiles whole) is
    maintained: every element below that triangle is replaced by its transpose."""
    g = np.asarray(gram, dtype=np.float64)
    t = np.arange(g.shape[0]) // TILE
    return np.where(t[None, :] < t[:, None], g.T, g)


def moments_to_mean_cov(count, total, gram, shift=None):
    """(mean, cov) from the shifted one-pass moments: mean = shift + sum / n, cov = (gram - sum sum^T / n) / (n - 1)
    with gram already symmetric.  fp64 NumPy."""
    n = int(count)
    if n < 2:
        raise ValueError(f"a covariance needs at least 2 samples, got {n}")
    total = np.asarray(total, dtype=np.float64)
    mean = total / n if shift is None else np.asarray(shift, dtype=np.float64) + total / n
    cov = (np.asarray(gram, dtype=np.float64) - np.outer(total, total) / n) / (n - 1)
    return mean, cov


class FeatureMoments:
    """count / sum / Gram matrix of feature rows about `shift` (a (dim,) fp64 device tensor or None), kept on the
    device.  The three accumulators and a copy of the shift share one buffer so that result() is one read-back."""

    def __init__(self, dim, shift=None):
        dim = int(dim)
        if not 1 <= dim <= MAX_DIM:
            raise ValueError(f"FeatureMoments: dim {dim} outside 1 ... {MAX_DIM}")
        if shift is not None and (shift.dtype != torch.float64 or tuple(shift.shape) != (dim,)):
            raise ValueError(f"FeatureMoments: shift must be ({dim},) fp64, got {tuple(shift.shape)} {shift.dtype}")
        self.dim = dim
        self.shift = None if shift is None else shift.contiguous()
        self._buf = None

    def _state(self, device):
        D = self.dim
        if self._buf is None:
            self._buf = torch.zeros(D * D + 2 * D + 1, dtype=torch.float64, device=device)
            if self.shift is not None:
                self._buf[D * D + D:D * D + 2 * D].copy_(self.shift)
        b = self._buf
        return b[D * D + 2 * D:].view(torch.int64), b[D * D:D * D + D], b[:D * D].view(D, D)

    def add(self, features):
        """Adds the rows of features (n, dim) fp64 on the device; nothing is read back."""
        if features.dim() != 2 or features.shape[1] != self.dim:
            raise ValueError(f"FeatureMoments.add: features of shape {tuple(features.shape)}, dim is {self.dim}")
        ops.moments_add(features, self._state(features.device), self.shift)

    def read(self):
        """The one read-back: (count, sum, mirrored gram, shift) as NumPy / int, before any division."""
        D = self.dim
        if self._buf is None:
            return 0, np.zeros(D), np.zeros((D, D)), None
        host = self._buf.cpu().numpy()
        shift = None if self.shift is None else host[D * D + D:D * D + 2 * D]
        count = int(host[D * D + 2 * D:].view(np.int64)[0])
        return count, host[D * D:D * D + D], mirror_triangle(host[:D * D].reshape(D, D)), shift

    def result(self):
        """{"count", "mean", "cov"} (NumPy fp64) from one read-back; raises for fewer than 2 samples."""
        count, total, gram, shift = self.read()
        mean, cov = moments_to_mean_cov(count, total, gram, shift)
        return {"count": count, "mean": mean, "cov": cov}


def _psd_sqrt(c):
    """(c^1/2, sum of the negative eigenvalues that were clipped to 0) of a symmetric matrix."""
    w, v = np.linalg.eigh((c + c.T) / 2.0)
    clipped = float(w[w < 0].sum())
    return (v * np.sqrt(np.clip(w, 0.0, None))) @ v.T, clipped


def frechet_distance(m1, c1, m2, c2):
    """|m1 - m2|^2 + tr(c1 + c2 - 2 (c1^1/2 c2 c1^1/2)^1/2) between two Gaussians, fp64 NumPy, two symmetric
    eigendecompositions: tr (c1^1/2 c2 c1^1/2)^1/2 is the sum of the square roots of that product's eigenvalues.
    Negative eigenvalues (rounding, rank deficiency) are clipped to 0 and their sum is reported."""
    m1, m2 = np.asarray(m1, dtype=np.float64), np.asarray(m2, dtype=np.float64)
    c1, c2 = np.asarray(c1, dtype=np.float64), np.asarray(c2, dtype=np.float64)
    if m1.shape != m2.shape or c1.shape != c2.shape or c1.shape != (m1.size, m1.size):
        raise ValueError(f"frechet_distance: shapes {m1.shape}, {c1.shape}, {m2.shape}, {c2.shape}")
    d = m1 - m2
    mean_term = float(d @ d)
    s1, clip1 = _psd_sqrt(c1)
    m = s1 @ c2 @ s1
    w = np.linalg.eigvalsh((m + m.T) / 2.0)
    clip2 = float(w[w < 0].sum())
    cov_term = float(np.trace(c1) + np.trace(c2) - 2.0 * np.sqrt(np.clip(w, 0.0, None)).sum())
    return {"fd": mean_term + cov_term, "mean_term": mean_term, "cov_term": cov_term, "clipped": clip1 + clip2}


class GenerationScorer:
    """Moments of the sets `real`, `real_a` / `real_b` (alternate real samples), `generated` and, with a codebook,
    `quantised` (the hard-quantised real latents), all about one shift -- the mean feature of the first real batch --
    so that the sets' means are differences of comparable sums."""
    SETS = ("real", "real_a", "real_b", "quantised", "generated")

    def __init__(self, pool, space="latent", decoder=None, hr_codebook=None):
        if space not in ("latent", "image"):
            raise ValueError(f"GenerationScorer: space must be 'latent' or 'image', got {space!r}")
        if space == "image" and decoder is None:
            raise ValueError("GenerationScorer: the image space needs a decoder")
        if int(pool) < 1:
            raise ValueError(f"GenerationScorer: pool must be positive, got {pool}")
        self.pool, self.space, self.decoder, self.hr_codebook = int(pool), space, decoder, hr_codebook
        self.dim = None
        self.shift = None
        self._sets = {}
        self._seen_real = 0

    @torch.no_grad()
    def features(self, z):
        """(N, D) fp64 features of a latent batch (N,C,H,W) on the device."""
        if self.space == "image":
            mode = self.decoder.training
            self.decoder.eval()
            try:
                z = self.decoder(z)
            finally:
                self.decoder.train(mode)
        return ops.pool_features(z, self.pool)

    def _add(self, name, f):
        if f.shape[0] == 0:
            return
        m = self._sets.get(name)
        if m is None:
            m = self._sets[name] = FeatureMoments(self.dim, self.shift)
        m.add(f)

    @torch.no_grad()
    def add(self, z, which="real"):
        """Adds one batch of latents to the real sets or to the generated set; nothing is read back."""
        if which not in ("real", "generated"):
            raise ValueError(f"GenerationScorer.add: which must be 'real' or 'generated', got {which!r}")
        f = self.features(z)
        if self.dim is None:
            if which != "real":
                raise RuntimeError("GenerationScorer: add a real batch first (its mean feature is every set's shift)")
            self.dim = f.shape[1]
            self.shift = f.mean(dim=0)       # any fixed vector near the data would do: it cancels in mean and cov
        elif f.shape[1] != self.dim:
            raise ValueError(f"GenerationScorer: {f.shape[1]} features per sample after {self.dim}")
        if which == "generated":
            self._add("generated", f)
            return
        self._add("real", f)
        first = self._seen_real & 1          # parity of this batch's first sample among all real samples
        self._add("real_a", f[first::2])
        self._add("real_b", f[1 - first::2])
        self._seen_real += f.shape[0]
        if self.hr_codebook is not None:
            mode = self.hr_codebook.training
            self.hr_codebook.eval()
            try:
                zq = self.hr_codebook(z, use_gaussian=False)
            finally:
                self.hr_codebook.train(mode)
            self._add("quantised", self.features(zq))

    def result(self):
        """One read-back per set.  Every distance is a frechet_distance dict; a pair with a set of fewer than 2
        samples is left out."""
        if self.dim is None:
            raise RuntimeError("GenerationScorer.result: no batch was added")
        if self.hr_codebook is not None:
            ops.check_index_flag(self.shift.device, "generation evaluation")
        stats = {}
        counts = {name: 0 for name in self.SETS if name != "quantised" or self.hr_codebook is not None}
        for name, m in self._sets.items():
            count, total, gram, shift = m.read()
            counts[name] = count
            if count >= 2:
                mean, cov = moments_to_mean_cov(count, total, gram, shift)
                stats[name] = {"mean": mean, "cov": cov}
        r = {"counts": counts, "dim": self.dim, "pool": self.pool, "space": self.space, "note": NOTE}
        for key, a, b in (("fd_real_generated", "real", "generated"),
                          ("fd_quantised_generated", "quantised", "generated"),
                          ("fd_real_quantised", "real", "quantised"), ("fd_real_split", "real_a", "real_b")):
            if a in stats and b in stats:
                r[key] = frechet_distance(stats[a]["mean"], stats[a]["cov"], stats[b]["mean"], stats[b]["cov"])
        return r


def summary_line(tag, result):
    parts = []
    for key in ("fd_real_generated", "fd_quantised_generated", "fd_real_quantised", "fd_real_split"):
        if key in result:
            parts.append("{}: {:.6g}".format(key[3:], result[key]["fd"]))
    return "{} latent-space Frechet distance (not FID) | {} | D: {} | {}".format(
        tag, " | ".join(parts), result["dim"], " ".join(f"{k}={v}" for k, v in result["counts"].items()))
