"""Generation evaluation (additive; the reference has none): the Frechet distance between two sample sets, with the
autoencoder's latent -- what the cascade models -- as the feature space instead of an Inception network.

A sample's feature vector is its latent, or its decoded image, mean-pooled over pool x pool blocks (ops.pool_features,
fp64).  Per set the count, the sum and the Gram matrix of the features, taken about one shift shared by all sets,
stay on the device in fp64 (ops.moments_add: fp64 MFMA, one fixed order, no atomics) and are read back once, in
result().  Means, covariances and the distance itself are host arithmetic in fp64 NumPy.

THE NUMBER IS NOT FID.  It is comparable only between runs that share the autoencoder (and, in image space, the
decoder), the pool and the space; the results carry a note saying so.

Optional (GenerationScorer(knn=k)): k-nearest-neighbour manifold statistics over the same features -- improved precision
and recall (Kynkaanniemi et al. 2019), density and coverage (Naeem et al. 2020) and every generated sample's distance to
its nearest real one.  The feature rows of a set stay on the device (FeatureBank); the squared distances, the k
smallest per row and the ball memberships come from ops.knn_smallest / ops.ball_count (fp64 MFMA, deterministic), and
only a handful of integers and quantiles are read back."""
import numpy as np
import torch

from . import ops

TILE = 16       # moments_add maintains the upper triangle of TILE x TILE tiles of the Gram matrix
MAX_DIM = 1024
NOTE = ("Frechet distance between pooled autoencoder features -- NOT FID: no Inception network is involved, and "
        "values are comparable only between runs that share the autoencoder, the feature pool and the space.")
MANIFOLD_NOTE = ("k-nearest-neighbour precision / recall / density / coverage over the same pooled features: the "
                 "values depend on k and on both sample counts and are comparable only between runs that share them "
                 "(and the autoencoder, the feature pool and the space); real_split is what two real samples of this "
                 "size reach.")
MAX_KNN = 8
KNN_MAX_SAMPLES = 16384          # default per-set cap of the feature banks
NN_QUANTILES = (("min", 0.0), ("q01", 0.01), ("q10", 0.10), ("q50", 0.50))


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


class FeatureBank:
    """The first `capacity` feature rows of a set, kept on the device in one (capacity, dim) fp64 buffer in the order
    they were added.  Rows past the capacity are counted (`dropped`) and ignored."""

    def __init__(self, dim, capacity):
        dim, capacity = int(dim), int(capacity)
        if not 1 <= dim <= MAX_DIM:
            raise ValueError(f"FeatureBank: dim {dim} outside 1 ... {MAX_DIM}")
        if not 1 <= capacity <= 1 << 20:
            raise ValueError(f"FeatureBank: capacity {capacity} outside 1 ... 2^20")
        self.dim, self.capacity = dim, capacity
        self.count = 0
        self.dropped = 0
        self._buf = None

    def add(self, features):
        """Copies the rows of features (n, dim) fp64 in, as far as there is room; nothing is read back."""
        if features.dim() != 2 or features.shape[1] != self.dim or features.dtype != torch.float64:
            raise ValueError(f"FeatureBank.add: features {tuple(features.shape)} {features.dtype}, need "
                             f"(n, {self.dim}) fp64")
        ops.require_cuda(features)
        if self._buf is None:
            self._buf = torch.empty((self.capacity, self.dim), dtype=torch.float64, device=features.device)
        take = min(features.shape[0], self.capacity - self.count)
        if take > 0:
            self._buf[self.count:self.count + take].copy_(features[:take])
        self.count += take
        self.dropped += features.shape[0] - take

    def rows(self):
        """(count, dim) fp64: a view of the rows held."""
        if self._buf is None:
            raise ValueError("FeatureBank.rows: no row was added")
        return self._buf[:self.count]


def _rows(s):
    return s.rows() if isinstance(s, FeatureBank) else s


def manifold_metrics(real, generated, k, shift=None):
    """{"precision", "recall", "density", "coverage"} of `generated` (m, D) against `real` (n, D) -- fp64 device
    tensors or FeatureBanks -- as Python floats after ONE read-back of four integers.  With r2_real[j] the k-th
    smallest squared distance from real j to the other real rows (r2_gen likewise):
      precision = mean_i [generated i lies in some real ball],      density = sum_i #(real balls holding i) / (k m),
      recall    = mean_j [real j lies in some generated ball],      coverage = mean_j [some generated i in j's ball].
    Each set needs at least k + 1 rows.  The values depend on k, n and m."""
    real, generated, k = _rows(real), _rows(generated), int(k)
    if not 1 <= k <= MAX_KNN:
        raise ValueError(f"manifold_metrics: k = {k}, need 1 ... {MAX_KNN}")
    n, m = real.shape[0], generated.shape[0]
    if n < k + 1 or m < k + 1:
        raise ValueError(f"manifold_metrics: k = {k} needs at least {k + 1} rows per set, got {n} and {m}")
    r2_real = ops.knn_smallest(real, real, k, shift, 0)[0][:, k - 1].contiguous()
    r2_gen = ops.knn_smallest(generated, generated, k, shift, 0)[0][:, k - 1].contiguous()
    in_real = ops.ball_count(generated, real, r2_real, shift)            # (m,): real balls around generated i
    in_gen = ops.ball_count(real, generated, r2_gen, shift)              # (n,): generated balls around real j
    nearest = ops.knn_smallest(real, generated, 1, shift)[0][:, 0]       # (n,): real j's nearest generated sample
    counts = torch.stack(((in_real > 0).sum(), in_real.sum(dtype=torch.int64), (in_gen > 0).sum(),
                          (nearest <= r2_real).sum())).cpu().tolist()
    return {"precision": counts[0] / m, "recall": counts[2] / n, "density": counts[1] / (k * m),
            "coverage": counts[3] / n}


def nearest_real(generated, real, shift=None):
    """(idx (m,) int32, d2 (m,) fp64) on the device: for every generated row the index of its nearest real row (ties
    to the lower index) and the SQUARED distance to it."""
    d2, idx = ops.knn_smallest(_rows(generated), _rows(real), 1, shift)
    return idx[:, 0], d2[:, 0]


def nn_quantiles(d2):
    """{"min", "q01", "q10", "q50"} of the distances sqrt(max(d2, 0)): order statistics floor(p (m - 1)) of the
    sorted device vector, one read-back of four values, the square root on the host."""
    s = torch.sort(d2).values
    at = torch.tensor([int(p * (s.numel() - 1)) for _, p in NN_QUANTILES], device=s.device)
    host = s[at].cpu().numpy()
    return {name: float(np.sqrt(max(v, 0.0))) for (name, _), v in zip(NN_QUANTILES, host)}


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
    so that the sets' means are differences of comparable sums.  knn = k > 0 also keeps the first knn_max_samples
    feature rows of real / generated (half as many of real_a / real_b) in FeatureBanks, and result() gains
    "manifold"; with knn = 0 no bank exists and nothing else changes."""
    SETS = ("real", "real_a", "real_b", "quantised", "generated")

    BANKS = ("real", "real_a", "real_b", "generated")

    def __init__(self, pool, space="latent", decoder=None, hr_codebook=None, knn=0, knn_max_samples=KNN_MAX_SAMPLES):
        if space not in ("latent", "image"):
            raise ValueError(f"GenerationScorer: space must be 'latent' or 'image', got {space!r}")
        if space == "image" and decoder is None:
            raise ValueError("GenerationScorer: the image space needs a decoder")
        if int(pool) < 1:
            raise ValueError(f"GenerationScorer: pool must be positive, got {pool}")
        if not 0 <= int(knn) <= MAX_KNN or int(knn_max_samples) < 1:
            raise ValueError(f"GenerationScorer: knn = {knn} outside 0 ... {MAX_KNN} (0 = off) or knn_max_samples = "
                             f"{knn_max_samples} not positive")
        self.knn, self.knn_max_samples = int(knn), int(knn_max_samples)
        self._banks = {}
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
        if self.knn and name in self.BANKS:
            b = self._banks.get(name)
            if b is None:      # the halves of the real set hold half of what the whole may
                cap = self.knn_max_samples if name in ("real", "generated") else (self.knn_max_samples + 1) // 2
                b = self._banks[name] = FeatureBank(self.dim, cap)
            b.add(f)

    def bank(self, name):
        """The FeatureBank of a set (knn > 0 only); KeyError for a set nothing was added to."""
        return self._banks[name]

    def manifold(self):
        """The "manifold" entry of result(): the k-NN statistics of (real, generated) and, as the ceiling two real
        samples of this size reach, of (real_a, real_b), with nearest-neighbour distance quantiles."""
        k = self.knn
        small = [n for n in self.BANKS if n not in self._banks or self._banks[n].count < k + 1]
        if small:
            raise ValueError(f"GenerationScorer: knn = {k} needs at least {k + 1} samples per set; too few in "
                             f"{', '.join(small)}")
        b = self._banks
        return {"k": k, "counts": {n: b[n].count for n in self.BANKS},
                "dropped": {n: b[n].dropped for n in self.BANKS},
                "real_generated": manifold_metrics(b["real"], b["generated"], k, self.shift),
                "real_split": manifold_metrics(b["real_a"], b["real_b"], k, self.shift),
                "nn_generated_real": nn_quantiles(nearest_real(b["generated"], b["real"], self.shift)[1]),
                "nn_real_split": nn_quantiles(nearest_real(b["real_b"], b["real_a"], self.shift)[1]),
                "note": MANIFOLD_NOTE}

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
        if self.knn:
            r["manifold"] = self.manifold()
        return r


def summary_line(tag, result):
    parts = []
    for key in ("fd_real_generated", "fd_quantised_generated", "fd_real_quantised", "fd_real_split"):
        if key in result:
            parts.append("{}: {:.6g}".format(key[3:], result[key]["fd"]))
    line = "{} latent-space Frechet distance (not FID) | {} | D: {} | {}".format(
        tag, " | ".join(parts), result["dim"], " ".join(f"{k}={v}" for k, v in result["counts"].items()))
    if "manifold" in result:
        m = result["manifold"]
        for key in ("real_generated", "real_split"):
            line += " | {} k={}: ".format(key, m["k"]) + " ".join(
                "{}={:.4f}".format(name, m[key][name]) for name in ("precision", "recall", "density", "coverage"))
    return line
