"""SOM topology evaluation of a codebook (additive; the reference has none): are codes that are neighbours on the
codebook's one-dimensional index axis neighbours in latent space?  Neighbour-smoothed targets, token noise within a
range R and the Gaussian over the index distance in Codebook.get_quantized_patches all assume so.

Two measurements.  From data: the topographic error -- the share of patch rows whose best and second-best matching
units (ops.bmu_top2) are not adjacent codes -- with the histogram of the index gap behind it, the mean distances to
both units and the histogram of d1 / d2 (how ambiguous the tokenisation is).  From the codebook alone: the lag
profile, the mean latent distance between codes t and t + r for every lag r (ops.code_lag_profile), the curve from
which --neighbour-range, --neighbour-sigma and --noise-range are read.

Built like recon_eval.ReconScorer: integer histograms and per-image fp64 sums stay on the device for a whole dataset
and are read back once, in result(); the blocks are pure host functions of what was read back."""
import math

import torch

from . import ops

RATIO_BINS = 32
LAG_LISTED = 64      # lags whose mean distance the block lists


def _powers_below(K):
    r, out = 1, []
    while r < K:
        out.append(r)
        r *= 2
    return out


def topology_block(gap_hist, ratio_hist, img_sums, rows):
    """The data side of a topology block from gap_hist (int [K]: rows per |idx1 - idx2|), ratio_hist (int [32]),
    img_sums (per image {sum d1, sum d2, sum d1^2}) and the number of rows they cover.  Host arithmetic only.
    median_gap is the smallest gap g with at least half of the rows at gaps <= g."""
    gap = [int(c) for c in gap_hist]
    ratio = [int(c) for c in ratio_hist]
    K, rows = len(gap), int(rows)
    if K < 2 or rows < 1 or sum(gap) != rows or sum(ratio) != rows or gap[0] != 0 or len(ratio) != RATIO_BINS:
        raise ValueError(f"topology_block: histograms of {sum(gap)} / {sum(ratio)} rows (gap 0: {gap[0]}) for "
                         f"{rows} rows of a {K}-code search")
    cum, c = [], 0
    for v in gap:
        c += v
        cum.append(c)
    radii = _powers_below(K)
    block = {
        "rows": rows,
        "topographic_error": 1.0 - gap[1] / rows,
        "within": {r: cum[r] / rows for r in radii},
        # the second unit uniform over the other K - 1 codes, averaged over the first:
        # mean_t (min(t, r) + min(K-1-t, r)) / (K-1), and sum_t min(t, r) = r (r-1) / 2 + r (K-r)
        "within_uniform": {r: (r * (r - 1) + 2 * r * (K - r)) / (K * (K - 1)) for r in radii},
        "mean_gap": sum(g * v for g, v in enumerate(gap)) / rows,
        "median_gap": next(g for g, v in enumerate(cum) if 2 * v >= rows),
        "quantisation_error": math.fsum(s[0] for s in img_sums) / rows,
        "second_error": math.fsum(s[1] for s in img_sums) / rows,
        "quantisation_mse": math.fsum(s[2] for s in img_sums) / rows,
        "ratio_hist": ratio,
    }
    if img_sums and rows % len(img_sums) == 0:
        per = rows // len(img_sums)
        block["per_image_quantisation_error"] = [s[0] / per for s in img_sums]
    return block


def lag_block(lag_sum, K):
    """The codebook side: lag_sum[r] = sum_t |w_t - w_{t+r}| (r = 1 ... K-1; [0] unused) -> the mean distance per
    lag (listed up to lag 64), the mean over all pairs, and lag_half, the first lag whose mean distance reaches
    half of that mean (None where none does).  Host arithmetic only."""
    K = int(K)
    if K < 2 or len(lag_sum) != K:
        raise ValueError(f"lag_block: {len(lag_sum)} lag sums for {K} codes")
    mean = [None] + [float(lag_sum[r]) / (K - r) for r in range(1, K)]
    all_pairs = math.fsum(float(v) for v in lag_sum[1:]) / (K * (K - 1) // 2)
    half = next((r for r in range(1, K) if mean[r] >= 0.5 * all_pairs), None) if all_pairs > 0.0 else None
    return {"mean_distance": {r: mean[r] for r in range(1, min(K - 1, LAG_LISTED) + 1)},
            "all_pairs_mean": all_pairs, "lag_half": half}


class TopologyScorer:
    def __init__(self, codebooks):
        self.codebooks = dict(codebooks)
        self.device = None
        self._state = {}     # codebook name -> [gap_hist int64 (K,), ratio_hist int64 (32,), [img_sums (N,3)], rows]

    @torch.no_grad()
    def add_batch(self, latent):
        """Searches one batch of latents (N,C,H,W) against every codebook and reduces it on the device; nothing is
        read back."""
        self.device = latent.device
        for name, cb in self.codebooks.items():
            st = self._state.get(name)
            if st is None:
                st = self._state[name] = [torch.zeros(cb.num_embeddings, dtype=torch.int64, device=latent.device),
                                          torch.zeros(RATIO_BINS, dtype=torch.int64, device=latent.device), [], 0]
            i1, i2, d1, d2 = ops.bmu_top2(latent, cb.codebook.weight.detach(), cb.patch_dim)
            st[2].append(ops.topology_rows(i1, i2, d1, d2, latent.shape[0], st[0], st[1]))
            st[3] += i1.numel()

    def result(self):
        """The one read-back: {name: topology block with its "lag" block}."""
        if self.device is None:
            raise RuntimeError("TopologyScorer.result: no batch was scored")
        ops.check_index_flag(self.device, "topology evaluation")
        out = {}
        for name, cb in self.codebooks.items():
            gap, ratio, sums, rows = self._state[name]
            block = topology_block(gap.cpu().tolist(), ratio.cpu().tolist(), torch.cat(sums).cpu().tolist(), rows)
            block["lag"] = lag_block(ops.code_lag_profile(cb.codebook.weight.detach()).cpu().tolist(),
                                     cb.num_embeddings)
            out[name] = block
        return out


def topology_summary_line(tag, block):
    """One log line for a codebook's topology block."""
    w = block["within"]
    return "Topology {} TE: {:.4f} | within 2/4/8: {} | lag_half: {}".format(
        tag, block["topographic_error"],
        " / ".join("{:.4f}".format(w[r]) if r in w else "-" for r in (2, 4, 8)), block["lag"]["lag_half"])
