"""qarig.evaluate.TokenScorer on the reference-derived train-step fixtures (tests/golden/train_step_{base,encdec}.npz:
recorded results of the reference's own step): one scored window per sample against the reference's logits and loss,
the whole sequences on the deterministic evaluation windows against the existing cross-entropy entry, and a scorer
call between two replays of a captured training step."""
import pytest
import torch

import row_kernel_cases as R
import token_score_cases as T
from conftest import load_golden

pytestmark = pytest.mark.gpu


def _tiny(use_enc, n_dec_emb, n_enc_emb, out_dim):
    from models.Transformer import Transformer
    return Transformer(use_encoder=use_enc, use_pos_cond=True, num_enc_layers=2 if use_enc else None,
                       num_dec_layers=2, num_enc_embedding=n_enc_emb if use_enc else None,
                       num_dec_embedding=n_dec_emb, self_attn_heads=4,
                       cross_attn_heads=2 if use_enc else None, transformer_in_dim=32,
                       transformer_out_dim=out_dim, transformer_hidden_dim=64, hidden_activation="silu")


def _codebook(w, p, image_dim=(8, 8)):
    from models.Codebook import Codebook
    cb = Codebook(patch_dim=(p, p), image_dim=image_dim, image_channel=4, num_embeddings=w.shape[0],
                  init_neighbour_range=4)
    with torch.no_grad():
        cb.codebook.weight.copy_(w)
    return cb.cuda()


def _setup(tag):
    g = load_golden("train_step_" + tag)
    base = tag == "base"
    K_lr, K_hr = g["lr_w"].shape[0], g["hr_w"].shape[0]
    lr_cb, hr_cb = _codebook(g["lr_w"], int(g["lr_patch"])), _codebook(g["hr_w"], int(g["hr_patch"]))
    m = _tiny(not base, K_lr + K_hr if base else K_hr + 1, K_lr, K_hr + 1)
    m.custom_load_state_dict(g["sd"])
    return g, base, lr_cb, hr_cb, m.cuda()


@pytest.mark.parametrize("tag", ["base", "encdec"])
def test_one_window_per_sample_matches_the_reference_step(tag):
    """Row nll within 2 x 1e-5 max|logits| of the fp64 log-softmax of the REFERENCE's logits (the model is held to
    1e-5 max|logits| per logit by tests/test_gpu_pipeline_golden.py; a row's nll moves by at most twice the largest
    logit error), the mean within 1e-5 of the reference's loss."""
    from qarig import ops, pipeline
    g, base, lr_cb, hr_cb, m = _setup(tag)
    window, seq = int(g["window"]), g["full_input"].shape[1]
    hr_in, lr_in, hr_tg, pos = pipeline.tokenize_window(g["fmap"].cuda(), lr_cb, hr_cb, base, window,
                                                        g["rand_indices"])
    with torch.no_grad():
        logits = m(x_dec=hr_in, x_enc=lr_in, pos_cond=pos, pos_bound=seq)
    N, W, C = logits.shape
    nll, rank = ops.token_score(logits.view(-1, C), hr_tg.flatten())
    ref = -torch.log_softmax(g["logits"].double(), -1).view(-1, C)
    ref = ref[torch.arange(N * W), g["hr_target"].flatten()]
    err = float((nll.cpu().double() - ref).abs().max())
    bound = 2 * 1e-5 * float(g["logits"].abs().max())
    print(f"{tag}: row nll err {err:.3e} (bound {bound:.3e})")
    assert err <= bound
    # the rank is exact on the logits the kernel read
    assert torch.equal(rank.cpu(), T.score_ref(logits.view(-1, C).cpu(), hr_tg.flatten().cpu())[1])
    dev = logits.device
    img = torch.zeros(N, dtype=torch.float64, device=dev)
    pos_nll = torch.zeros(W, dtype=torch.float64, device=dev)
    cnt = torch.zeros(W, dtype=torch.int64, device=dev)
    tot = torch.zeros(3, dtype=torch.int64, device=dev)
    ops.score_reduce(nll, rank, N, W, 0, 5, img, pos_nll, cnt, tot)
    assert int(tot[0]) == N * W and (cnt == N).all()
    mean = float(img.sum()) / (N * W)
    print(f"{tag}: mean {mean:.7f} (reference loss {float(g['loss']):.7f})")
    assert abs(mean - float(g["loss"])) < 1e-5
    ops.check_index_flag(dev, "evaluate golden")


@pytest.mark.parametrize("tag", ["base", "encdec"])
def test_scorer_counts_every_token_once_and_agrees_with_cross_entropy(tag):
    from qarig import evaluate, ops, pipeline
    g, base, lr_cb, hr_cb, m = _setup(tag)
    window, seq = int(g["window"]), g["full_input"].shape[1]
    z = g["fmap"].cuda()
    N = z.shape[0]
    scorer = evaluate.TokenScorer(m, lr_cb, hr_cb, base, window)
    m.train()
    scorer.add_batch(z)
    assert m.training
    r = scorer.result()
    assert r["tokens"] == N * seq and r["images"] == N and r["per_position_count"] == [N] * seq
    assert len(r["per_position_nll"]) == seq and len(r["per_image_nll"]) == N
    s_img, s_pos = sum(r["per_image_nll"]), sum(r["per_position_nll"])
    assert abs(s_img - s_pos) <= 4 * (N + seq) * 2.0 ** -53 * s_pos        # two orders of one fp64 sum
    assert r["nll_mean"] == float(torch.tensor(r["per_position_nll"], dtype=torch.float64).sum()) / r["tokens"]
    assert r["bits_per_token"] == pytest.approx(r["nll_mean"] / 0.6931471805599453, rel=1e-15)
    assert 0.0 <= r["top1"] <= r["topk"] <= 1.0

    # the same windows one at a time through the existing cross-entropy entry.  Its row losses are the row kernel's,
    # whose arithmetic token_score_kernel repeats on the same logits; what differs is the mean (fp32, mean2_kernel,
    # within CE_MEAN_TOL_U = 4 u of the rows' mean) against the scorer's fp64 sums: inside CE_TOL_U's 8 u for unit rows
    lr_idx = lr_cb.get_patches_bmu(z, reshape=True)
    hr_idx = hr_cb.get_patches_bmu(z, reshape=True)
    total, rows = 0.0, 0
    with torch.no_grad():
        for start, skip in pipeline.eval_windows(seq, window):
            offs = torch.full((N,), start, dtype=torch.int64, device=z.device)
            hr_in, hr_tg, pos = ops.assemble_tokens(lr_idx, hr_idx, base, lr_cb.num_embeddings, hr_cb.num_embeddings,
                                                    offs, window)
            logits = m(x_dec=hr_in, x_enc=None if base else lr_idx, pos_cond=pos, pos_bound=seq)
            keep = logits[:, skip:].reshape(-1, logits.shape[-1]).contiguous()
            pair, _ = ops.cross_entropy_fwd(keep, hr_tg[:, skip:].reshape(-1).contiguous(), want_grad=False)
            total += float(pair[0]) * keep.shape[0]
            rows += keep.shape[0]
    assert rows == N * seq
    want = total / rows
    e = abs(r["nll_mean"] - want) / (R.U * max(1.0, want))
    print(f"{tag}: nll_mean {r['nll_mean']:.7f}, windows through cross_entropy_fwd {want:.7f}: {e:.3f} u")
    assert e <= R.CE_TOL_U[("loss", "unit")]

    # a second scorer over the same batch twice: the sums double, the means stay
    twice = evaluate.TokenScorer(m, lr_cb, hr_cb, base, window)
    twice.add_batch(z)
    twice.add_batch(z)
    r2 = twice.result()
    assert r2["tokens"] == 2 * r["tokens"] and r2["nll_mean"] == r["nll_mean"]
    assert r2["per_image_nll"] == r["per_image_nll"] * 2


def _graphed_losses(score_between):
    from qarig import evaluate, pipeline
    from qarig.optim import FlatAdam
    g, base, lr_cb, hr_cb, m = _setup("base")
    window = int(g["window"])
    opt = FlatAdam(m.parameters(), lr=1e-3, betas=(0.5, 0.999))
    step = pipeline.GraphedTrainStep(m, opt, lr_cb, hr_cb, base, window, warmup=2)
    z = g["fmap"].cuda()
    losses = []
    for i in range(5):
        if i == 4 and score_between:
            scorer = evaluate.TokenScorer(m, lr_cb, hr_cb, base, window)
            scorer.add_batch(z)
            assert scorer.result()["tokens"] == z.shape[0] * g["full_input"].shape[1]
            assert m.training
        losses.append(step(z, g["rand_indices"]).clone())
    torch.cuda.synchronize()
    assert step.graph is not None
    return torch.stack(losses).cpu(), opt.flat_param.clone().cpu()


def test_scorer_between_two_replays_leaves_the_captured_step_alone():
    la, pa = _graphed_losses(False)
    lb, pb = _graphed_losses(True)
    assert torch.equal(la.view(torch.int32), lb.view(torch.int32))
    assert torch.equal(pa.view(torch.int32), pb.view(torch.int32))
