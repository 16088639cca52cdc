"""Generation from a token prefix, host side (no GPU): the statuses of the cache-fill entry, the position
numbering of a prefix, which prefixes generate from the cache, and the command line's prompt arithmetic."""
import sys

import pytest
import torch

from conftest import PKG

X = 0x7f0000000000          # a fake, 16-B aligned device address: every call below is refused before any launch


def _fill(*a):
    from qarig import _lib
    return _lib.load().qarig_decode_cache_fill(*a), _lib.last_error()


def test_cache_fill_entry_refuses_bad_arguments_with_a_status():
    # (k, v, ld, batch_stride, kv, images, beams, H, d, P1, max_len, stream); a good call for reference:
    # X, X, 64, 15 * 64, X, 2, 3, 8, 8, 15, 16 -- every variant below breaks one thing
    good = [X, X, 64, 15 * 64, X, 2, 3, 8, 8, 15, 16, None]

    def bad(i, value):
        a = list(good)
        a[i] = value
        return a

    for i in (0, 1, 4):
        st, msg = _fill(*bad(i, None))
        assert st == -1 and "null pointer" in msg
        st, msg = _fill(*bad(i, X + 4))
        assert st == -1 and "16-B aligned" in msg
    for i in (5, 6, 7, 8, 9, 10):                       # images, beams, H, d, P1, max_len
        for v in (0, -1, -7):
            assert _fill(*bad(i, v))[0] == -1, (i, v)
    st, msg = _fill(*bad(9, 17))                        # P1 > max_len
    assert st == -1 and "17 prefix rows for a cache of 16" in msg
    assert _fill(*bad(8, 6))[0] == -1                   # d % 4 != 0
    assert _fill(*bad(2, 60))[0] == -1                  # row stride shorter than H * d
    assert _fill(*bad(2, 66))[0] == -1                  # ... or no multiple of 4
    assert _fill(*bad(2, -64))[0] == -1
    assert _fill(*bad(3, 14 * 64))[0] == -1             # images overlap
    assert _fill(*bad(3, 15 * 64 + 2))[0] == -1
    assert _fill(*bad(3, -4))[0] == -1
    for i in (5, 6, 7, 10):                             # huge extents: refused, no overflow in the grid arithmetic
        assert _fill(*bad(i, 2 ** 31 - 1))[0] == -1, i
    assert _fill(*bad(2, 2 ** 40))[0] == -1 and _fill(*bad(3, 2 ** 44))[0] == -1
    huge = list(good)
    huge[5:11] = [2 ** 24, 2 ** 24, 2 ** 24, 2 ** 24, 2 ** 24, 2 ** 24]
    huge[2], huge[3] = 2 ** 32, 2 ** 40
    assert _fill(*huge)[0] == -1


def test_prefix_position_numbering_in_both_modes():
    from qarig import sampling
    gen = sampling._prefix_pos(2, 5, 1, "cpu")          # generate: cur + tok + 1 -- position 1 is never used
    assert gen.shape == (2, 5) and gen.dtype == torch.float32
    assert gen[0].tolist() == [0.0, 2.0, 3.0, 4.0, 5.0] and torch.equal(gen[0], gen[1])
    train = sampling._prefix_pos(3, 4, 0, "cpu")
    assert train[2].tolist() == [0.0, 1.0, 2.0, 3.0]
    one = sampling._prefix_pos(3, 1, 1, "cpu")          # today's start: zeros (N, 1)
    assert torch.equal(one, torch.zeros(3, 1))
    # the numbering of the cache's own table (_generate_fused: positions) restricted to the prefix
    limit, off = 9, 1
    positions = [0.0] + [float(L + off) for L in range(1, limit)]
    assert gen[0].tolist() == positions[:5]


def test_prefixes_that_generate_from_the_cache():
    from models.Transformer import Transformer
    from qarig import sampling
    m = Transformer(use_encoder=False, use_pos_cond=True, num_enc_layers=None, num_dec_layers=1, num_enc_embedding=None,
                    num_dec_embedding=20, self_attn_heads=4, cross_attn_heads=None, transformer_in_dim=32,
                    transformer_out_dim=21, transformer_hidden_dim=64)
    one, five = torch.zeros(2, 1, dtype=torch.int64), torch.zeros(2, 5, dtype=torch.int64)
    assert sampling._cacheable(m, one, True)                                    # as before, no limit needed
    assert not sampling._cacheable(m, five, True)                               # a prefix needs the cache's size
    assert sampling._cacheable(m, five, True, None, 4, 9)                       # 5 + 4 <= 9: one cached chunk fits
    assert not sampling._cacheable(m, five, True, None, 4, 8)
    assert not sampling._cacheable(m, five, False, None, 4, 9)                  # (position conditioning needs the window)
    # the cache's rows: the window, or the tokens the loop reaches with its overshoot
    assert sampling._cache_limit(five, 24, True, 16, 4, "generate") == 16
    assert sampling._cache_limit(five, 24, False, 16, 4, "generate") == 28
    assert sampling._cache_limit(five, 24, False, 16, 4, "train") == 5 + 24 + 4


def test_prompt_rows_arithmetic_and_refusals():
    from qarig import cli_common as cc
    # an 8 x 8 latent in 1 x 1 patches: 8 rows of 8 tokens
    assert cc.prompt_tokens(0.5, (8, 8), (1, 1), 8) == 32
    assert cc.prompt_tokens(0.25, (8, 8), (1, 1), 8) == 16
    assert cc.prompt_tokens(0.3, (8, 8), (1, 1), 8) == 16          # floor(2.4) rows
    assert cc.prompt_tokens(0.1, (8, 8), (1, 1), 8) == 0           # floor(0.8) rows: an unprompted stage
    assert cc.prompt_tokens(0.29, (100, 4), (1, 2), 2) == 29 * 2   # 0.29 x 100 rows is 29, not 28.999...
    assert cc.prompt_tokens(0.5, (8, 8), (2, 2), 4) == 8           # 4 x 4 grid: 2 rows
    assert cc.prompt_tokens(0.5, (32, 16), (4, 2), 8) == 4 * 8     # rows from the height, tokens per row from the width
    with pytest.raises(Exception, match="Invalid value for beam_width!"):
        cc.prompt_tokens(0.25, (8, 8), (2, 2), 8)                  # 1 row of 4 tokens, chunks of 8
    with pytest.raises(Exception, match="Invalid value for beam_width!"):
        cc.prompt_tokens(0.5, (8, 8), (1, 1), 5)
    # a stage that slides its window: start token + kept tokens stay below the window
    assert cc.prompt_tokens(0.25, (8, 8), (1, 1), 8, sliding_window=32) == 16
    with pytest.raises(Exception, match="sliding window"):
        cc.prompt_tokens(0.5, (8, 8), (1, 1), 8, sliding_window=32)
    assert cc.check_prompt_args(None, None) is False
    assert cc.check_prompt_args("x.json", 0.5) is True
    for fmaps, frac in (("x.json", None), (None, 0.5), ("x.json", 0.0), ("x.json", 1.0), ("x.json", -0.5),
                        ("x.json", float("nan"))):
        with pytest.raises(SystemExit):
            cc.check_prompt_args(fmaps, frac)


def test_generate_images_defaults_are_unchanged_by_the_prompt_flags():
    sys.path.insert(0, PKG)
    import generate_images as gi
    base = ["--decoder-path", "d.pt", "--config-path", "c.json", "--out-dir", "out"]
    a = gi.parse_args(base)
    assert a["prompt_fmaps"] is None and a["prompt_fraction"] is None
    rest = {k: v for k, v in a.items() if not k.startswith("prompt_")}
    assert {k: (str(v) if k.endswith(("_path", "_dir")) else v) for k, v in rest.items()} == dict(
        device="cpu", decoder_path="d.pt", num_images=25, seed=None, config_path="c.json", out_dir="out",
        batch_beams=False, sampler=None, no_kv_cache=False, window_graph=False, cache_padded_heads=False, top_k=None,
        top_p=None, decode_weights="f32")
    b = gi.parse_args(base + ["--prompt-fmaps", "f.json", "--prompt-fraction", "0.25"])
    assert str(b["prompt_fmaps"]) == "f.json" and b["prompt_fraction"] == 0.25
    assert {k: v for k, v in b.items() if not k.startswith("prompt_")} == rest
