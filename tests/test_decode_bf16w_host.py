"""Host side of the weight-only bf16 decode step (no GPU): the C entry validates its arguments before it touches a
device, the generation CLI knows --decode-weights, and generate_tokens refuses an unknown mode up front."""
import sys

import pytest


def test_bf16w_entry_validates_without_a_gpu():
    from qarig import _lib
    assert "qarig_decode_linear_bf16w" in _lib.SIGNATURES
    assert _lib.SIGNATURES["qarig_decode_linear_bf16w"] == _lib.SIGNATURES["qarig_decode_linear_f32"]
    h = _lib.load()
    assert h.qarig_decode_linear_bf16w(None, 0, 0, 1e-5, None, None, None, None, 0, None, 0, 0, None, 0, None, 0, None,
                                       0, None, 0, 0, 1, 1, 1, 256, 0, None) == -1
    assert "null operand" in _lib.last_error()


def test_generate_images_parser_knows_decode_weights(monkeypatch, capsys):
    import generate_images
    base = ["generate_images.py", "--decoder-path", "d.pt", "--config-path", "c.json", "--out-dir", "out"]
    monkeypatch.setattr(sys, "argv", base)
    assert generate_images.parse_args()["decode_weights"] == "f32"
    monkeypatch.setattr(sys, "argv", base + ["--decode-weights", "bf16"])
    assert generate_images.parse_args()["decode_weights"] == "bf16"
    monkeypatch.setattr(sys, "argv", base + ["--decode-weights", "fp16"])
    with pytest.raises(SystemExit):
        generate_images.parse_args()
    assert "invalid choice" in capsys.readouterr().err


def test_generate_tokens_refuses_an_unknown_mode_before_touching_a_device():
    import torch
    from qarig import sampling

    class NoDevice:
        def __getattr__(self, name):
            raise AssertionError(f"model.{name} touched before the mode was checked")
    with pytest.raises(ValueError, match="decode weights"):
        sampling.generate_tokens(NoDevice(), torch.zeros((1, 1), dtype=torch.int64), None, 4, 1.0, False, 16,
                                 end_token=3, decode_weights="x")
