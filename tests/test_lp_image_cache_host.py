"""The cached weight images of qarig.ops (bf16 / e4m3 / MX shadows, the transposed and zero-padded bf16 forms, the
conv forward's re-ordered weights): every user keeps one image per weight until the weight changes -- torch's
version counter, ops.lp_invalidate() -- serves it only to the tensor it was made from, and neither reads nor
writes the cache under stream capture.  No GPU: the library is a stand-in whose entries succeed, so the
"images" are uninitialised CPU tensors; what is checked is which object comes back."""
import pytest
import torch

LP_EPOCH, OPTION_EPOCH = 7, 3
GEOM = (2, 16, 16, 1, 1, 0)


class _Lib:
    def __getattr__(self, name):
        return lambda *a: 0


def _tagged(w):
    wd = w.detach()
    wd._qarig_weight = True
    wd._qarig_src = w
    return wd


def _users():
    """name -> (weight shape, image of a weight as that user builds it)."""
    from qarig import functional_lp, ops
    return {
        "cast_bf16": ((256, 128), lambda w: ops.cast_bf16(_tagged(w), cache=True)),
        "cast_fp8": ((256, 128), lambda w: ops.cast_fp8(_tagged(w), cache=True)),
        "cast_transpose_bf16": ((256, 128), lambda w: ops.cast_transpose_bf16(_tagged(w), cache=True)),
        "mx_weight": ((130, 128), lambda w: ops.mx_weight(w, 256)),
        "conv": ((8, 4, 3, 3), lambda w: ops._conv_workspace(w, 4096, GEOM, "convfwd", True)[0]),
        "shadow_padded": ((130, 128), lambda w: functional_lp._shadow(w, transpose=True, pad_rows=256)),
    }


# list(ops._lp_cache) after one call of each user, as the code before the shared helper left it ("ptr": the
# weight's address)
KEYS = {
    "cast_bf16": [("n", "ptr", (256, 128), 0, LP_EPOCH)],
    "cast_fp8": [("f8", "ptr", (256, 128), 0, LP_EPOCH)],
    "cast_transpose_bf16": [("t", "ptr", (256, 128), 128, 0, LP_EPOCH)],
    "mx_weight": [("mx", "ptr", (130, 128), 256, 0, LP_EPOCH)],
    "conv": [("convfwd", "ptr", (8, 4, 3, 3), 0, LP_EPOCH, OPTION_EPOCH, GEOM)],
    "shadow_padded": [("p", "ptr", (130, 128), 256, True, 0, LP_EPOCH)],
}


@pytest.fixture
def cache(monkeypatch):
    from qarig import _lib, ops
    state = {"capturing": False}
    monkeypatch.setattr(_lib, "load", lambda: _Lib())
    monkeypatch.setattr(_lib, "OPTION_EPOCH", OPTION_EPOCH)
    monkeypatch.setattr(ops, "stream", lambda: 0)
    monkeypatch.setattr(ops, "workspace", lambda nbytes, device, tag="default": torch.empty(16, dtype=torch.uint8))
    monkeypatch.setattr(ops, "LP_EPOCH", LP_EPOCH)
    monkeypatch.setattr(ops, "_lp_cache", {})
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: state["capturing"])
    return state


def _weight(shape):
    return torch.nn.Parameter(torch.randn(shape, generator=torch.Generator().manual_seed(0)))


@pytest.mark.parametrize("user", sorted(KEYS))
def test_image_is_kept_until_the_weight_changes(cache, user):
    from qarig import ops
    shape, image = _users()[user]
    w = _weight(shape)
    first = image(w)
    keys = [tuple("ptr" if e == w.data_ptr() else e for e in k) for k in ops._lp_cache]
    assert keys == KEYS[user]
    assert image(w) is first and len(ops._lp_cache) == 1
    ops.lp_invalidate()
    assert ops.LP_EPOCH == LP_EPOCH + 1 and not ops._lp_cache
    second = image(w)
    assert second is not first and image(w) is second
    with torch.no_grad():
        w.add_(1.0)                                   # raises w._version
    third = image(w)
    assert third is not second and image(w) is third


@pytest.mark.parametrize("user", sorted(KEYS))
def test_image_serves_only_the_tensor_it_was_made_from(cache, user):
    from qarig import ops
    shape, image = _users()[user]
    w = _weight(shape)
    other = w.detach()                                # another tensor object at the same address / shape / version
    assert (other.data_ptr(), other.shape, other._version) == (w.data_ptr(), w.shape, w._version) and other is not w
    first = image(w)
    (key,) = list(ops._lp_cache)
    got = image(other)
    assert got is not first
    assert list(ops._lp_cache) == [key] and ops._lp_cache[key][0]() is other and image(other) is got


@pytest.mark.parametrize("user", sorted(KEYS))
def test_nothing_is_read_or_stored_under_stream_capture(cache, user):
    from qarig import ops
    shape, image = _users()[user]
    w = _weight(shape)
    cache["capturing"] = True
    a = image(w)
    assert not ops._lp_cache and image(w) is not a and not ops._lp_cache
    cache["capturing"] = False
    kept = image(w)
    entries = dict(ops._lp_cache)
    cache["capturing"] = True
    assert image(w) is not kept and ops._lp_cache == entries
    cache["capturing"] = False
    assert image(w) is kept
