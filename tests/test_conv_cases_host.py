"""The pieces of tests/conv_cases.py on the CPU: the exact arm's premise holds for every case on its own, the tables
hold what they say, the split rows are the ones the scratch-size functions promise slabs for, and offset_view does
what the GPU test relies on.  No GPU is touched."""
import pytest
import torch

from conftest import PKG  # noqa: F401  (puts the package on sys.path)
import conv_cases as cc


def _lib():
    import build as qbuild
    qbuild.build_lib(verbose=False)
    from qarig import _lib
    return _lib.load(), _lib


def test_every_exact_case_stays_below_2_to_24_and_its_reference_is_fp32():
    """Every product and partial sum of every output is an integer below 2^24 (the sums over absolute values
    bound every partial sum in every order), and the fp64 reference survives a round trip through fp32."""
    cases = cc.exact_cases() + (cc.SHORTCUT,)
    assert len(cases) == len(set(cases)) >= len(cc.GEOMETRY) + len(cc.FORWARD_ONLY) + 10
    for c in cases:
        (x, w, b, dy), ref, ref_nb = cc.int_case(c)
        for t in (x, w, b, dy):
            assert torch.equal(t, t.round())
        assert float(x.abs().max()) <= 4 and float(dy.abs().max()) <= 4 and float(w.abs().max()) <= 3
        assert float(b.abs().max()) <= 8
        assert cc.exact_bound(c, x, w, b, dy) < 2 ** 24, c.name
        for r in (ref, ref_nb):
            for t in r:
                if t is not None:
                    assert torch.equal(t.float().double(), t) and torch.equal(t, t.round()), c.name
        assert ref_nb.db is None and ref.db is not None


def test_a_quarter_of_the_integer_weights_is_zero_and_moves_with_the_group():
    for c in (cc.GEOMETRY[0], cc.PATH["ring_s1_fwd"].case, cc.PATH["ring_convt_fwd"].case):
        _, w, _, _ = cc.int_operands(c)
        i = torch.arange(w.numel())
        forced = (i + i // 4 + i // 16) % 4 == 0
        assert bool((w.view(-1)[forced] == 0).all())
        assert int(forced.sum()) * 4 in range(w.numel(), w.numel() + 4)
        if w.numel() >= 32:
            assert len({int(torch.nonzero(forced[g * 4:g * 4 + 4])[0]) for g in range(8)}) == 4
        assert float((w != 0).float().mean()) > 0.5


def test_geometry_holds_every_combination_in_every_regime():
    assert len(cc.GEOMETRIES) == 20
    for reg in cc.REGIMES:
        got = {(c.k, c.stride, c.pad) for c in cc.GEOMETRY if cc.regime(c) == reg}
        assert got == set(cc.GEOMETRIES), reg
    for c in cc.GEOMETRY:
        assert c.kind == "conv" and cc.bwd_data_accepts(c) and cc.wgrad_accepts(c)
        assert c.N <= 3 and c.H <= 32 and c.W <= 32 and c.Cin <= 128 and c.Cout <= 136
        Ho, Wo = cc.out_hw(c)
        assert Ho > 0 and Wo > 0
        if cc.regime(c) == "gather-row":
            assert Wo % 8 == 0 and c.Cout > 128
        if cc.regime(c) == "direct":
            assert c.Cin <= 8 and c.Cout <= 8
    assert {(c.Cin, c.Cout) for c in cc.GEOMETRY if cc.regime(c) == "direct"} == {(5, 3), (3, 5)}
    extra = [c for c in cc.GEOMETRY if cc.regime(c) not in cc.REGIMES]
    assert [(c.N, c.Cin, c.H, c.W, c.Cout, c.k, c.stride, c.pad) for c in extra] == [(1, 128, 16, 16, 16, 1, 2, 0)]
    # most gather cases are no multiple of 4 wide (SrcIm2col), some are (SrcIm2colRow with guarded tiles)
    wide4 = [cc.out_hw(c)[1] % 4 == 0 for c in cc.GEOMETRY if cc.regime(c) == "gather"]
    assert 0 < sum(wide4) < len(wide4) / 2


def test_every_stride2_kernel_size_has_an_uncovered_trailing_row_with_zero_gradient():
    for k in (1, 2, 3, 4):
        hit = [c for c in cc.GEOMETRY if c.k == k and c.stride == 2 and cc.uncovered_rows(c)]
        assert hit, k
        for c in hit:
            _, ref, _ = cc.int_case(c)
            assert bool((ref.dx[:, :, c.H - 1, :] == 0).all()), c.name
            assert bool((ref.dx != 0).any())
    odd = [c for c in cc.GEOMETRY if c.stride == 2 and c.H % 2 and c.W % 2]
    assert odd and all(c.H != 2 * cc.out_hw(c)[0] for c in odd)


def test_the_1x1_stride2_reference_gradient_is_zero_at_odd_rows_and_columns():
    cases = [c for c in cc.GEOMETRY if (c.k, c.stride, c.pad) == (1, 2, 0)] + [cc.SHORTCUT]
    assert len(cases) == 6
    for c in cases:
        _, ref, _ = cc.int_case(c)
        assert bool((ref.dx[:, :, 1::2, :] == 0).all()) and bool((ref.dx[:, :, :, 1::2] == 0).all())
        assert bool((ref.dx[:, :, ::2, ::2] != 0).any())


def test_forward_only_geometries_are_the_ones_a_gradient_refuses():
    assert len({(c.k, c.stride, c.pad) for c in cc.FORWARD_ONLY}) == len(cc.FORWARD_ONLY_GEOMETRIES) >= 5
    for c in cc.FORWARD_ONLY:
        assert 1 <= c.k <= 4 and 1 <= c.stride <= 4 and 0 <= c.pad <= 4
        assert not cc.bwd_data_accepts(c) and (c.stride > 2 or c.pad >= c.k)
        assert min(cc.out_hw(c)) > 0
    assert any(c.stride == 3 for c in cc.FORWARD_ONLY) and any(c.stride == 4 for c in cc.FORWARD_ONLY)
    assert any(c.pad >= c.k and c.stride <= 2 for c in cc.FORWARD_ONLY) and any(c.pad == 4 for c in cc.FORWARD_ONLY)
    for N, Cin, H, W, k, s, p in cc.EMPTY_OUTPUTS:
        assert H + 2 * p < k or W + 2 * p < k


def test_split_rows_are_promised_slabs_and_the_others_are_not():
    h, lib = _lib()
    seen = set()
    for path in cc.PATHS:
        olds = [(name, lib.set_option(name, v)) for name, v in path.opts]
        try:
            sizes = cc.workspace_sizes(h, path.case)
        finally:
            for name, old in reversed(olds):
                lib.set_option(name, old)
        assert set(path.splits) <= set(sizes)
        for which, (n, base) in sizes.items():
            assert base > 0
            if which in path.splits:
                assert n > base, (path.case.name, which)
                seen.add(which)
            else:
                assert n == base, (path.case.name, which)
    assert seen == {"fwd", "dgrad", "convt_fwd", "convt_dgrad"}


def test_alignment_rows_name_paths_and_cover_the_issue_table():
    want = {("fwd", "x", 4), ("fwd", "y", 4), ("fwd", "y", 8), ("fwd", "w", 4), ("fwd", "workspace", 4),
            ("convt_fwd", "x", 4), ("convt_fwd", "y", 4), ("convt_fwd", "y", 8), ("convt_fwd", "workspace", 4),
            ("dgrad", "dT", 4), ("dgrad", "dx", 4), ("dgrad", "dx", 8),
            ("convt_dgrad", "dT", 4), ("convt_dgrad", "dx", 4), ("convt_dgrad", "dx", 8),
            ("wgrad", "G", 4), ("wgrad", "X", 4), ("wgrad", "dw", 4)}
    assert {(a.entry, a.operand, a.off) for a in cc.ALIGNMENT} == want
    for a in cc.ALIGNMENT:
        kind = cc.PATH[a.path].case.kind
        assert (kind == "convt") == a.entry.startswith("convt")
    # the dx offsets reach the stride-1 and the stride-2 data gradient; the weight gradient both channel regimes
    for off in (4, 8):
        assert {cc.PATH[a.path].case.stride for a in cc.ALIGNMENT if (a.entry, a.operand, a.off) == ("dgrad", "dx", off)} == {1, 2}
    for operand in ("G", "X", "dw"):
        cg = {cc.PATH[a.path].case.Cout for a in cc.ALIGNMENT if a.entry == "wgrad" and a.operand == operand}
        assert min(cg) <= 4 and max(cg) == 128


@pytest.mark.parametrize("off", [4, 8])
def test_offset_view_is_contiguous_offset_and_guarded(off):
    t = torch.arange(2 * 3 * 5 * 7, dtype=torch.float32).reshape(2, 3, 5, 7)
    for copy in (True, False):
        v, buf, front, back = cc.offset_view(t, off, copy=copy)
        assert v.is_contiguous() and v.shape == t.shape and v.data_ptr() % 16 == off
        assert front.numel() == back.numel() == 64
        assert front.data_ptr() + 4 * front.numel() == v.data_ptr()
        assert back.data_ptr() == v.data_ptr() + 4 * v.numel()
        assert buf.data_ptr() <= front.data_ptr() and back.data_ptr() + 4 * back.numel() <= buf.data_ptr() + 4 * buf.numel()
        assert cc.guards_intact(front, back)
        if copy:
            assert torch.equal(v, t)
        else:
            assert bool(torch.isnan(v).all()) and bool((v.view(torch.int32) == cc.NAN_PATTERN).all())
        v.fill_(1.0)                          # a write to the view leaves the guards alone ...
        assert cc.guards_intact(front, back)
        front[-1] = 0.0                       # ... and a write to a guard is seen
        assert not cc.guards_intact(front, back)
