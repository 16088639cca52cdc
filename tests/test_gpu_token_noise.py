"""qarig_assemble_tokens_noise and qarig_token_noise on the GPU against the NumPy rule of tests/token_noise_cases.py,
bit for bit: N = 3 samples of 37 hr tokens, 1 and 4 lr tokens, base and encoder-decoder, the whole sequence and
windows of 16 and 1 starting at 0, at the last start and mixed, codebooks of 5, 513 and 8192 codes, neighbour ranges
0, 1 and 7 with ids at both ends of the axis, the smallest, a middle and the largest threshold, a 64-bit seed with
both words set, two steps and two ranks."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import token_noise_cases as TN

pytestmark = pytest.mark.gpu

K_LR = 11


def _key(seed, step, rank):
    from qarig.dropout import DropoutKey
    key = DropoutKey(seed, rank, torch.device("cuda", torch.cuda.current_device()))
    key.set_step(step)
    return key


def _offsets(mode, o_max, N):
    if mode == "zero":
        return [0] * N
    if mode == "last":
        return [o_max] * N
    return [(o_max * n + n) // N % (o_max + 1) for n in range(N)] if o_max else [0] * N      # mixed per sample


def _windows(s_in):
    """(W, offsets mode) pairs: the whole sequence (no offsets), then windows of 16 and 1 at the three starts."""
    return [(None, None)] + [(W, mode) for W in (16, 1) for mode in ("zero", "last", "mixed")]


def _launch(lr, hr, base, K, offs, W, noise):
    from qarig import ops
    t = lambda a: None if a is None else torch.from_numpy(np.asarray(a, dtype=np.int64)).cuda()
    out = ops.assemble_tokens(t(lr), t(hr), base, K_LR, K, t(offs), W, noise=noise)
    return [None if o is None else o.cpu().numpy() for o in out]


@pytest.mark.parametrize("S_lr", TN.S_LRS)
@pytest.mark.parametrize("base", [True, False], ids=["base", "encdec"])
def test_fused_entry_against_the_rule(base, S_lr):
    rng = np.random.default_rng(10 + S_lr + 2 * base)
    lead = S_lr if base else 1
    s_in = lead + TN.S_HR
    keys = {(step, rank): _key(TN.SEED, step, rank) for _, step, rank in TN.STREAMS}
    streams = itertools.cycle(sorted(keys))
    changed = 0
    for K in TN.KS:
        hr = TN.tokens(TN.N, TN.S_HR, K, rng)
        lr = rng.integers(0, K_LR, (TN.N, S_lr)).astype(np.int64)
        for W, mode in _windows(s_in):
            offs = None if W is None else _offsets(mode, s_in - W, TN.N)
            plain = _launch(lr, hr, base, K, offs, W, None)
            for R, T in itertools.product(TN.RS, TN.TS):
                step, rank = next(streams)
                got = _launch(lr, hr, base, K, offs, W, (T, R, keys[(step, rank)].buffer))
                noisy = TN.noise(hr, K, T, R, TN.SEED, 0, step, rank)
                want = TN.assemble(lr, hr, base, K_LR, K, offs, W, noisy_hr=noisy)
                tag = (K, W, mode, R, T, step, rank)
                assert np.array_equal(got[0], want[0]), tag
                # hr_tg and pos: the plain entry's bits (and the rule's)
                assert np.array_equal(got[1], plain[1]) and np.array_equal(got[1], want[1]), tag
                if W is None:
                    assert got[2] is None and plain[2] is None
                else:
                    assert np.array_equal(got[2], plain[2]) and np.array_equal(got[2], want[2]), tag
                # <start> / the leading lr tokens are the plain entry's
                j = np.broadcast_to(np.arange(s_in)[None], (TN.N, s_in)) if W is None else want[2]
                assert np.array_equal(got[0][j < lead], plain[0][j < lead]), tag
                changed += int((got[0] != plain[0]).sum())
    assert changed > 1000
    from qarig import ops
    ops.check_index_flag(torch.device("cuda"), "token noise")


def test_steps_ranks_and_both_seed_words():
    rng = np.random.default_rng(20)
    K, T, R = 513, 32768, 7
    hr = TN.tokens(TN.N, TN.S_HR, K, rng)
    outs = {}
    for _, step, rank in TN.STREAMS:
        outs[(step, rank)] = _launch(None, hr, False, K, None, None, (T, R, _key(TN.SEED, step, rank).buffer))[0]
        want = TN.assemble(None, hr, False, K_LR, K, None, None, TN.noise(hr, K, T, R, TN.SEED, 0, step, rank))[0]
        assert np.array_equal(outs[(step, rank)], want)
    ks = sorted(outs)
    for a, b in itertools.combinations(ks, 2):
        assert not np.array_equal(outs[a], outs[b])
    for seed in (0, 1, 1 << 32, 0xFFFFFFFFFFFFFFFF):
        got = _launch(None, hr, False, K, None, None, (T, R, _key(seed, 0xFFFFFFFF, 0x80000000).buffer))[0]
        want = TN.assemble(None, hr, False, K_LR, K, None, None,
                           TN.noise(hr, K, T, R, seed, 0, 0xFFFFFFFF, 0x80000000))[0]
        assert np.array_equal(got, want), seed


def test_a_token_is_corrupted_alike_through_every_window():
    rng = np.random.default_rng(21)
    K, T, R, W = 513, 32768, 7, 16
    hr = TN.tokens(TN.N, TN.S_HR, K, rng)
    lr = rng.integers(0, K_LR, (TN.N, 4)).astype(np.int64)
    key = _key(TN.SEED, 4, 1)
    for base, lead in ((False, 1), (True, 4)):
        seen = {}
        for offs in ([0, 5, 21], [8, 9, 10], [lead + TN.S_HR - W] * 3):
            hr_in, _, pos = _launch(lr, hr, base, K, offs, W, (T, R, key.buffer))
            for n in range(TN.N):
                for w in range(W):
                    if pos[n, w] >= lead:
                        assert seen.setdefault((n, int(pos[n, w])), int(hr_in[n, w])) == int(hr_in[n, w])
        assert len(seen) > 3 * W


def test_token_noise_entry_agrees_with_the_fused_one_and_the_rule():
    from qarig import ops
    rng = np.random.default_rng(22)
    for K, R, T in itertools.product(TN.KS, TN.RS, TN.TS):
        hr = TN.tokens(TN.N, TN.S_HR, K, rng)
        key = _key(TN.SEED, 3, 1)
        ids = torch.from_numpy(hr).cuda()
        for stream in (0, 1):
            out = ops.token_noise(ids, K, T, R, stream, key.buffer)
            assert np.array_equal(out.cpu().numpy(), TN.noise(hr, K, T, R, TN.SEED, stream, 3, 1)), (K, R, T, stream)
            assert torch.equal(ids.cpu(), torch.from_numpy(hr))                # out of place: the input is kept
            inplace = ids.clone()
            assert ops.token_noise(inplace, K, T, R, stream, key.buffer, out=inplace) is inplace
            assert torch.equal(inplace, out)                                   # in place equals out of place
        fused = _launch(None, hr, False, K, None, None, (T, R, key.buffer))[0]
        assert np.array_equal(fused[:, 1:], ops.token_noise(ids, K, T, R, 0, key.buffer).cpu().numpy())
    # the encoder's shapes: one and four lr tokens, more than one workgroup
    for N, S in ((3, 1), (3, 4), (5, 777)):
        lr = TN.tokens(N, S, K_LR, rng) if S > 1 else rng.integers(0, K_LR, (N, S)).astype(np.int64)
        key = _key(TN.SEED, 2, 0)
        out = ops.token_noise(torch.from_numpy(lr).cuda(), K_LR, 58982, 1, 1, key.buffer)
        assert np.array_equal(out.cpu().numpy(), TN.noise(lr, K_LR, 58982, 1, TN.SEED, 1, 2, 0))


def test_window_start_out_of_range_is_flagged_and_clamped():
    from qarig import ops
    rng = np.random.default_rng(23)
    K, T, R, W = 513, 58982, 1, 16
    hr = TN.tokens(TN.N, TN.S_HR, K, rng)
    key = _key(TN.SEED, 1, 0)
    o_max = 1 + TN.S_HR - W
    ops.check_index_flag(torch.device("cuda"), "before")
    got = _launch(None, hr, False, K, [-1, o_max + 3, 2], W, (T, R, key.buffer))
    with pytest.raises(IndexError):
        ops.check_index_flag(torch.device("cuda"), "window start")
    want = TN.assemble(None, hr, False, K_LR, K, [0, o_max, 2], W, TN.noise(hr, K, T, R, TN.SEED, 0, 1, 0))
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
    ops.check_index_flag(torch.device("cuda"), "after")           # the flag was reset


def test_an_id_out_of_range_passes_through():
    from qarig import ops
    rng = np.random.default_rng(24)
    K, T, R = 513, 58982, 0
    hr = TN.tokens(TN.N, TN.S_HR, K, rng)
    hr[0, 4], hr[1, 9], hr[2, 30] = -1, K, 1 << 40
    key = _key(TN.SEED, 1, 0)
    got = _launch(None, hr, False, K, None, None, (T, R, key.buffer))[0]
    assert got[0, 5] == -1 and got[1, 10] == K and got[2, 31] == 1 << 40
    assert np.array_equal(got[:, 1:], TN.noise(hr, K, T, R, TN.SEED, 0, 1, 0))
    out = ops.token_noise(torch.from_numpy(hr).cuda(), K, T, R, 0, key.buffer).cpu().numpy()
    assert np.array_equal(out, got[:, 1:])
    ops.check_index_flag(torch.device("cuda"), "the noise kernels flag nothing")


def test_refusals_without_a_launch():
    from qarig import _lib
    from qarig.ops import ptr, stream
    lib = _lib.load()
    key = _key(TN.SEED, 1, 0)
    null = ctypes.c_void_p(0)
    N, S, W, K = 3, 37, 16, 513
    hr = torch.from_numpy(TN.tokens(N, S, K, np.random.default_rng(25))).cuda()
    offs = torch.zeros(N, dtype=torch.int64).cuda()
    flag = torch.zeros(1, dtype=torch.int32).cuda()

    def fused(hrp=None, inp=None, tgp=None, keyp=None, threshold=32768, rng_=1, k_hr=K, n=N, s_hr=S):
        hr_in, hr_tg, pos = (torch.full((N, W), 7, dtype=torch.int64).cuda() for _ in range(3))
        r = lib.qarig_assemble_tokens_noise(None, 0, ptr(hr) if hrp is None else hrp, s_hr, n, 0, K_LR, k_hr, ptr(offs), W,
                                            ptr(hr_in) if inp is None else inp, ptr(hr_tg) if tgp is None else tgp,
                                            ptr(pos), ptr(flag), threshold, rng_, ptr(key.buffer) if keyp is None else keyp,
                                            stream())
        torch.cuda.synchronize()
        return r, all(bool((t == 7).all()) for t in (hr_in, hr_tg, pos))

    def whole(idp=None, outp=None, keyp=None, threshold=32768, rng_=1, k=K, n=N, s=S, stream_id=0):
        out = torch.full((N, S), 7, dtype=torch.int64).cuda()
        r = lib.qarig_token_noise(ptr(hr) if idp is None else idp, ptr(out) if outp is None else outp, n, s, k, threshold,
                                  rng_, stream_id, ptr(key.buffer) if keyp is None else keyp, stream())
        torch.cuda.synchronize()
        return r, bool((out == 7).all())

    assert fused() == (0, False) and whole() == (0, False)             # the control: accepted and launched
    big = dict(n=1 << 16, s_hr=1 << 15)                                # N S_hr = 2^31
    for bad in (dict(hrp=null), dict(inp=null), dict(tgp=null), dict(keyp=null), dict(threshold=0),
                dict(threshold=58983), dict(rng_=-1), dict(k_hr=0), big):
        assert fused(**bad) == (-1, True), bad
        assert "assemble_tokens" in _lib.last_error()
    for bad in (dict(idp=null), dict(outp=null), dict(keyp=null), dict(threshold=0), dict(threshold=58983),
                dict(rng_=-1), dict(k=0), dict(n=1 << 16, s=1 << 15), dict(stream_id=2), dict(stream_id=-1)):
        assert whole(**bad) == (-1, True), bad
        assert "token_noise" in _lib.last_error()
    # out overlapping ids without being ids
    buf = torch.full((N * S + 1,), 7, dtype=torch.int64).cuda()
    r = lib.qarig_token_noise(ptr(buf), buf.data_ptr() + 8, N, S, K, 32768, 1, 0, ptr(key.buffer), stream())
    torch.cuda.synchronize()
    assert r == -1 and bool((buf == 7).all()) and "overlap" in _lib.last_error()
    assert int(flag.item()) == 0


def test_a_captured_launch_reads_the_step_of_its_replay():
    from qarig import ops
    rng = np.random.default_rng(26)
    K, T, R, W = 513, 32768, 7, 16
    hr_np = TN.tokens(TN.N, TN.S_HR, K, rng)
    hr = torch.from_numpy(hr_np).cuda()
    offs = torch.tensor([0, 5, 21]).cuda()
    key = _key(TN.SEED, 1, 0)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                      # the bad-index flag exists before the capture
        ops.assemble_tokens(None, hr, False, K_LR, K, offs, W, noise=(T, R, key.buffer))
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        hr_in, hr_tg, pos = ops.assemble_tokens(None, hr, False, K_LR, K, offs, W, noise=(T, R, key.buffer))
    seen = []
    for step in (1, 2):
        key.set_step(step)
        graph.replay()
        torch.cuda.synchronize()
        want = TN.assemble(None, hr_np, False, K_LR, K, [0, 5, 21], W, TN.noise(hr_np, K, T, R, TN.SEED, 0, step, 0))
        assert np.array_equal(hr_in.cpu().numpy(), want[0]), step
        assert np.array_equal(hr_tg.cpu().numpy(), want[1]) and np.array_equal(pos.cpu().numpy(), want[2])
        seen.append(hr_in.cpu().numpy().copy())
    assert not np.array_equal(seen[0], seen[1])
