"""qarig_grad_clip_coef and qarig_adam_clip_step (csrc/optim.hip) against their fp64 definition, against the plain
Adam entries and against their own documented behaviour around n: tolerances, inputs and sizes from
tests/grad_clip_cases.py, where the bounds are derived (tests/test_grad_clip_host.py shows the specified arithmetic
meets them and seven wrong clips do not)."""
import math

import numpy as np
import pytest
import torch

import adamw_cases as A
import grad_clip_cases as C

pytestmark = pytest.mark.gpu

PAD = 32
CANARY = 0x7FC0BEEF                     # an fp32 NaN with a payload
CANARY16 = 0x7FC1
CANARY64 = 0x7FF8BEEF0BADF00D           # an fp64 NaN with a payload
CASES = list(C.cases())
ADAM_SIZES = [1, 7, 8, 9, 15, 16, 17, 2047, 2048, 2049, 8 * 256 * 3 + 5]
BIG = 8192 * 256 * 8 + 8 + 3            # past one sweep of the Adam kernel's capped grid


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _padded(values):
    n = values.numel()
    buf = torch.full((n + PAD,), CANARY, dtype=torch.int32, device="cuda")
    view = buf.view(torch.float32)[:n]
    view.copy_(values)
    return buf, view


def _padded_shadow(n):
    buf = torch.full((n + PAD,), CANARY16, dtype=torch.int16, device="cuda")
    return buf, buf.view(torch.bfloat16)[:n]


def _intact(buf, n):
    return bool((buf[n:] == (CANARY if buf.dtype == torch.int32 else CANARY16)).all())


class _Scratch:
    """partials and state with canaries in front and behind."""

    def __init__(self):
        self.pbuf = torch.full((PAD + C.PARTIALS + PAD,), CANARY64, dtype=torch.int64, device="cuda")
        self.sbuf = torch.full((PAD + 4 + PAD,), CANARY64, dtype=torch.int64, device="cuda")
        self.partials = self.pbuf.view(torch.float64)[PAD:PAD + C.PARTIALS]
        self.state = self.sbuf.view(torch.float64)[PAD:PAD + 4]
        self.state.zero_()

    def intact(self):
        return all(bool((b[:PAD] == CANARY64).all()) and bool((b[-PAD:] == CANARY64).all())
                   for b in (self.pbuf, self.sbuf))

    def partials_written(self, n):
        """The first B partials were written (no canary left), nothing behind them."""
        blocks = C.grid(n)[0]
        raw = self.pbuf[PAD:PAD + C.PARTIALS]
        return bool((raw[:blocks] != CANARY64).all()) and bool((raw[blocks:] == CANARY64).all())


def _host_coef(norm, max_norm):
    return C.coef_def(norm, max_norm)


# ================================================================================================================
# qarig_grad_clip_coef
# ================================================================================================================
@pytest.mark.parametrize("n", C.NORM_SIZES)
def test_norm_and_coefficient_against_fp64(n):
    """Gaussian data at three scales, three grad_scales, max_norm below the norm, above it and inf: the norm inside
    its derived bound of the fp64 reference, the coefficient bit-equal to the rule evaluated on the device's own
    norm, the counters following, the same bits on a second call, canaries behind n and around both buffers."""
    from qarig import ops
    gen = torch.Generator(device="cuda").manual_seed(77 + n)
    sc = _Scratch()
    worst, skipped, clipped, k = 0.0, 0, 0, 0
    for scale in (1.0, 2.0 ** -10, 2.0 ** 10):
        buf, g = _padded(torch.randn(n, device="cuda", generator=gen) * scale)
        for gs in (1.0, 0.5, 2.0 ** -10):
            ref = C.norm_ref64(g, gs)
            max_norm = (0.37 * ref, 3.0 * ref, float("inf"))[k % 3] if ref > 0 else 1.0
            k += 1
            ops.grad_clip_coef(g, gs, max_norm, sc.partials, sc.state)
            first = sc.state.clone()
            ops.grad_clip_coef(g, gs, max_norm, sc.partials, sc.state)
            second = sc.state.clone()
            norm, coef, sk, cl = second.tolist()
            assert torch.equal(first[:2].view(torch.int64), second[:2].view(torch.int64))
            err = abs(norm - ref) / ref if ref > 0 else abs(norm)
            worst = max(worst, err / C.bound_norm(n))
            want = _host_coef(norm, max_norm)
            assert coef == want and A.f32(coef) == coef, (n, scale, gs, coef, want)
            if want < 1.0:
                clipped += 2
            assert (sk, cl) == (skipped, clipped), (n, scale, gs)
            assert (coef < 1.0) == (k % 3 == 1) or ref < 1e-5     # (k was advanced: the first of three clips)
            assert sc.partials_written(n)
        assert _intact(buf, n)
    assert sc.intact()
    print(f"grad_clip_coef n={n}: worst |norm - ref| / bound = {worst:.4f} (bound {C.bound_norm(n) / C.U64:.1f} "
          f"x 2^-53 relative), clipped {clipped} of {2 * k} calls")
    assert worst <= 1.0
    assert clipped > 0 or n == 1


def test_exact_norms():
    """4^j entries equal to 2^k: every partial sum is a power of two times an integer below 2^53, so the norm is
    2^(k + j) exactly, whatever the order."""
    from qarig import ops
    sc = _Scratch()
    for j, k in ((0, 0), (1, 3), (2, -5), (3, 0), (5, -7), (6, 9), (8, 10), (10, 0), (11, -3)):
        g_np, want = C.exact_power_data(j, k)
        g = torch.from_numpy(g_np).cuda()
        ops.grad_clip_coef(g, 1.0, want, sc.partials, sc.state)
        norm, coef = sc.state.tolist()[:2]
        assert norm == want, (j, k, norm)
        assert coef == A.f32(want / (want + 1e-6))
        ops.grad_clip_coef(g, 0.5, float("inf"), sc.partials, sc.state)
        assert sc.state.tolist()[:2] == [want / 2, 1.0]
    assert sc.intact()


@pytest.mark.parametrize("n", [5, 1025, C.SWEEP + 1])
def test_squares_beyond_fp32_range(n):
    """1e30: fp32 squares overflow, the fp64 norm is finite and the step is clipped, not skipped.  1e-30: fp32
    squares vanish, the norm must not."""
    from qarig import ops
    sc = _Scratch()
    g = torch.full((n,), 1e30, device="cuda")
    ops.grad_clip_coef(g, 1.0, 1.0, sc.partials, sc.state)
    norm, coef, sk, cl = sc.state.tolist()
    ref = C.norm_ref64(g)
    assert math.isfinite(norm) and abs(norm - ref) <= C.bound_norm(n) * ref
    assert (sk, cl) == (0, 1) and 0.0 < coef < 1e-29 and coef == _host_coef(norm, 1.0)
    g.fill_(1e-30)
    ops.grad_clip_coef(g, 1.0, 1.0, sc.partials, sc.state)
    norm, coef, sk, cl = sc.state.tolist()
    ref = C.norm_ref64(g)
    assert norm > 0 and abs(norm - ref) <= C.bound_norm(n) * ref
    assert (coef, sk, cl) == (1.0, 0, 1)


@pytest.mark.parametrize("n", [1, 6, 1027, C.SWEEP + 1027])
def test_one_non_finite_element_anywhere_skips(n):
    """A single NaN, +inf or -inf at index 0, at n - 1, at the first tail element and in the last workgroup's
    range: a non-finite state[0], skipped + 1, clipped unchanged; the data put back gives a finite norm again."""
    from qarig import ops
    sc = _Scratch()
    g = torch.ones(n, device="cuda")
    blocks = C.grid(n)[0]
    places = sorted({0, n - 1, 4 * (n // 4) if n % 4 else n - 1, min(n - 1, (blocks - 1) * 1024 + 4 * 64 + 1)})
    skipped = 0
    for at in places:
        for bad in (float("nan"), float("inf"), float("-inf")):
            g[at] = bad
            ops.grad_clip_coef(g, 0.5, 1e9, sc.partials, sc.state)
            norm, coef, sk, cl = sc.state.tolist()
            skipped += 1
            assert not math.isfinite(norm) and coef == 0.0 and (sk, cl) == (skipped, 0), (n, at, bad)
            g[at] = 1.0
    ops.grad_clip_coef(g, 0.5, 1e9, sc.partials, sc.state)
    norm, coef, sk, cl = sc.state.tolist()
    assert norm == 0.5 * math.sqrt(n) or abs(norm - 0.5 * math.sqrt(n)) <= C.bound_norm(n) * norm
    assert (coef, sk, cl) == (1.0, skipped, 0)
    assert sc.intact()


def test_counters_over_a_sequence():
    from qarig import ops
    sc = _Scratch()
    n = 1029
    g = torch.randn(n, device="cuda")
    norm = C.norm_ref64(g)
    want = [0, 0]
    for kind in ("clip", "pass", "skip", "skip", "clip", "inf", "pass", "skip", "clip"):
        g[7] = float("nan") if kind == "skip" else 0.25
        ops.grad_clip_coef(g, 1.0, {"clip": 0.5 * norm, "pass": 2 * norm, "skip": 1.0, "inf": float("inf")}[kind],
                           sc.partials, sc.state)
        want[0] += kind == "skip"
        want[1] += kind == "clip"
        assert sc.state.tolist()[2:] == want, kind
    assert want == [3, 3]


def test_grad_clip_coef_refusals_launch_nothing():
    from qarig import _lib
    lib = _lib.load()
    sc = _Scratch()
    g = torch.ones(64, device="cuda")
    before_p, before_s = sc.pbuf.clone(), sc.sbuf.clone()
    s = _lib.stream()

    def call(g=g.data_ptr(), n=64, gs=1.0, c=1.0, partials=sc.partials.data_ptr(), state=sc.state.data_ptr()):
        return lib.qarig_grad_clip_coef(g, n, gs, c, partials, state, s)

    for kw in (dict(g=None), dict(partials=None), dict(state=None), dict(n=0), dict(n=-4), dict(n=(1 << 40) + 1),
               dict(g=g.data_ptr() + 4, n=32), dict(g=g.data_ptr() + 8, n=32),
               dict(c=0.0), dict(c=-1.0), dict(c=float("nan")), dict(c=float("-inf")),
               dict(gs=float("nan")), dict(gs=float("inf")), dict(gs=float("-inf"))):
        assert call(**kw) == -1, kw
        assert _lib.last_error().startswith("grad_clip_coef"), kw
    torch.cuda.synchronize()
    assert torch.equal(sc.pbuf, before_p) and torch.equal(sc.sbuf, before_s)
    assert call() == 0 and call(c=float("inf")) == 0
    torch.cuda.synchronize()
    assert sc.state.tolist() == [8.0, 1.0, 0.0, 1.0] and sc.intact()


# ================================================================================================================
# qarig_adam_clip_step
# ================================================================================================================
def _inputs(n, case, steps=C.STEPS):
    """Device inputs in the shape of grad_clip_cases.make_inputs: p at the case's scale (0, -0 and +-scale in
    front), an EMA off the parameters, unit Gaussian gradients with a tenth exact zeros, the second a quarter."""
    g = torch.Generator(device="cuda").manual_seed(2000 + case["seed"] + n)
    s = float(case["scale"])
    p = torch.randn(n, device="cuda", generator=g) * s
    p[:4] = torch.tensor([0.0, -0.0, s, -s], device="cuda")[:min(4, n)]
    ema = p + torch.randn(n, device="cuda", generator=g) * (1e-2 * s)
    grads = []
    for t in range(steps):
        x = torch.randn(n, device="cuda", generator=g)
        x[torch.rand(n, device="cuda", generator=g) < 0.1] = 0.0
        grads.append(x * 0.25 if t == 1 else x)
    scalars = [A.step_scalars(t, A.LR, case["lam"], case["betas"], A.EMA_WS[(t - 1) % len(A.EMA_WS)])
               for t in range(1, steps + 1)]
    return dict(p=p, ema=ema, grads=grads, scalars=scalars, beta1=A.f32(case["betas"][0]),
                beta2=A.f32(case["betas"][1]), eps=A.f32(A.EPS))


def _clip_state(norm, coef):
    return torch.tensor([norm, coef, 0.0, 0.0], dtype=torch.float64, device="cuda")


@pytest.mark.parametrize("with_ema", [False, True])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("n", ADAM_SIZES + [BIG])
def test_coefficient_one_is_the_plain_entry_bit_for_bit(n, masked, with_ema):
    """qarig_adam_step / qarig_adam_ema_step without a mask, qarig_adamw_step with one; shadow on, grad_scale 0.5,
    the second step through dev_step."""
    from qarig import ops
    x = _inputs(n, CASES[3], steps=2)
    assert n < 2 or int(_bits(x["p"])[1]) == -2 ** 31                   # p = -0.0 is in
    mask = torch.from_numpy(A.masks(n, seed=5)["random"]).cuda() if masked else None
    state = _clip_state(123.0, 1.0)
    a = dict(p=x["p"].clone(), m=torch.zeros(n, device="cuda"), v=torch.zeros(n, device="cuda"),
             e=x["ema"].clone(), sh=torch.zeros(n, dtype=torch.bfloat16, device="cuda"))
    b = {k: t.clone() for k, t in a.items()}
    for t, (grad, s) in enumerate(zip(x["grads"], x["scalars"])):
        dev = None
        host = (s["step_size"], s["bc2_sqrt"], s["ema_w"], s["decay"])
        if t == 1:
            dev = torch.tensor(host, device="cuda")
            host = (7.0, 0.125, 0.77, 0.5)
        if masked:
            ops.adamw_step(a["p"], grad, a["m"], a["v"], a["e"] if with_ema else None, mask, x["beta1"], x["beta2"],
                           x["eps"], *host, 0.5, dev_step=dev, shadow=a["sh"])
        elif with_ema:
            ops.adam_ema_step(a["p"], grad, a["m"], a["v"], a["e"], x["beta1"], x["beta2"], x["eps"], *host[:3], 0.5,
                              dev_step=None if dev is None else dev[:3], shadow=a["sh"])
        else:
            ops.adam_step(a["p"], grad, a["m"], a["v"], x["beta1"], x["beta2"], x["eps"], *host[:2], 0.5,
                          dev_step=None if dev is None else dev[:2], shadow=a["sh"])
        ops.adam_clip_step(b["p"], grad, b["m"], b["v"], b["e"] if with_ema else None, mask, x["beta1"], x["beta2"],
                           x["eps"], *host, state, 0.5, dev_step=dev, shadow=b["sh"])
        for k in ("p", "m", "v", "e"):
            assert _same_bits(a[k], b[k]), (k, t)
        assert torch.equal(a["sh"].view(torch.int16), b["sh"].view(torch.int16))
    assert not _same_bits(a["p"], x["p"])
    assert with_ema or _same_bits(b["e"], x["ema"])


def _chain(x, mask, with_ema, with_shadow, with_dev, grad_scale, max_norm):
    """STEPS pairs of launches (the norm, then the step) on padded buffers."""
    from qarig import ops
    n = x["p"].numel()
    sc = _Scratch()
    bp, p = _padded(x["p"])
    bm, m = _padded(torch.zeros(n, device="cuda"))
    bv, v = _padded(torch.zeros(n, device="cuda"))
    be, e = _padded(x["ema"]) if with_ema else (None, None)
    bs, sh = _padded_shadow(n) if with_shadow else (None, None)
    dev = torch.zeros(4, device="cuda") if with_dev else None
    steps, shadow_ok = [], True
    for grad, s in zip(x["grads"], x["scalars"]):
        host = s
        if with_dev:
            dev.copy_(torch.tensor([s["step_size"], s["bc2_sqrt"], s["ema_w"], s["decay"]]))
            host = dict(step_size=7.0, bc2_sqrt=0.125, ema_w=0.77, decay=0.5)        # must all be ignored
        ops.grad_clip_coef(grad, grad_scale, max_norm, sc.partials, sc.state)
        ops.adam_clip_step(p, grad, m, v, e, mask, x["beta1"], x["beta2"], x["eps"], host["step_size"],
                           host["bc2_sqrt"], host["ema_w"], host["decay"], sc.state, grad_scale, dev_step=dev,
                           shadow=sh)
        norm, coef = sc.state.tolist()[:2]
        steps.append(dict(p=p.clone(), m=m.clone(), v=v.clone(), ema=None if e is None else e.clone(), norm=norm,
                          coef=coef))
        if with_shadow:
            shadow_ok = shadow_ok and torch.equal(sh.view(torch.int16), p.to(torch.bfloat16).view(torch.int16))
    intact = all(_intact(b, n) for b in (bp, bm, bv, be, bs) if b is not None) and sc.intact()
    return steps, intact, shadow_ok, sc.state.tolist()


VARIANTS = [dict(with_shadow=False, with_dev=False, grad_scale=1.0),
            dict(with_shadow=True, with_dev=True, grad_scale=0.5),
            dict(with_shadow=True, with_dev=False, grad_scale=2.0 ** -10)]


def _check_against_ref(n, with_ema, mask_names, variants, case_of):
    worst = {"p": 0.0, "m": 0.0, "v": 0.0, "ema": 0.0}
    k = 0
    for name in mask_names:
        for var in variants:
            case = case_of(k)
            k += 1
            mask = None if name is None else torch.from_numpy(A.masks(n, seed=k)[name]).cuda()
            x = _inputs(n, case)
            max_norm = 0.5 * math.sqrt(n) * var["grad_scale"]
            got, intact, shadow_ok, state = _chain(x, mask, with_ema, var["with_shadow"], var["with_dev"],
                                                   var["grad_scale"], max_norm)
            for t, g in enumerate(got):
                assert g["coef"] == C.coef_def(g["norm"], max_norm)
                ref_norm = C.norm_ref64(x["grads"][t], var["grad_scale"])
                assert abs(g["norm"] - ref_norm) <= C.bound_norm(n) * ref_norm
            if n >= 2047:       # by construction the outer steps clip and the middle one does not
                assert [g["coef"] < 1 for g in got] == [True, False, True], [g["coef"] for g in got]
                assert state[2:] == [0.0, 2.0]
            ref = C.clip_adamw_ref64(x["p"], x["grads"], mask, x["scalars"], x["beta1"], x["beta2"], x["eps"],
                                     var["grad_scale"], max_norm, ema=x["ema"] if with_ema else None,
                                     coefs=[g["coef"] for g in got], norms=[g["norm"] for g in got])
            r = C.worst_ratios(ref, got)
            for key in worst:
                worst[key] = max(worst[key], r[key]) if r[key] == r[key] else float("nan")
            assert intact, (n, name, var)
            assert shadow_ok, (n, name, var)
            assert all(torch.isfinite(g[q]).all() for g in got[-1:] for q in ("p", "m", "v"))
    return worst


@pytest.mark.parametrize("with_ema", [False, True])
@pytest.mark.parametrize("n", ADAM_SIZES)
def test_clipped_chain_matches_fp64_definition(n, with_ema):
    """Three chained steps, the norm launch in front of each; no mask and every named mask, three variants (shadow /
    dev_step / grad_scale), the cases in rotation; the definition is fed the device's own coefficients."""
    worst = _check_against_ref(n, with_ema, [None, "zeros", "ones", "alternating", "first", "last", "random"],
                               VARIANTS, lambda k: CASES[k % len(CASES)])
    print("adam_clip n={} ema={}: worst / bound after {} steps  p {:.4f} (bound {:g})  m {:.4f} ({:g})  v {:.4f} "
          "({:g})  ema {:.4f} ({:g})  [x 2^-24 M]".format(n, int(with_ema), C.STEPS, worst["p"], C.bound_p(C.STEPS),
                                                          worst["m"], C.bound_m(C.STEPS), worst["v"],
                                                          C.bound_v(C.STEPS), worst["ema"], C.bound_ema(C.STEPS)))
    assert all(0.0 <= x <= 1.0 for x in worst.values()), worst
    assert worst["p"] > 0 or n < 2047


def test_clipped_chain_past_one_sweep_of_the_grid():
    worst = _check_against_ref(BIG, True, ["random"], VARIANTS[1:2], lambda k: CASES[5])
    print("adam_clip n={} ema=1: worst / bound  p {:.4f}  m {:.4f}  v {:.4f}  ema {:.4f}".format(
        BIG, worst["p"], worst["m"], worst["v"], worst["ema"]))
    assert all(0.0 <= x <= 1.0 for x in worst.values()), worst


@pytest.mark.parametrize("norm", [float("nan"), float("inf"), float("-inf")])
@pytest.mark.parametrize("n", [1, 9, 2049, 8 * 256 * 3 + 5, BIG])
def test_non_finite_norm_changes_no_byte(n, norm):
    """Whatever coefficient stands beside it: p (with -0.0), m, v, ema, the shadow and the canaries keep every bit,
    with and without mask, ema and dev_step."""
    from qarig import ops
    x = _inputs(n, CASES[2], steps=1)
    grad, s = x["grads"][0], x["scalars"][0]
    for with_ema, masked, with_dev, coef in ((True, True, True, 0.5), (False, False, False, 0.0),
                                             (True, False, False, 1.0)):
        bp, p = _padded(x["p"])
        bm, m = _padded(torch.randn(n, device="cuda"))
        bv, v = _padded(torch.rand(n, device="cuda"))
        be, e = _padded(x["ema"])
        bs, sh = _padded_shadow(n)
        sh.copy_(p)
        before = [b.clone() for b in (bp, bm, bv, be, bs)]
        mask = torch.ones((n + 7) // 8, dtype=torch.uint8, device="cuda") if masked else None
        dev = torch.tensor([s["step_size"], s["bc2_sqrt"], s["ema_w"], s["decay"]], device="cuda") if with_dev \
            else None
        ops.adam_clip_step(p, grad, m, v, e if with_ema else None, mask, x["beta1"], x["beta2"], x["eps"],
                           s["step_size"], s["bc2_sqrt"], s["ema_w"], s["decay"], _clip_state(norm, coef), 1.0,
                           dev_step=dev, shadow=sh)
        for b, was in zip((bp, bm, bv, be, bs), before):
            assert torch.equal(b, was)
        assert n < 2 or int(_bits(p)[1]) == -2 ** 31
    # the control: a finite norm with the same arguments moves everything
    ops.adam_clip_step(p, grad, m, v, e, mask, x["beta1"], x["beta2"], x["eps"], s["step_size"], s["bc2_sqrt"],
                       s["ema_w"], s["decay"], _clip_state(1.0, 1.0), 1.0, shadow=sh)
    assert not torch.equal(bp, before[0]) and _intact(bp, n) and _intact(bs, n)


def test_nothing_is_written_at_or_behind_n():
    for n in list(range(1, 26)) + [2041, 2042, 2043, 2044, 2045, 2046]:
        x = _inputs(n, CASES[1], steps=1)
        mask = torch.ones((n + 7) // 8, dtype=torch.uint8, device="cuda")
        got, intact, shadow_ok, _ = _chain(x, mask, True, True, False, 1.0, 0.5 * math.sqrt(n))
        assert intact and shadow_ok, n
        assert bool((got[0]["p"] != x["p"])[4:].all()), n


def test_adam_clip_step_refusals_launch_nothing():
    from qarig import _lib
    lib = _lib.load()
    n = 64
    base = torch.arange(7 * n, dtype=torch.float32, device="cuda")
    p, g, m, v, e = (base[k * n:(k + 1) * n] for k in range(1, 6))
    sh = torch.zeros(n, dtype=torch.bfloat16, device="cuda")
    mask = torch.ones(n // 8, dtype=torch.uint8, device="cuda")
    state = _clip_state(1.0, 1.0)
    before = base.clone()
    s = _lib.stream()

    def call(p=p.data_ptr(), g=g.data_ptr(), m=m.data_ptr(), v=v.data_ptr(), e=e.data_ptr(),
             mask=mask.data_ptr(), n=n, decay=1e-4, sh=sh.data_ptr(), state=state.data_ptr()):
        return lib.qarig_adam_clip_step(p, g, m, v, e, mask, n, 0.5, 0.999, 1e-8, 2e-3, 0.0316, 0.1, decay, 1.0, None,
                                        sh, state, s)

    for kw in (dict(p=None), dict(g=None), dict(m=None), dict(v=None), dict(state=None),
               dict(state=state.data_ptr() + 4),
               dict(n=0), dict(n=-8), dict(n=(1 << 40) + 1),
               dict(p=p.data_ptr() + 4, n=n - 8), dict(g=g.data_ptr() + 8, n=n - 8), dict(m=m.data_ptr() + 4, n=n - 8),
               dict(v=v.data_ptr() + 12, n=n - 8), dict(e=e.data_ptr() + 4, n=n - 8),
               dict(sh=sh.data_ptr() + 2, n=n - 8),
               dict(decay=-1e-4), dict(decay=1.0), dict(decay=float("nan")), dict(decay=float("inf")),
               dict(e=p.data_ptr()), dict(e=p.data_ptr() + 16), dict(e=p.data_ptr() + 4 * n - 16),
               dict(e=p.data_ptr() - 4 * n + 16),
               dict(sh=p.data_ptr()), dict(sh=p.data_ptr() + 4 * n - 16), dict(sh=p.data_ptr() - 2 * n + 16)):
        assert call(**kw) == -1, kw
        assert _lib.last_error().startswith("adam_clip"), kw
    torch.cuda.synchronize()
    assert _same_bits(base, before) and not sh.view(torch.int16).any()
    # the controls: nothing wrong; no optional buffer; no mask (the host decay is then not looked at)
    assert call() == 0
    assert call(e=None, sh=None) == 0
    assert call(mask=None, decay=float("nan")) == 0
    torch.cuda.synchronize()
    assert not _same_bits(base[n:2 * n], before[n:2 * n]) and _same_bits(base[2 * n:3 * n], before[2 * n:3 * n])
    assert _same_bits(base[:n], before[:n]) and _same_bits(base[6 * n:], before[6 * n:])
