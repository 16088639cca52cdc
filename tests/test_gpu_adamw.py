"""qarig_adamw_step (csrc/optim.hip adam_groups_kernel) against its fp64 definition and against the plain Adam
entries: tolerances, inputs and masks from tests/adamw_cases.py, where the bounds are derived (and
tests/test_adamw_host.py shows the specified arithmetic meets them and seven wrong AdamWs do not)."""
import pytest
import torch

import adamw_cases as C

pytestmark = pytest.mark.gpu

SIZES = [1, 7, 8, 9, 15, 16, 17, 2047, 2048, 2049, 8 * 256 * 3 + 5]
BIG = 8192 * 256 * 8 + 8 + 3            # past one sweep of the capped grid, a full group behind it and a partial one
PAD = 32                                # canary elements behind every buffer
CANARY = 0x7FC0BEEF                     # a NaN with a payload
CANARY16 = 0x7FC1                       # (as int16) a bf16 NaN with a payload
CASES = list(C.cases())


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _padded(values):
    """A fresh buffer holding `values` followed by PAD canaries; returns (buffer as int32, the float view)."""
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


def _inputs(n, case, steps=C.STEPS):
    """Device inputs in the shape of adamw_cases.make_inputs: p at the case's scale (with 0, -0 and +-scale in
    front), an EMA off the parameters, unit Gaussian gradients with a tenth exact zeros."""
    g = torch.Generator(device="cuda").manual_seed(1000 + case["seed"] + n)
    s = float(case["scale"])
    p = torch.randn(n, device="cuda", generator=g) * s
    p[:4] = torch.tensor([0.0, -0.0, s, -s], device="cuda")[:min(4, n)]
    ema = p + torch.randn(n, device="cuda", generator=g) * (1e-2 * s)
    grads = []
    for _ in range(steps):
        x = torch.randn(n, device="cuda", generator=g)
        x[torch.rand(n, device="cuda", generator=g) < 0.1] = 0.0
        grads.append(x)
    scalars = [C.step_scalars(t, C.LR, case["lam"], case["betas"], C.EMA_WS[(t - 1) % len(C.EMA_WS)])
               for t in range(1, steps + 1)]
    return dict(p=p, ema=ema, grads=grads, scalars=scalars, beta1=C.f32(case["betas"][0]),
                beta2=C.f32(case["betas"][1]), eps=C.f32(C.EPS))


def _chain(x, mask, with_ema, with_shadow, with_dev, grad_scale):
    """STEPS launches on padded copies of x.  Returns (per-step dict(p, m, v, ema) of clones, canaries intact,
    shadow equals the nearest-even bf16 of p after every step)."""
    from qarig import ops
    n = x["p"].numel()
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
        ops.adamw_step(p, grad, m, v, e, mask, x["beta1"], x["beta2"], x["eps"], host["step_size"],
                       host["bc2_sqrt"], host["ema_w"], host["decay"], grad_scale, dev_step=dev, shadow=sh)
        steps.append(dict(p=p.clone(), m=m.clone(), v=v.clone(), ema=None if e is None else e.clone()))
        if with_shadow:
            shadow_ok = shadow_ok and torch.equal(sh.view(torch.int16), p.to(torch.bfloat16).view(torch.int16))
    intact = all(_intact(b, n) for b in (bp, bm, bv, be, bs) if b is not None)
    return steps, intact, shadow_ok


VARIANTS = [dict(with_shadow=False, with_dev=False, grad_scale=1.0),
            dict(with_shadow=True, with_dev=True, grad_scale=0.5),
            dict(with_shadow=True, with_dev=False, grad_scale=1.0)]


def _check_against_ref(n, with_ema, mask_names, variants, case_of):
    worst = {"p": 0.0, "m": 0.0, "v": 0.0, "ema": 0.0}
    k = 0
    for name in mask_names:
        for var in variants:
            case = case_of(k)
            k += 1
            mask = torch.from_numpy(C.masks(n, seed=k)[name]).cuda()
            x = _inputs(n, case)
            got, intact, shadow_ok = _chain(x, mask, with_ema, var["with_shadow"], var["with_dev"],
                                            var["grad_scale"])
            ref = C.adamw_ref64(x["p"], x["grads"], mask, x["scalars"], x["beta1"], x["beta2"], x["eps"],
                                var["grad_scale"], ema=x["ema"] if with_ema else None)
            r = C.worst_ratios(ref, got)
            for key in worst:
                worst[key] = max(worst[key], r[key]) if r[key] == r[key] else float("nan")
            assert intact, (n, name, var)
            assert shadow_ok, (n, name, var)
            assert all(torch.isfinite(t).all() for t in got[-1].values() if t is not None)
    return worst


@pytest.mark.parametrize("with_ema", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_adamw_matches_fp64_definition(n, with_ema):
    """Three chained steps, every mask, three variants (shadow / dev_step / grad_scale 0.5), the cases of
    adamw_cases.cases() in rotation (every scale, lambda and beta pair appears at every n)."""
    worst = _check_against_ref(n, with_ema, ["zeros", "ones", "alternating", "first", "last", "random"], VARIANTS,
                               lambda k: CASES[k % len(CASES)])
    print("adamw n={} ema={}: worst / bound after {} steps  p {:.4f} (bound {:g})  m {:.4f} ({:g})  v {:.4f} ({:g})"
          "  ema {:.4f} ({:g})  [x 2^-24 M]".format(n, int(with_ema), C.STEPS, worst["p"], C.bound_p(C.STEPS),
                                                     worst["m"], C.bound_m(C.STEPS), worst["v"],
                                                     C.bound_v(C.STEPS), worst["ema"], C.bound_ema(C.STEPS)))
    assert all(0.0 <= x <= 1.0 for x in worst.values()), worst
    assert worst["p"] > 0 or n < 2047            # (fp32 did round somewhere)


def test_adamw_past_one_sweep_of_the_grid():
    """n = 8192 * 256 * 8 + 8 + 3: the grid-stride loop wraps, by one full group and the partial one."""
    worst = _check_against_ref(BIG, True, ["random"], VARIANTS[1:2], lambda k: CASES[5])
    print("adamw n={} ema=1: worst / bound  p {:.4f}  m {:.4f}  v {:.4f}  ema {:.4f}".format(
        BIG, worst["p"], worst["m"], worst["v"], worst["ema"]))
    assert all(0.0 <= x <= 1.0 for x in worst.values()), worst


@pytest.mark.parametrize("with_ema", [False, True])
@pytest.mark.parametrize("n", SIZES + [BIG])
def test_mask_of_zeros_is_the_plain_launch_bit_for_bit(n, with_ema):
    from qarig import ops
    case = CASES[3]
    x = _inputs(n, case, steps=2)
    assert n < 2 or (float(x["p"][1]) == 0.0 and int(_bits(x["p"])[1]) == -2 ** 31)      # p = -0.0 is in
    mask = torch.zeros((n + 7) // 8, dtype=torch.uint8, device="cuda")
    a = dict(p=x["p"].clone(), m=torch.zeros(n, device="cuda"), v=torch.zeros(n, device="cuda"),
             e=x["ema"].clone(), sh=torch.zeros(n, dtype=torch.bfloat16, device="cuda"))
    b = {k: t.clone() for k, t in a.items()}
    for grad, s in zip(x["grads"], x["scalars"]):
        if with_ema:
            ops.adam_ema_step(a["p"], grad, a["m"], a["v"], a["e"], x["beta1"], x["beta2"], x["eps"], s["step_size"],
                              s["bc2_sqrt"], s["ema_w"], 0.5, shadow=a["sh"])
        else:
            ops.adam_step(a["p"], grad, a["m"], a["v"], x["beta1"], x["beta2"], x["eps"], s["step_size"],
                          s["bc2_sqrt"], 0.5, shadow=a["sh"])
        ops.adamw_step(b["p"], grad, b["m"], b["v"], b["e"] if with_ema else None, mask, x["beta1"], x["beta2"],
                       x["eps"], s["step_size"], s["bc2_sqrt"], s["ema_w"], s["decay"], 0.5, shadow=b["sh"])
        for k in ("p", "m", "v", "e"):
            assert _same_bits(a[k], b[k]), k
        assert torch.equal(a["sh"].view(torch.int16), b["sh"].view(torch.int16))
    assert not _same_bits(a["p"], x["p"])
    if n >= 2:
        # a -0.0 parameter with a zero gradient and zero moments stays -0.0 in both
        z = torch.zeros(n, device="cuda")
        q = [torch.full((n,), -0.0, device="cuda") for _ in range(2)]
        ops.adam_step(q[0], z, z.clone(), z.clone(), 0.5, 0.999, 1e-8, 2e-3, 0.0316)
        ops.adamw_step(q[1], z, z.clone(), z.clone(), None, mask, 0.5, 0.999, 1e-8, 2e-3, 0.0316, 0.0, 1e-4)
        assert _same_bits(q[0], q[1]) and int(_bits(q[1])[0]) == -2 ** 31


@pytest.mark.parametrize("name", ["ones", "alternating", "first", "last", "random"])
@pytest.mark.parametrize("n", [1, 9, 17, 2049, 8 * 256 * 3 + 5])
def test_zero_gradient_decays_the_masked_groups_exactly(n, name):
    """g = m = v = 0: the update is step_size * (0 / eps) = 0, so a decayed element becomes fma(-c, p, p) -- the
    product exact in double, one rounding to fp32 -- and every other element keeps its bits."""
    from qarig import ops
    x = _inputs(n, CASES[0], steps=1)
    mask_np = C.masks(n, seed=3)[name]
    mask = torch.from_numpy(mask_np).cuda()
    dec = C.element_mask(mask, n)
    c = C.f32(1e-3 * 0.1)
    p, z = x["p"].clone(), torch.zeros(n, device="cuda")
    m, v = z.clone(), z.clone()
    ops.adamw_step(p, z, m, v, None, mask, 0.5, 0.999, 1e-8, 2e-3, 0.0316, 0.0, c)
    want = torch.where(dec, (x["p"].double() * (-c) + x["p"].double()).float(), x["p"])
    assert _same_bits(p, want)
    assert _same_bits(p[~dec], x["p"][~dec])
    if n >= 8 and bool(dec.any()):
        assert not _same_bits(p[dec], x["p"][dec])
    assert not m.any() and not v.any()


def test_dev_step_values_override_the_host_values():
    from qarig import ops
    n = 2049
    x = _inputs(n, CASES[4], steps=1)
    mask = torch.from_numpy(C.masks(n)["alternating"]).cuda()
    s, grad = x["scalars"][0], x["grads"][0]
    runs = []
    for dev, host in ((None, (s["step_size"], s["bc2_sqrt"], s["ema_w"], s["decay"])),
                      (torch.tensor([s["step_size"], s["bc2_sqrt"], s["ema_w"], s["decay"]], device="cuda"),
                       (3.0, 0.5, 0.1, 0.25))):
        p, e, m, v = x["p"].clone(), x["ema"].clone(), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
        ops.adamw_step(p, grad, m, v, e, mask, x["beta1"], x["beta2"], x["eps"], *host, dev_step=dev)
        runs.append((p, e, m, v))
    for a, b in zip(*runs):
        assert _same_bits(a, b)
    # the host's decay is not even looked at with dev_step: one the entry would refuse passes
    p, m, v = x["p"].clone(), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    dev = torch.tensor([s["step_size"], s["bc2_sqrt"], 0.0, s["decay"]], device="cuda")
    ops.adamw_step(p, grad, m, v, None, mask, x["beta1"], x["beta2"], x["eps"], 3.0, 0.5, 0.1, 0.0, dev_step=dev)
    assert _same_bits(p, runs[0][0])              # (without an EMA dev_step[2] is ignored)
    # a different device decay gives different parameters: it is the device value that is read
    dev2 = torch.tensor([s["step_size"], s["bc2_sqrt"], 0.0, 2 * s["decay"]], device="cuda")
    p2, m2, v2 = x["p"].clone(), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    ops.adamw_step(p2, grad, m2, v2, None, mask, x["beta1"], x["beta2"], x["eps"], 3.0, 0.5, 0.1, 0.0, dev_step=dev2)
    assert not _same_bits(p2, p)


@pytest.mark.parametrize("with_ema", [False, True])
def test_nothing_is_written_at_or_behind_n(with_ema):
    """Every n % 8, below and above one group, all-ones mask, shadow on: the canaries behind p, m, v, ema and the
    shadow stay, and the elements in front of them all moved."""
    for n in list(range(1, 26)) + [2041, 2042, 2043, 2044, 2045, 2046]:
        x = _inputs(n, CASES[1], steps=1)
        mask = torch.ones((n + 7) // 8, dtype=torch.uint8, device="cuda")
        got, intact, shadow_ok = _chain(x, mask, with_ema, True, False, 1.0)
        assert intact and shadow_ok, n
        assert bool((got[0]["p"] != x["p"])[4:].all()), n         # (elements 0 and 1 are +-0: they may stay)


def test_refusals_return_an_error_and_launch_nothing():
    from qarig import _lib
    lib = _lib.load()
    n = 64
    base = torch.arange(7 * n, dtype=torch.float32, device="cuda")        # every pointer below stays inside it
    p, g, m, v, e = (base[k * n:(k + 1) * n] for k in range(1, 6))
    sh = torch.zeros(n, dtype=torch.bfloat16, device="cuda")
    mask = torch.ones(n // 8, dtype=torch.uint8, device="cuda")
    before = base.clone()
    s = _lib.stream()

    def call(p=p.data_ptr(), g=g.data_ptr(), m=m.data_ptr(), v=v.data_ptr(), e=e.data_ptr(),
             mask=mask.data_ptr(), n=n, decay=1e-4, sh=sh.data_ptr()):
        return lib.qarig_adamw_step(p, g, m, v, e, mask, n, 0.5, 0.999, 1e-8, 2e-3, 0.0316, 0.1, decay, 1.0, None,
                                    sh, s)

    for kw in (dict(p=None), dict(g=None), dict(m=None), dict(v=None), dict(mask=None),
               dict(n=0), dict(n=-8), dict(n=(1 << 40) + 1),
               dict(p=p.data_ptr() + 4, n=n - 8), dict(g=g.data_ptr() + 8, n=n - 8), dict(m=m.data_ptr() + 4, n=n - 8),
               dict(v=v.data_ptr() + 12, n=n - 8), dict(e=e.data_ptr() + 4, n=n - 8),
               dict(sh=sh.data_ptr() + 2, n=n - 8),
               dict(decay=-1e-4), dict(decay=1.0), dict(decay=float("nan")), dict(decay=float("inf")),
               dict(e=p.data_ptr()), dict(e=p.data_ptr() + 16), dict(e=p.data_ptr() + 4 * n - 16),
               dict(e=p.data_ptr() - 4 * n + 16),
               dict(sh=p.data_ptr()), dict(sh=p.data_ptr() + 4 * n - 16), dict(sh=p.data_ptr() - 2 * n + 16)):
        assert call(**kw) == -1, kw
        assert _lib.last_error().startswith("adamw"), kw
    torch.cuda.synchronize()
    assert _same_bits(base, before) and not sh.view(torch.int16).any()
    # the control: the same call with nothing wrong runs, with and without the optional buffers
    assert call() == 0
    assert call(e=None, sh=None) == 0
    torch.cuda.synchronize()
    assert not _same_bits(base[n:2 * n], before[n:2 * n]) and _same_bits(base[2 * n:3 * n], before[2 * n:3 * n])
    assert _same_bits(base[:n], before[:n]) and _same_bits(base[6 * n:], before[6 * n:])
