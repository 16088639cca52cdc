"""Inputs, fp64 reference, error measure and tolerances shared by tests/test_gpu_attention_selectors.py (the
training attention kernels on an MI355X) and tests/test_attention_selectors_host.py (the same pieces on the CPU).

SELECTOR INPUTS.  For head dim d: b = min(d - 1, 10) code bits, gain = the smallest power of two >= 12 sqrt(d).
Key j holds the low b bits of j as +-1 in columns 0..b-1, 1 in column b and random integers of [-3, 3] behind it;
query i of head h holds gain * code(pi(i)) for its target key pi(i), -gain * b ("shifted") or +gain * b ("offset")
in column b and zeros behind it.  The raw score is -2 gain hamming(code(j), code(pi)) when shifted and 2 gain b
higher when offset: exact in fp32 and in bf16, adjacent Hamming levels >= 24 nats apart after the 1/sqrt(d) scale.
So every row attends with equal weight to the visible keys nearest to its target, everything else carries < 1e-7 of
the row (S <= 257), the unnormalised probabilities are 1 or ~0 and the online-softmax rescale factor is 0 or 1; v and
dO are integers of [-8, 8], so a dropped, duplicated or leaked key is a wrong small-integer average.

MEASURE.  Per row (n, head, position): max_c |got - ref| over the row's largest absolute-sum scale, i.e. the same
contraction with absolute values of its terms in fp64 (P|V| for o, |dS|_abs |K| / sqrt(d) for dq with
|dS|_abs = P (|dO||V|^T + sum_c |dO| (P|V|)), the transposed forms for dk and dv), floored (1 on the integer selector
data).  A largest-value-of-the-row denominator fails through the reference alone where a gradient row cancels.  The
log-sum-exp is compared in natural units relative to max(1, |ref|).

TOLERANCES, u = 2^-24, L2 = max(1, max|lse_ref| / ln 2), X2 = max(1, max over visible pairs of
sum_c |q_c k_c| log2(e) / sqrt(d)):
    selector, fp32 families   o, lse 8u;  dq, dk, dv (8 + 2 L2) u   (the backward recomputes p = exp2(s c2 - L) from
                                                                     a stored fp32 L: its rounding is in the exponent)
    selector, bf16 products   o, lse 8u;  dq, dk, dv 2^-7            (bf16 roundings of 2^-9 on p and on dS, x2 margin)
    Gaussian, fp32 families   all five (8 + 4 X2) u                  (the score rounding scales with the absolute score)
They come from the number formats, not from what the kernels give, and are not to be widened."""
import functools
import math
import zlib

import torch

U = 2.0 ** -24
LN2 = math.log(2.0)
PATTERNS = ("diag", "next", "first", "last", "rand")
OUTPUTS = ("o", "lse", "dq", "dk", "dv")
HEAD_CYCLE = (1, 3, 5, 6)        # one head, a ragged head group, a second (ragged) group, a second group of two
CAUSAL_LENGTHS = (1, 3, 16, 63, 64, 65, 129, 200, 257)
CROSS_SHAPES = ((1, 200), (130, 1), (65, 257), (200, 63))
N_BATCH = 2


def selector_params(d):
    """(b, gain) of head dim d."""
    assert d >= 4
    gain = 1
    while gain < 12.0 * math.sqrt(d):
        gain *= 2
    return min(d - 1, 10), gain


def _seed(*key):
    return zlib.crc32(repr(key).encode())


def _code(j, b):
    """(...,) integer tensor -> (..., b) of +-1: the low b bits."""
    bits = (j[..., None] >> torch.arange(b)) & 1
    return (2 * bits - 1).double()


def selector_targets(pattern, N, Sq, Sk, H, gen):
    """(N, H, Sq) target keys.  Head h shifts the pattern by h so that heads differ, in the direction that keeps what
    the pattern is for under the causal mask: `diag` moves back (still visible), `next` moves on (still masked)."""
    i = torch.arange(Sq)[None, None, :]
    h = torch.arange(H)[None, :, None]
    if pattern == "diag":
        t = i - h
    elif pattern == "next":
        t = i + 1 + h
    elif pattern == "first":
        t = h + 0 * i
    elif pattern == "last":
        t = Sk - 1 - h + 0 * i
    elif pattern == "rand":
        return torch.randint(0, Sk, (N, H, Sq), generator=gen)
    else:
        raise ValueError(pattern)
    return (t % Sk).expand(N, H, Sq).contiguous()


def build_selector(Sq, Sk, H, d, pattern, offset, N=N_BATCH):
    """fp64 q (N,H,Sq,d), k, v (N,H,Sk,d), dO (N,H,Sq,d) in head layout and the targets (N,H,Sq)."""
    b, gain = selector_params(d)
    gen = torch.Generator().manual_seed(_seed("selector", Sq, Sk, H, d, pattern, offset))
    pi = selector_targets(pattern, N, Sq, Sk, H, gen)
    k = torch.zeros((N, H, Sk, d), dtype=torch.float64)
    k[..., :b] = _code(torch.arange(Sk), b)
    k[..., b] = 1.0
    if d > b + 1:
        k[..., b + 1:] = torch.randint(-3, 4, (N, H, Sk, d - b - 1), generator=gen).double()
    q = torch.zeros((N, H, Sq, d), dtype=torch.float64)
    q[..., :b] = gain * _code(pi, b)
    q[..., b] = (gain * b) if offset else -(gain * b)
    v = torch.randint(-8, 9, (N, H, Sk, d), generator=gen).double()
    do = torch.randint(-8, 9, (N, H, Sq, d), generator=gen).double()
    return q, k, v, do, pi


def build_gaussian(Sq, Sk, H, d, N=N_BATCH):
    """q, k ~ 3 randn, v, dO ~ randn, rounded to fp32 (what the kernels are given), as fp64 in head layout."""
    gen = torch.Generator().manual_seed(_seed("gauss", Sq, Sk, H, d))
    q = 3 * torch.randn((N, H, Sq, d), generator=gen)
    k = 3 * torch.randn((N, H, Sk, d), generator=gen)
    v = torch.randn((N, H, Sk, d), generator=gen)
    do = torch.randn((N, H, Sq, d), generator=gen)
    return tuple(t.double() for t in (q, k, v, do))


def to_rows(t):
    """head layout (N,H,S,d) -> the kernels' (N,S,H*d), fp32."""
    N, H, S, d = t.shape
    return t.permute(0, 2, 1, 3).reshape(N, S, H * d).float().contiguous()


def to_heads(t, H):
    """(N,S,H*d) -> fp64 head layout (N,H,S,d) on the CPU."""
    N, S, D = t.shape
    return t.detach().double().cpu().reshape(N, S, H, D // H).permute(0, 2, 1, 3)


def _mask(Sq, Sk):
    return torch.triu(torch.ones(Sq, Sk, dtype=torch.bool), 1)


def reference(q, k, v, do, causal):
    """fp64 attention forward and backward in closed form on head-layout tensors.  Returns
    ref  {o, lse (natural units), dq, dk, dv},
    scale {o, dq, dk, dv}: per row, the largest absolute-sum contraction (see the module docstring),
    and P (N,H,Sq,Sk)."""
    d = q.shape[-1]
    Sq, Sk = q.shape[2], k.shape[2]
    rs = 1.0 / math.sqrt(d)
    s = q @ k.transpose(-1, -2) * rs
    if causal:
        s = s.masked_fill(_mask(Sq, Sk), float("-inf"))
    lse = torch.logsumexp(s, -1)
    P = torch.exp(s - lse[..., None])
    o = P @ v
    dP = do @ v.transpose(-1, -2)
    delta = (do * o).sum(-1, keepdim=True)
    dS = P * (dP - delta)
    ref = {"o": o, "lse": lse, "dq": dS @ k * rs, "dk": dS.transpose(-1, -2) @ q * rs, "dv": P.transpose(-1, -2) @ do}
    oa = P @ v.abs()
    dSa = P * (do.abs() @ v.abs().transpose(-1, -2) + (do.abs() * oa).sum(-1, keepdim=True))
    scale = {"o": oa, "dq": dSa @ k.abs() * rs, "dk": dSa.transpose(-1, -2) @ q.abs() * rs,
             "dv": P.transpose(-1, -2) @ do.abs()}
    scale = {n: t.amax(-1) for n, t in scale.items()}
    return ref, scale, P


def autograd_reference(q, k, v, do, causal):
    """The same five tensors from torch's softmax and autograd in fp64 (the check of `reference` itself)."""
    d = q.shape[-1]
    a = [t.clone().requires_grad_(True) for t in (q, k, v)]
    s = a[0] @ a[1].transpose(-1, -2) / math.sqrt(d)
    if causal:
        s = s.masked_fill(_mask(q.shape[2], k.shape[2]), float("-inf"))
    o = torch.softmax(s, -1) @ a[2]
    (o * do).sum().backward()
    return {"o": o.detach(), "lse": torch.logsumexp(s.detach(), -1), "dq": a[0].grad, "dk": a[1].grad, "dv": a[2].grad}


def row_errors(got, ref, scale, floor):
    """{output: worst row error}: max_c |got - ref| / max(floor, scale of the row); lse relative to max(1, |ref|)."""
    out = {}
    for name, g in got.items():
        if name == "lse":
            e = (g - ref["lse"]).abs() / ref["lse"].abs().clamp_min(1.0)
        else:
            e = (g - ref[name]).abs().amax(-1) / scale[name].clamp_min(floor)
        out[name] = float(e.max())
    return out


def lse_bits(ref):
    """L2: the largest |lse| of the case in base-2 units, at least 1."""
    return max(1.0, float(ref["lse"].abs().max()) / LN2)


def score_bits(q, k, causal):
    """X2: the largest absolute score sum_c |q_c k_c| log2(e) / sqrt(d) over the visible pairs, at least 1."""
    a = q.abs() @ k.abs().transpose(-1, -2)
    if causal:
        a = a.masked_fill(_mask(q.shape[2], k.shape[2]), 0.0)
    return max(1.0, float(a.max()) / (LN2 * math.sqrt(q.shape[-1])))


def selector_tolerances(ref, lp):
    """{output: tolerance} on selector data; lp: the bf16-product instantiation."""
    grad = 2.0 ** -7 if lp else (8 + 2 * lse_bits(ref)) * U
    return {"o": 8 * U, "lse": 8 * U, "dq": grad, "dk": grad, "dv": grad}


def gaussian_tolerances(q, k, causal):
    t = (8 + 4 * score_bits(q, k, causal)) * U
    return {n: t for n in OUTPUTS}


class Case:
    """One input set with its fp64 reference; built once per parameter tuple and shared (never modified) by every
    test that runs a kernel on it."""

    def __init__(self, kind, Sq, Sk, H, d, causal, pattern=None, offset=False):
        self.kind, self.Sq, self.Sk, self.H, self.d, self.causal = kind, Sq, Sk, H, d, causal
        if kind == "selector":
            self.q, self.k, self.v, self.do, self.pi = build_selector(Sq, Sk, H, d, pattern, offset)
            self.floor = 1.0
        else:
            self.q, self.k, self.v, self.do = build_gaussian(Sq, Sk, H, d)
            self.pi, self.floor = None, 1e-30
        self.ref, self.scale, self.P = reference(self.q, self.k, self.v, self.do, causal)

    def tolerances(self, lp=False):
        if self.kind == "selector":
            return selector_tolerances(self.ref, lp)
        assert not lp
        return gaussian_tolerances(self.q, self.k, self.causal)

    def errors(self, got):
        """got: {output: fp64 head-layout tensor, lse in natural units}."""
        return row_errors(got, self.ref, self.scale, self.floor)


@functools.lru_cache(maxsize=None)
def selector_case(Sq, Sk, H, d, causal, pattern, offset):
    return Case("selector", Sq, Sk, H, d, causal, pattern, offset)


@functools.lru_cache(maxsize=None)
def gaussian_case(Sq, Sk, H, d, causal):
    return Case("gauss", Sq, Sk, H, d, causal)


def selector_mass(case):
    """Per row, the softmax mass on the visible keys nearest to the target in Hamming distance, and the spread of the
    probabilities among them: (min mass, max spread)."""
    b, _ = selector_params(case.d)
    j = torch.arange(case.Sk)
    ham = ((j[None, None, None, :] ^ case.pi[..., None]) & ((1 << b) - 1))
    cnt = torch.zeros_like(ham)
    for t in range(b):
        cnt += (ham >> t) & 1
    if case.causal:
        cnt = cnt.masked_fill(_mask(case.Sq, case.Sk), 1 << 20)
    tied = cnt == cnt.amin(-1, keepdim=True)
    mass = (case.P * tied).sum(-1)
    pt = torch.where(tied, case.P, torch.full_like(case.P, float("nan")))
    hi = torch.nan_to_num(pt, nan=-1.0).amax(-1)
    lo = torch.nan_to_num(pt, nan=2.0).amin(-1)
    return float(mass.min()), float((hi - lo).max())


def _fma32(a, b, c):
    """fl32(a * b + c) of fp32 tensors: the product of two fp32 values is exact in fp64, the one fp64 rounding of the
    sum lies 2^-29 below the fp32 one."""
    return (a.double() * b.double() + c.double()).float()


def _bf16(t):
    return t.bfloat16().float()


def restate_fp32(q, k, v, do, causal, family, scale_dim=None):
    """The kernels' formulation in fp32 torch ops on the CPU: base-2 softmax with c2 = fl(fl(log2 e) / sqrt(d)), the
    log-sum-exp L saved in fp32 base-2 units, the backward's probabilities recomputed as exp2(fma(s, c2, -L)), the
    delta from the fp32 output.  family: "mfma" (csrc/attention.hip), "lp" (its bf16-product instantiation: operands,
    probabilities and score gradients rounded to bf16 on their way into a product) or "wide"
    (csrc/attention_wide.hip: the forward rounds s * c2 before subtracting the maximum).  One pass over the row, not
    the online form: on what the tolerances cover (roundings of the scores, of L and of the sums) the two agree.
    Returns {o, lse (natural units), dq, dk, dv} as fp64."""
    lp = family == "lp"
    d = scale_dim or q.shape[-1]
    sqrt_d = torch.tensor(float(d ** 0.5), dtype=torch.float32)
    c2 = torch.tensor(1.4426950408889634, dtype=torch.float32) / sqrt_d
    rsd = torch.tensor(1.0, dtype=torch.float32) / sqrt_d
    q, k, v, do = (t.float() for t in (q, k, v, do))
    op = _bf16 if lp else (lambda t: t)
    s = op(q) @ op(k).transpose(-1, -2)
    mask = _mask(q.shape[2], k.shape[2]) if causal else None
    sm = s.masked_fill(mask, float("-inf")) if causal else s
    if family == "wide":
        t = s * c2
        m = (t.masked_fill(mask, float("-inf")) if causal else t).amax(-1, keepdim=True)
        p = torch.exp2(t - m)
    else:
        m = sm.amax(-1, keepdim=True) * c2
        p = torch.exp2(_fma32(s, c2, -m))
    if causal:
        p = p.masked_fill(mask, 0.0)
    l = p.sum(-1, keepdim=True)
    # the output is normalised by the sum of the probabilities that enter the PV product (the rounded ones under bf16)
    o = (op(p) @ op(v)) * (1.0 / op(p).sum(-1, keepdim=True))
    L = m + torch.log2(l)
    pb = torch.exp2(_fma32(s, c2, -L))
    if causal:
        pb = pb.masked_fill(mask, 0.0)
    dl = (do * o).sum(-1, keepdim=True)
    ds = pb * (op(do) @ op(v).transpose(-1, -2) - dl)
    dq = (op(ds) @ op(k)) * rsd
    dk = (op(ds).transpose(-1, -2) @ op(q)) * rsd
    dv = op(pb).transpose(-1, -2) @ op(do)
    return {"o": o.double(), "lse": L[..., 0].double() * LN2, "dq": dq.double(), "dk": dk.double(), "dv": dv.double()}


def selector_shapes(d):
    """[(Sq, Sk, causal, H, offset)] of head dim d: the full list at d = 8 and 128, {3, 65, 129} and one cross shape at
    the other instantiated head dims, {65, 129} at the padded ones; heads cycle through HEAD_CYCLE; the offset form at
    one length per head dim."""
    if d in (8, 128):
        shapes = [(S, S, True) for S in CAUSAL_LENGTHS] + [(a, b, False) for a, b in CROSS_SHAPES]
    elif d in (4, 16, 32, 64):
        shapes = [(3, 3, True), (65, 65, True), (129, 129, True), (65, 257, False)]
    else:
        shapes = [(65, 65, True), (129, 129, True)]
    out = [(Sq, Sk, c, HEAD_CYCLE[n % 4], False) for n, (Sq, Sk, c) in enumerate(shapes)]
    out.append((129, 129, True, HEAD_CYCLE[len(shapes) % 4], True))
    return out


GAUSSIAN_SHAPES = ((70, 70, True, 3, 4), (130, 130, True, 5, 8), (200, 200, False, 6, 8), (129, 129, True, 3, 16),
                   (67, 67, True, 5, 64), (65, 65, True, 3, 128), (257, 257, True, 1, 8))     # Sq, Sk, causal, H, d
