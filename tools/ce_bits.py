"""SHA-256 of every output buffer of the cross-entropy entries and of qarig_token_score, through the C ABI alone (the
four older entries: qarig_cross_entropy_fwd, _ld_fwd, _reg_fwd, _soft_fwd), so the same file runs on any commit that
exports them.  tests/golden/ce_parent_bits.json is its output on the commit before the loss path was folded into one
row kernel and one launcher; tests/test_gpu_ce_bits.py recomputes it.  The build has -ffp-contract=off: a digest that
differs is an operation that changed, not noise.

Cases (tests/row_kernel_cases.py, ce_reg_cases.py, ce_soft_cases.py): ce_case(37, C), C in CLASSES, and
ce_case(257, 41, mixed=False), whose mean crosses 256 rows.
  plain   once per case
  ld      ld = ld_grad in {C, C + 3} (+ 528 at C = 513), NaN behind the classes; the whole (M, ld) gradient buffer
  reg     every point of REG_GRID, with dlogits and with NULL
  soft    every point of SOFT_GRID and SOFT_BITS_POINT, R in (1, 31), sigma = R / 2, codes = C - 1 (not at C = 3)
  score   qarig_token_score on the same logits, and with bad_targets()

    python tools/ce_bits.py --out tests/golden/ce_parent_bits.json --recorded-on <commit>
"""
import argparse
import hashlib
import json
import os
import sys

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
for p in (ROOT, os.path.join(ROOT, "quantized-autoregression-image-generator_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, os.path.abspath(p))

from ce_reg_cases import REG_GRID  # noqa: E402
from ce_soft_cases import SOFT_BITS_POINT, SOFT_GRID  # noqa: E402
from qarig import _lib  # noqa: E402
from row_kernel_cases import ce_case  # noqa: E402

CLASSES = (3, 64, 65, 257, 513)
SOFT_R = (1, 31)
NAN = float("nan")


def sha(t):
    return None if t is None else hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def cases():
    return [ce_case(37, C) for C in CLASSES] + [ce_case(257, 41, mixed=False)]


def digests():
    """{"<entry> M=.. C=.. <arguments>": {buffer: sha256 | None, "flag": int}} on the current device."""
    lib, s, P = _lib.load(), _lib.stream(), _lib.ptr
    dev = torch.device("cuda", torch.cuda.current_device())
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    out = {}

    def f32(*shape):
        return torch.full(shape, NAN, dtype=torch.float32, device=dev)

    def record(key, rc, **bufs):
        assert rc == 0, (key, rc, _lib.last_error())
        torch.cuda.synchronize()
        out[key] = {k: sha(v) for k, v in bufs.items()}
        out[key]["flag"] = int(flag.item())
        flag.zero_()

    for c in cases():
        M, C = c.M, c.C
        x, t = c.x.to(dev), c.t.to(dev)
        at = f"M={M} C={C}"
        loss, rows, dl = f32(1), f32(M), f32(M, C)
        record(f"plain {at}", lib.qarig_cross_entropy_fwd(P(x), P(t), M, C, P(loss), P(dl), P(rows), P(flag), s),
               loss=loss, row_ws=rows, dlogits=dl)
        for ld in (C, C + 3) + ((528,) if C == 513 else ()):
            buf = f32(M, ld)
            buf[:, :C] = x
            loss, rows, dl = f32(1), f32(M), f32(M, ld)
            record(f"ld {at} ld={ld}",
                   lib.qarig_cross_entropy_ld_fwd(P(buf), ld, P(t), M, C, P(loss), P(dl), ld, P(rows), P(flag), s),
                   loss=loss, row_ws=rows, dlogits=dl)
        for eps, zeta in REG_GRID:
            for grad in (True, False):
                loss, rows, dl = f32(2), f32(2 * M), (f32(M, C) if grad else None)
                record(f"reg {at} eps={eps} zeta={zeta} grad={int(grad)}",
                       lib.qarig_cross_entropy_reg_fwd(P(x), P(t), M, C, eps, zeta, P(loss), P(dl), P(rows), P(flag), s),
                       loss=loss, row_ws=rows, dlogits=dl)
        if C > 3:
            for R in SOFT_R:
                d = torch.arange(R + 1, dtype=torch.float64)
                w = torch.exp(-(d * d) / (2.0 * (R / 2.0) ** 2)).float().to(dev)
                for eps, zeta, nu in SOFT_GRID + (SOFT_BITS_POINT,):
                    loss, rows, dl = f32(2), f32(2 * M), f32(M, C)
                    record(f"soft {at} codes={C - 1} R={R} eps={eps} zeta={zeta} nu={nu}",
                           lib.qarig_cross_entropy_soft_fwd(P(x), P(t), M, C, C - 1, eps, zeta, nu, R, P(w), P(loss),
                                                            P(dl), P(rows), P(flag), s),
                           loss=loss, row_ws=rows, dlogits=dl)
        for name, tt in (("targets", t), ("bad_targets", c.bad_targets().to(dev))):
            nll, rank = f32(M), torch.full((M,), -7, dtype=torch.int32, device=dev)
            record(f"score {at} {name}", lib.qarig_token_score(P(x), P(tt), M, C, -100, P(nll), P(rank), P(flag), s),
                   row_nll=nll, row_rank=rank)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None, help="write the JSON here as well as to stdout")
    ap.add_argument("--recorded-on", default=None, help="the commit the library was built from, kept in the file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    torch.cuda.set_device(0)
    text = json.dumps({"recorded_on": args.recorded_on, "device": torch.cuda.get_device_name(0),
                       "digests": digests()}, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
