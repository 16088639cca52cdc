"""How v_mfma_scale_f32_32x32x64_f8f6f4 applies its scale bytes (run on the GPU box): qarig_gemm_mx on
small-integer e4m3 operands with scales constant, per row, per 32-block and random, against fp64.  It
showed that a lane's 32 fragment bytes are two 16-byte halves of two different 32-blocks of the
instruction's k (bytes 0-15 of lanes 0-31 and 32-63, then bytes 16-31), which f8_frag<true> follows."""
import os, sys, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "quantized-autoregression-image-generator_amd"))
from qarig import ops
F8 = torch.float8_e4m3fn
g = torch.Generator().manual_seed(0)
M = N = K = 128
Aq = torch.randint(-4, 5, (M, K), generator=g).float().to(F8).view(torch.uint8)
Bq = torch.randint(-4, 5, (N, K), generator=g).float().to(F8).view(torch.uint8)
def deq(q, s):
    return (q.view(F8).double().reshape(q.shape[0], -1, 32) * torch.pow(2.0, s.double() - 127)[..., None]).reshape(q.shape)
variants = {}
one = torch.full((M, K // 32), 127, dtype=torch.uint8)
rnd = lambda: torch.randint(125, 130, (M, K // 32), generator=g).to(torch.uint8)
rowc = torch.randint(125, 130, (M, 1), generator=g).to(torch.uint8).repeat(1, K // 32)
blkc = torch.randint(125, 130, (1, K // 32), generator=g).to(torch.uint8).repeat(M, 1)
variants["ones"] = (one, one)
variants["a128"] = (torch.full_like(one, 128), one)
variants["b128"] = (one, torch.full_like(one, 128))
variants["a_row"] = (rowc, one)
variants["a_blk"] = (blkc, one)
variants["b_row"] = (one, rowc)
variants["b_blk"] = (one, blkc)
variants["a_rnd"] = (rnd(), one)
variants["b_rnd"] = (one, rnd())
for name, (sa, sb) in variants.items():
    C = torch.full((M, N), float("nan"), device="cuda")
    ops.gemm_mx(ops.MxOperand(Aq.cuda(), sa.cuda()), ops.MxOperand(Bq.cuda(), sb.cuda()), M, N, K, C=C)
    C = C.cpu()
    want = deq(Aq, sa) @ deq(Bq, sb).t()
    ok = torch.equal(C.double(), want)
    print(name, "exact" if ok else "DIFF", float((C.double() - want).abs().max()), flush=True)
