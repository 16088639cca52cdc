#!/usr/bin/env python3
"""Prices the parts of the fp32 ring k-loop (gemm_dma_pf_kernel / pf_ring in csrc/gemm.hip) by
compile-time ablation.

    python tools/gemm_ablation.py build        # CPU: one library per variant under lib/ablation/
    python tools/gemm_ablation.py run          # GPU: tools/gemm_bench.py against each variant
    python tools/gemm_ablation.py clock        # GPU: in-kernel clock from the stamps build

Each variant is csrc/gemm.hip compiled with the QARIG_RING_* defines below and linked with the
default build's other objects into lib/ablation/libqarig_<variant>.so; `run` starts tools/gemm_bench.py
in a fresh child process per variant (QARIG_LIB selects the library), in the order
base, variants..., base, so that drift over the run shows in the two base rows.  Results of the
ablation builds are wrong by design: only their times mean anything."""
import ctypes
import os
import re
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "quantized-autoregression-image-generator_amd")
sys.path.insert(0, PKG)

VARIANTS = {
    "base": [],
    "a_nodma": ["QARIG_RING_ABL_NODMA"],
    "b_nodma_nobar": ["QARIG_RING_ABL_NODMA", "QARIG_RING_ABL_NOBAR"],
    "c_noread": ["QARIG_RING_ABL_NOREAD"],
    "abc_mfma_loop": ["QARIG_RING_ABL_NODMA", "QARIG_RING_ABL_NOBAR", "QARIG_RING_ABL_NOREAD"],
    "d_noepi": ["QARIG_RING_ABL_NOEPI"],
    "stamps": ["QARIG_RING_STAMPS"],
}
ABL_DIR = os.path.join(PKG, "lib", "ablation")


def build():
    import build as qbuild
    qbuild.build_lib(verbose=False)
    os.makedirs(ABL_DIR, exist_ok=True)
    others = [os.path.join(qbuild.OBJ, f[:-4] + ".o") for f in sorted(os.listdir(qbuild.CSRC))
              if f.endswith(".hip") and f != "gemm.hip"]
    procs = []
    for name, defs in VARIANTS.items():
        obj = os.path.join(ABL_DIR, f"gemm_{name}.o")
        cmd = [qbuild.HIPCC, *qbuild.FLAGS, *[f"-D{d}" for d in defs], "-c", os.path.join(qbuild.CSRC, "gemm.hip"),
               "-o", obj]
        procs.append((name, obj, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)))
    for name, obj, p in procs:
        out = p.communicate()[0]
        if p.returncode:
            raise RuntimeError(f"{name}: hipcc failed\n{out}")
        so = os.path.join(ABL_DIR, f"libqarig_{name}.so")
        subprocess.run([qbuild.HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", so, obj, *others], check=True)
        print("built", so)


_LINE = re.compile(r"^(.{36}) M=.*median\s+([\d.]+) TF")


def _bench(name, rows):
    env = dict(os.environ, QARIG_LIB=os.path.join("ablation", f"libqarig_{name}.so"), ROWS=str(rows))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gemm_bench.py")], env=env,
                       capture_output=True, text=True, timeout=600)
    if r.returncode:
        raise RuntimeError(f"{name}: gemm_bench exited {r.returncode}\n{r.stdout}\n{r.stderr}")
    res = {}
    for line in r.stdout.splitlines():
        m = _LINE.match(line)
        if m:
            res[m.group(1).strip()] = float(m.group(2))
    return res


def run(rows=16384):
    order = ["base", "a_nodma", "b_nodma_nobar", "c_noread", "abc_mfma_loop", "d_noepi", "base"]
    table = []
    for name in order:
        table.append((name, _bench(name, rows)))
        print(f"done {name}", file=sys.stderr, flush=True)
    shapes = list(table[0][1])
    print("median TF (tools/gemm_bench.py, ROWS=%d)" % rows)
    print(f"{'shape':36s} " + " ".join(f"{n[:13]:>13s}" for n, _ in table))
    for s in shapes:
        print(f"{s:36s} " + " ".join(f"{r.get(s, float('nan')):13.1f}" for _, r in table))


def clock(seconds=3.0):
    """In-kernel clock of the ring k-loop: d(s_memtime) / d(s_memrealtime) x 100 MHz, per workgroup of the
    last launch after `seconds` of back-to-back launches on random data; median over workgroups."""
    os.environ["QARIG_LIB"] = os.path.join("ablation", "libqarig_stamps.so")
    import torch
    from qarig import _lib, ops
    lib = ctypes.CDLL(_lib.LIB_PATH)
    lib.qarig_ring_stamps_read.argtypes = [ctypes.c_void_p, ctypes.c_int]
    g = torch.Generator(device="cuda").manual_seed(0)
    cases = [("fwd 512->2048 plain", 16384, 2048, 512, True, True),
             ("dX  [M,2048]@[2048,512]", 16384, 512, 2048, True, False),
             ("dW  2048x512 over M (splitk)", 2048, 512, 16384, False, False)]
    for name, m, n, k, ak, bk in cases:
        A = torch.randn((m, k) if ak else (k, m), device="cuda", generator=g)
        B = torch.randn((n, k) if bk else (k, n), device="cuda", generator=g)
        sk = ops.pick_splitk(m, n, k) if not ak else 1
        t_end = time.time() + seconds
        while time.time() < t_end:
            for _ in range(20):
                ops.gemm(A, B, a_kcontig=ak, b_kcontig=bk, splitk=sk)
            torch.cuda.synchronize()
        buf = (ctypes.c_uint64 * (4 * 4096))()
        assert lib.qarig_ring_stamps_read(buf, 4096) == 0
        ghz = []
        for w in range(4096):
            c0, r0, c1, r1 = buf[4 * w:4 * w + 4]
            if r1 > r0:
                ghz.append((c1 - c0) / (r1 - r0) * 0.1)
        print(f"{name:32s} k-loop in-kernel clock: median {statistics.median(ghz):.3f} GHz "
              f"(min {min(ghz):.3f}, max {max(ghz):.3f}, {len(ghz)} workgroups)")


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "run"
    {"build": build, "run": run, "clock": clock}[what]()
