"""The pair Transition (relu(LN(z) W1 + b1) W2 + b2 + z, 192 -> 768 -> 192): the tile kernel gemm3_mlp_kernel<2> (tune 2048: one block per
128 rows, z walked once per hidden chunk) against the default dispatch (gemm_as_mlp_kernel of gemm_as.hip: one block per 64 rows, z split
once, chosen by the shape class at any M).  Same box, alternating in one process, live random data, out of place over B L^2 rows.
    python tools/probes/kb_mlp_as.py [B] [L] [alternations]"""
import os, sys, torch
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..'))
from abx_amd import ops
from tools.kbench import timeit
DEV = 'cuda:0'
B = int(sys.argv[1]) if len(sys.argv) > 1 else 100
L = int(sys.argv[2]) if len(sys.argv) > 2 else 352
alt = int(sys.argv[3]) if len(sys.argv) > 3 else 3
M = B * L * L
ops.RANGE_CHECK = False
r = lambda *s: torch.randn(*s, device=DEV)
z, out = r(M, 192) * 2 + 0.5, torch.empty(M, 192, device=DEV)
W1, W2 = r(192, 768) / 14, r(768, 192) / 28
W13, cs1, b1, W23, b2 = ops.split_weights(W1), W1.sum(0).contiguous(), r(768) * 0.1, ops.split_weights(ops.permute_k16(W2)), r(192) * 0.1
def mlp(tune):
    ops.gemm(z, W1, out, bias=b1, ln=(None, cs1), B3=W13, act=1, resid=z, exact=2, mlp=(W23, b2), tune=tune)
fl = 2.0 * M * 768 * (192 + 192)
for rep in range(alt):
    for name, tune in (('transition, tile kernel (tune 2048)', 2048), ('transition, default dispatch', 0)):
        ms = timeit(lambda: mlp(tune), reps=7)
        print(f'{name:40s} B={B} L={L} {ms:8.3f} ms  {fl / ms / 1e9:7.1f} TFLOP/s', flush=True)
