"""The row-fused triangle attention under its three z-touch schedules (ops.tri_row_touch: 0 none, 1 whole next row a phase ahead, 2 per
k-group just in time), alternated launch by launch in ONE process on live data (random z, bias maps and a key mask; not constant
operands), both orientations.  Prints median and minimum per setting and checks that the three give equal bits.
    python tools/probes/kb_tri_touch.py [Bc] [L] [rounds]"""
import os
import sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from abx_amd import ops
DEV = 'cuda:0'
Bc = int(sys.argv[1]) if len(sys.argv) > 1 else 100
L = int(sys.argv[2]) if len(sys.argv) > 2 else 352
rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 7
LL, M2, C = L * L, Bc * L * L, 192
ge = torch.Generator().manual_seed(11)
W = lambda n: (torch.randn(n, C, generator=ge) / C ** 0.5).to(DEV)
b = lambda n: (torch.randn(n, generator=ge) * 0.3).to(DEV)
ln = ((1.0 + 0.2 * torch.randn(C, generator=ge)).to(DEV), (0.1 * torch.randn(C, generator=ge)).to(DEV))
rowp = ops.TriRowPack(ops.LinearPack([(W(C), b(C), 0), (W(C), b(C), 0), (W(C), b(C), 0)], C, ln=ln))
z = torch.randn(Bc, LL, C, device=DEV) * 1.3 + 0.2
Lp = (L + 3) // 4 * 4
bias = torch.zeros(Bc, 4, L, Lp, device=DEV)
bias[..., :L] = torch.randn(Bc, 4, L, L, device=DEV) * 150.0
mask = (torch.rand(Bc, L, device=DEV) > 0.1).float()
mask[:, 0] = 1
outs = [torch.empty(M2, C, device=DEV) for _ in range(2)]
start = ops.tri_row_touch()
for per_row in (True, False):
    ts = {0: [], 1: [], 2: []}

    def run(touch, o):
        ops.tri_row_touch(touch)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ops.tri_attn(z.view(M2, C), bias, mask, o, Bc, L, per_row, bias_is_qk=True, bias_log2=True, rowpack=rowp)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)
    run(1, outs[0])
    equal = True
    for r in range(rounds):
        for touch in ((1, 2, 0), (2, 0, 1), (0, 1, 2))[r % 3]:
            ts[touch].append(run(touch, outs[1] if touch != 1 else outs[0]))
            if touch != 1:
                equal = equal and torch.equal(outs[0], outs[1])
    line = f'Bc={Bc} L={L} per_row={per_row} ({rounds} rounds, alternating):'
    for touch in (0, 1, 2):
        t = sorted(ts[touch])
        line += f'   touch {touch}: median {t[len(t) // 2]:7.3f} min {t[0]:7.3f} ms'
    print(line + f'   equal bits: {equal}', flush=True)
ops.tri_row_touch(start)
