"""The head of the triangle-attention group at the bench geometry, per kernel: today's two launches (q | k | v projection with the pair bias in
its grid, tri_attn8 on the projected rows) against the row-fused route (the pair-bias projection alone, tri_attn8_rowfused on the z rows, both
slot orders).  Checks that the two routes give equal bits on the way.  python tools/probes/kb_tri_rowfused.py [Bc] [L] [reps]"""
import os
import sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from abx_amd import ops, _lib
from tools.kbench import timeit
DEV = 'cuda:0'
Bc = int(sys.argv[1]) if len(sys.argv) > 1 else 100
L = int(sys.argv[2]) if len(sys.argv) > 2 else 352
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 7
LL, M2, C = L * L, Bc * L * L, 192
ge = torch.Generator().manual_seed(7)
W = lambda n: (torch.randn(n, C, generator=ge) / C ** 0.5).to(DEV)
b = lambda n: (torch.randn(n, generator=ge) * 0.3).to(DEV)
ln = ((1.0 + 0.2 * torch.randn(C, generator=ge)).to(DEV), (0.1 * torch.randn(C, generator=ge)).to(DEV))
qkv = ops.LinearPack([(W(C), b(C), 0), (W(C), b(C), 0), (W(C), b(C), 0)], C, ln=ln)
pair = ops.LinearPack([(W(4), None, 0)], C, ln=ln)
rowp = ops.TriRowPack(qkv)
z = torch.randn(Bc, LL, C, device=DEV) * 1.3 + 0.2
mask = torch.ones(Bc, L, device=DEV)
rows = torch.empty(M2, 576, device=DEV)
bT = torch.empty(Bc, 4, LL, device=DEV)
bT2 = torch.empty(Bc, 4, L, L, device=DEV)
o0, o1 = torch.empty(M2, C, device=DEV), torch.empty(M2, C, device=DEV)
side = lambda: ops.gemm_side(ops.gemm(z.view(M2, C), qkv.Wt, rows, defer=True, bias=qkv.bias, ln=(None, qkv.csum), B3=qkv.planes, exact=2),
                             ops.gemm(z, pair.Wt, bT.transpose(1, 2), defer=True, bias=pair.bias, ln=(None, pair.csum), B3=pair.planes, exact=2, alpha=ops.TRI_BIAS_LOG2))
bias_only = lambda: ops.gemm(z, pair.Wt, bT.transpose(1, 2), bias=pair.bias, ln=(None, pair.csum), B3=pair.planes, exact=2, alpha=ops.TRI_BIAS_LOG2)
lib = _lib.LIB_PATH.split('/')[-1]
t_side = timeit(side, reps)
t_bias = timeit(bias_only, reps)
print(f'{lib}: Bc={Bc} L={L}   q|k|v + pair bias (one launch) {t_side:7.3f} ms   pair bias alone {t_bias:7.3f} ms', flush=True)
for per_row in (True, False):
    bias = bT.view(Bc, 4, L, L)
    if not per_row:
        ops.transpose_last2(bT.view(Bc * 4, L, L), bT2.view(Bc * 4, L, L), transpose=True)
        bias = bT2
    two = lambda: ops.tri_attn(rows, bias, mask, o0, Bc, L, per_row, bias_is_qk=True, bias_log2=True)
    t_two = timeit(two, reps)
    line = f'per_row={per_row}: tri_attn8 {t_two:7.3f} ms (head of the group: {t_side + t_two:7.3f})'
    for order in (0, 1):
        fused = lambda: ops.tri_attn(z.view(M2, C), bias, mask, o1, Bc, L, per_row, bias_is_qk=True, bias_log2=True, rowpack=rowp, slot_order=order)
        t_f = timeit(fused, reps)
        line += f'   rowfused order {order}: {t_f:7.3f} ms (head: {t_bias + t_f:7.3f}, equal bits: {torch.equal(o0, o1)})'
    print(line, flush=True)
