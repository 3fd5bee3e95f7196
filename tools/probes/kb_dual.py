"""The tri-mul tail (dual GEMM: proj_out(LN product) x sigmoid(final_gate(LN z)) + z): the two-tile kernel (tune 2048) against the default
dispatch (the A-stationary kernel of gemm_as.hip from 1 024 blocks of 64 rows on; `as` forces it below that: tune 16384) - or, with `one`,
round 6's one block per 128-row tile (tune bit 7) against the two-tile kernel.  Same box, alternating, random data.
    python tools/probes/kb_dual.py [Bc] [L] [as|one]"""
import os, sys, torch
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..'))
from abx_amd import ops
from tools.kbench import timeit
DEV = 'cuda:0'
Bc = int(sys.argv[1]) if len(sys.argv) > 1 else 100
L = int(sys.argv[2]) if len(sys.argv) > 2 else 352
mode = sys.argv[3] if len(sys.argv) > 3 else ''
LL, Lp = L * L, (L + 3) // 4 * 4
pad = (L, Lp) if Lp != L else None          # L % 4 != 0: padded pair rows, as the network runs it
ops.RANGE_CHECK = False
r = lambda *s: torch.randn(*s, device=DEV)
tt, z, out = r(Bc, 128, L * Lp), r(Bc, LL, 192), torch.empty(Bc, LL, 192, device=DEV)
Wo, Wg = r(128, 192) / 11, r(192, 192) / 14
Wo3, cso, bo, Wg3, csg, bg = ops.split_weights(Wo), Wo.sum(0).contiguous(), r(192), ops.split_weights(Wg), Wg.sum(0).contiguous(), r(192)
def dual(tune):
    ops.gemm(tt.transpose(1, 2), Wo, out, bias=bo, ln=(None, cso), B3=Wo3, resid=z, pair=pad, c_pair=pad is not None, dual=(z, Wg3, csg, bg), exact=2, tune=tune)
fl = 2.0 * Bc * LL * 192 * 320
for rep in range(3):
    pairs = ((('dual, one block per row tile (tune 128)', 128), ('dual, two column tiles (tune 2048)', 2048)) if mode == 'one' else
             (('dual, two column tiles (tune 2048)', 2048), ('dual, A-stationary forced (tune 16384)', 16384) if mode == 'as' else ('dual, default dispatch', 0)))
    for name, tune in pairs:
        ms = timeit(lambda: dual(tune), reps=7)
        print(f'{name:44s} Bc={Bc} L={L} {ms:8.3f} ms  {fl / ms / 1e9:7.1f} TFLOP/s', flush=True)
