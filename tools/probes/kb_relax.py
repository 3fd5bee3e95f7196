#!/usr/bin/env python
"""abx_relax beside abx_clash_grad at the headline shape (B = 100 designs, L = 352, Lab = 228) in one process: HIP events around windows
of R calls, median of the windows.  The designs are the synthetic complex with every residue moved as a rigid body (0.3 A) and every
atom by 0.05 A; the movable set is the CDR-H3 segment (+ --flank linked neighbours on each side).
    python tools/probes/kb_relax.py [--B 100] [--workload L352] [--flank 0] [--iters 200]"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..'))
from abx_amd import ops, relax, synthetic  # noqa: E402

DEV = 'cuda:0'


def timeit(fn, calls=5, windows=7):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(windows):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / calls)
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--B', type=int, default=100)
    ap.add_argument('--workload', default='L352')
    ap.add_argument('--flank', type=int, default=0)
    ap.add_argument('--iters', type=int, default=200)
    a = ap.parse_args()
    cx = {k: v.to(DEV) for k, v in synthetic.make_complex(seed=2, **synthetic.WORKLOADS[a.workload]).items()}
    B, L, Lab = a.B, cx['seq'].shape[0], cx['anchor_flag'].shape[0]
    g = torch.Generator().manual_seed(23)
    x = cx['atom14_gt_positions'][None].repeat(B, 1, 1, 1)
    x[:, :Lab] += (0.3 * torch.randn(B, Lab, 1, 3, generator=g) + 0.05 * torch.randn(B, Lab, 14, 3, generator=g)).to(DEV)
    sq = cx['seq'][None].repeat(B, 1)
    rep = lambda k: cx[k][None].expand(B, *cx[k].shape).contiguous()
    exists, chain, residx, ft = rep('atom14_gt_exists'), rep('chain_id'), rep('residx'), x[:, :, 1].contiguous()
    t_g = timeit(lambda: ops.clash_grad(x, exists, sq, chain, ft, residx=residx), calls=20)
    print(f'B = {B}, L = {L}, Lab = {Lab}')
    print(f'abx_clash_grad                      {t_g[0]:9.3f} ms per call (windows {t_g[1]:.3f} .. {t_g[2]:.3f})')
    for iters in sorted({0, 20, a.iters}):
        r = relax.ViolationRelaxer(cx, movable=cx['cdr_def'] == 5, flank=a.flank, max_iter=iters)
        t_r = timeit(lambda: r.relax(x[:, :Lab], sq[:, :Lab]))
        h = r.relax(x[:, :Lab], sq[:, :Lab])[1].cpu()
        ev = h[:, 7]
        print(f'abx_relax M = {r.M:3d} max_iter = {iters:4d}   {t_r[0]:9.3f} ms per call (windows {t_r[1]:.3f} .. {t_r[2]:.3f}); evaluations {ev.min():.0f} .. '
              f'{ev.max():.0f} (mean {ev.mean():.1f}), E {h[:, :3].sum(1).mean():.2f} -> {h[:, 3:7].sum(1).mean():.2f}; '
              f'{1e3 * t_r[0] / float(ev.max()):.1f} us per evaluation of the longest structure; ratio to abx_clash_grad {t_r[0] / t_g[0]:.2f}')


if __name__ == '__main__':
    main()
