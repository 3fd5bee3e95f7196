#!/usr/bin/env python
"""abx_interface_scores beside abx_clash_grad and abx_design_scores at the headline shape (B = 100 designs, L = 352, Lab = 228) in one
process, for P = 128 and 960 sphere points: HIP events around windows of R calls, median of the windows.  abx_clash_grad walks the
same atom pairs in fp32 and forms gradients; the interface kernel adds the float64 point loop over each atom's neighbours.
    python tools/probes/kb_interface.py [--B 100] [--workload L352] [--points 128 960]"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..'))
from abx_amd import interface, metrics, ops, synthetic  # noqa: E402

DEV = 'cuda:0'


def timeit(fn, calls=10, windows=7):
    for _ in range(3):
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
    ap.add_argument('--points', type=int, nargs='+', default=[128, 960])
    ap.add_argument('--step_ms', type=float, default=596.0, help='time of one sampler step at this shape, for the share')
    a = ap.parse_args()
    cx = {k: v.to(DEV) for k, v in synthetic.make_complex(seed=2, **synthetic.WORKLOADS[a.workload]).items()}
    B, L, Lab = a.B, cx['seq'].shape[0], cx['anchor_flag'].shape[0]
    g = torch.Generator().manual_seed(23)
    # designs that still look like the complex: residues moved as a whole by 0.3 A, atoms by 0.05 A
    x = cx['atom14_gt_positions'][None] + (0.3 * torch.randn(B, L, 1, 3, generator=g) + 0.05 * torch.randn(B, L, 14, 3, generator=g)).to(DEV)
    sq = cx['seq'][None].repeat(B, 1)
    scorer = metrics.DesignScorer(cx)
    table = scorer.new_table(B)
    rep = lambda k: cx[k][None].expand(B, *cx[k].shape).contiguous()
    exists, chain, residx, ft = rep('atom14_gt_exists'), rep('chain_id'), rep('residx'), x[:, :, 1].contiguous()
    t_s = timeit(lambda: scorer.score(x[:, :Lab], sq[:, :Lab], out=table))
    t_g = timeit(lambda: ops.clash_grad(x, exists, sq, chain, ft, residx=residx))
    print(f'B = {B}, L = {L}, Lab = {Lab}')
    print(f'abx_design_scores             {t_s[0]:8.3f} ms per call (windows {t_s[1]:.3f} .. {t_s[2]:.3f})')
    print(f'abx_clash_grad                {t_g[0]:8.3f} ms per call (windows {t_g[1]:.3f} .. {t_g[2]:.3f})')
    for P in a.points:
        sc = interface.InterfaceScorer(cx, region=cx['cdr_def'] == 5, n_points=P)
        out = sc.new_table(B)
        t_i = timeit(lambda: sc.score(x[:, :Lab], sq[:, :Lab], out=out))
        h = out.cpu()
        print(f'abx_interface_scores P = {P:4d} {t_i[0]:8.3f} ms per call (windows {t_i[1]:.3f} .. {t_i[2]:.3f}); ratio to abx_clash_grad '
              f'{t_i[0] / t_g[0]:.2f}; {100 * t_i[0] / a.step_ms:.3f} % of a {a.step_ms:.0f} ms step; atoms {int(h[0, 11])}, '
              f'dsasa_int {float(h[:, 3].min()):.0f} .. {float(h[:, 3].max()):.0f}, contacts {int(h[:, 9].min())} .. {int(h[:, 9].max())}')


if __name__ == '__main__':
    main()
