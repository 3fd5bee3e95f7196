#!/usr/bin/env python
"""abx_polar_scores beside abx_interface_scores (P = 128) and abx_design_scores at the headline shape (B = 100 designs, L = 352,
Lab = 228) in one process: HIP events around windows of R calls, median of the windows.  The polar kernel walks every pair of polar
atoms once in float64 (about 10^6 tests per structure); the interface kernel adds the sphere-point loop over each atom's neighbours.
    python tools/probes/kb_polar.py [--B 100] [--workload L352] [--points 128]"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..'))
from abx_amd import interface, metrics, polar, synthetic  # noqa: E402

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
    ap.add_argument('--points', type=int, default=128)
    ap.add_argument('--step_ms', type=float, default=596.0, help='time of one sampler step at this shape, for the share')
    a = ap.parse_args()
    cx = {k: v.to(DEV) for k, v in synthetic.make_complex(seed=2, **synthetic.WORKLOADS[a.workload]).items()}
    B, L, Lab = a.B, cx['seq'].shape[0], cx['anchor_flag'].shape[0]
    g = torch.Generator().manual_seed(23)
    # designs that still look like the complex: residues moved as a whole by 0.3 A, atoms by 0.05 A
    x = cx['atom14_gt_positions'][None] + (0.3 * torch.randn(B, L, 1, 3, generator=g) + 0.05 * torch.randn(B, L, 14, 3, generator=g)).to(DEV)
    sq = cx['seq'][None].repeat(B, 1)
    xa, sa = x[:, :Lab], sq[:, :Lab]
    scorer = metrics.DesignScorer(cx)
    table = scorer.new_table(B)
    it = interface.InterfaceScorer(cx, region=cx['cdr_def'] == 5, n_points=a.points)
    po = polar.PolarScorer(cx, interface=it)
    iout, pout, pts = it.new_table(B), po.new_table(B), po.new_points(B)
    it.score(xa, sa, out=iout, points=pts)
    t_s = timeit(lambda: scorer.score(xa, sa, out=table))
    t_i = timeit(lambda: it.score(xa, sa, out=iout, points=pts))
    t_p = timeit(lambda: po.score(xa, sa, out=pout, points=pts))
    t_b = timeit(lambda: po.score(xa, sa, out=pout))
    h = pout.cpu()
    print(f'B = {B}, L = {L}, Lab = {Lab}, P = {a.points}')
    print(f'abx_design_scores                 {t_s[0]:8.3f} ms per call (windows {t_s[1]:.3f} .. {t_s[2]:.3f})')
    print(f'abx_interface_scores              {t_i[0]:8.3f} ms per call (windows {t_i[1]:.3f} .. {t_i[2]:.3f})')
    print(f'abx_polar_scores (points given)   {t_p[0]:8.3f} ms per call (windows {t_p[1]:.3f} .. {t_p[2]:.3f}); ratio to abx_interface_scores '
          f'{t_p[0] / t_i[0]:.2f}; {100 * t_p[0] / a.step_ms:.4f} % of a {a.step_ms:.0f} ms step')
    print(f'surface + abx_polar_scores        {t_b[0]:8.3f} ms per call (windows {t_b[1]:.3f} .. {t_b[2]:.3f})')
    print(f'polar atoms {int(h[0, 13])}, hbond_total {int(h[:, 12].min())} .. {int(h[:, 12].max())}, hbond_int {int(h[:, 0].min())} .. '
          f'{int(h[:, 0].max())}, salt_int {int(h[:, 4].min())} .. {int(h[:, 4].max())}, unsat {int(h[:, 8].min())} .. {int(h[:, 8].max())}')


if __name__ == '__main__':
    main()
