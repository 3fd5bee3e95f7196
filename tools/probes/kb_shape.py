#!/usr/bin/env python
"""abx_shape_scores beside abx_interface_scores and abx_polar_scores at the headline shape (B = 100 designs, L = 352, Lab = 228) in one
process, at P = 128 and 512 sphere points: HIP events around windows of R calls, median of the windows.  The shape kernels generate the
dots of the few hundred interface atoms again (the point test of the interface kernel on a tenth of the atoms), trim them against the open
dots of their side and search the nearest dot of the other side (all pairs of a few hundred to a few thousand dots, float64).
    python tools/probes/kb_shape.py [--B 100] [--workload L352] [--points 128 512] [--j_chunk 0]"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..'))
from abx_amd import interface, polar, shape, synthetic  # noqa: E402
from kb_polar import timeit  # noqa: E402

DEV = 'cuda:0'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--B', type=int, default=100)
    ap.add_argument('--workload', default='L352')
    ap.add_argument('--points', type=int, nargs='+', default=[128, 512])
    ap.add_argument('--j_chunk', type=int, default=0)
    ap.add_argument('--step_ms', type=float, default=596.0, help='time of one sampler step at this shape, for the share')
    a = ap.parse_args()
    cx = {k: v.to(DEV) for k, v in synthetic.make_complex(seed=2, **synthetic.WORKLOADS[a.workload]).items()}
    B, L, Lab = a.B, cx['seq'].shape[0], cx['anchor_flag'].shape[0]
    g = torch.Generator().manual_seed(23)
    # designs that still look like the complex: residues moved as a whole by 0.3 A, atoms by 0.05 A
    x = cx['atom14_gt_positions'][None] + (0.3 * torch.randn(B, L, 1, 3, generator=g) + 0.05 * torch.randn(B, L, 14, 3, generator=g)).to(DEV)
    sq = cx['seq'][None].repeat(B, 1)
    xa, sa = x[:, :Lab], sq[:, :Lab]
    for P in a.points:
        it = interface.InterfaceScorer(cx, region=cx['cdr_def'] == 5, n_points=P)
        po = polar.PolarScorer(cx, interface=it)
        sh = shape.ShapeScorer(cx, interface=it)
        iout, pout, sout, pts = it.new_table(B), po.new_table(B), sh.new_table(B), sh.new_points(B)
        it.score(xa, sa, out=iout, points=pts)
        t_i = timeit(lambda: it.score(xa, sa, out=iout, points=pts))
        t_p = timeit(lambda: po.score(xa, sa, out=pout, points=pts))
        t_s = timeit(lambda: sh.score(xa, sa, out=sout, points=pts, j_chunk=a.j_chunk))
        h = sout.cpu()
        print(f'B = {B}, L = {L}, Lab = {Lab}, P = {P}, j_chunk = {a.j_chunk}')
        print(f'abx_interface_scores              {t_i[0]:8.3f} ms per call (windows {t_i[1]:.3f} .. {t_i[2]:.3f})')
        print(f'abx_polar_scores (points given)   {t_p[0]:8.3f} ms per call (windows {t_p[1]:.3f} .. {t_p[2]:.3f})')
        print(f'abx_shape_scores (points given)   {t_s[0]:8.3f} ms per call (windows {t_s[1]:.3f} .. {t_s[2]:.3f}); ratio to '
              f'abx_interface_scores {t_s[0] / t_i[0]:.2f}; {100 * t_s[0] / a.step_ms:.4f} % of a {a.step_ms:.0f} ms step')
        print(f'sc {float(h[:, 0].min()):.4f} .. {float(h[:, 0].max()):.4f}, dots {int(h[:, 6].min())} .. {int(h[:, 6].max())} / '
              f'{int(h[:, 7].min())} .. {int(h[:, 7].max())}, trimmed {int(h[:, 9].min())} .. {int(h[:, 9].max())} / '
              f'{int(h[:, 10].min())} .. {int(h[:, 10].max())}')


if __name__ == '__main__':
    main()
