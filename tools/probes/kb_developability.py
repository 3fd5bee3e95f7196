#!/usr/bin/env python
"""abx_developability_scores beside abx_interface_scores (P = 128) and abx_polar_scores at the headline shape (B = 100 designs, L = 352,
Lab = 228) in one process: HIP events around windows of R calls, median of the windows.  The pair kernel tests every counted atom of
the antibody against its weighted atoms in float64 (about 10^6 tests per structure); the interface kernel adds the sphere-point loop
over each atom's neighbours.
    python tools/probes/kb_developability.py [--B 100] [--workload L352] [--points 128] [--j_chunk 0]"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..'))
from abx_amd import developability, interface, polar, synthetic  # noqa: E402
from kb_polar import timeit  # noqa: E402

DEV = 'cuda:0'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--B', type=int, default=100)
    ap.add_argument('--workload', default='L352')
    ap.add_argument('--points', type=int, default=128)
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
    it = interface.InterfaceScorer(cx, region=cx['cdr_def'] == 5, n_points=a.points)
    po = polar.PolarScorer(cx, interface=it)
    dv = developability.DevelopabilityScorer(cx, interface=it)
    iout, pout, dout, pts = it.new_table(B), po.new_table(B), dv.new_table(B), dv.new_points(B)
    it.score(xa, sa, out=iout, points=pts)
    t_i = timeit(lambda: it.score(xa, sa, out=iout, points=pts))
    t_p = timeit(lambda: po.score(xa, sa, out=pout, points=pts))
    t_d = timeit(lambda: dv.score(xa, sa, out=dout, points=pts, j_chunk=a.j_chunk))
    t_b = timeit(lambda: dv.score(xa, sa, out=dout))
    h = dout.cpu()
    print(f'B = {B}, L = {L}, Lab = {Lab}, P = {a.points}, j_chunk = {a.j_chunk}')
    print(f'abx_interface_scores                      {t_i[0]:8.3f} ms per call (windows {t_i[1]:.3f} .. {t_i[2]:.3f})')
    print(f'abx_polar_scores (points given)           {t_p[0]:8.3f} ms per call (windows {t_p[1]:.3f} .. {t_p[2]:.3f})')
    print(f'abx_developability_scores (points given)  {t_d[0]:8.3f} ms per call (windows {t_d[1]:.3f} .. {t_d[2]:.3f}); ratio to '
          f'abx_interface_scores {t_d[0] / t_i[0]:.2f}; {100 * t_d[0] / a.step_ms:.4f} % of a {a.step_ms:.0f} ms step')
    print(f'surface + abx_developability_scores       {t_b[0]:8.3f} ms per call (windows {t_b[1]:.3f} .. {t_b[2]:.3f})')
    print(f'atoms {int(h[0, 20])}, sap_pos {float(h[:, 0].min()):.2f} .. {float(h[:, 0].max()):.2f}, sap_max_res {float(h[:, 3].min()):.3f} .. '
          f'{float(h[:, 3].max()):.3f}, n_liab {int(h[:, 17].min())} .. {int(h[:, 17].max())}, charge {int(h[0, 6])} / {int(h[0, 7])}')


if __name__ == '__main__':
    main()
