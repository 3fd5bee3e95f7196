#!/usr/bin/env python
"""abx_patch_scores beside abx_developability_scores and abx_interface_scores (P = 128) at the headline shape (B = 100 designs, L = 352,
Lab = 228) in one process: HIP events around windows of R calls, median of the windows.  The pair kernel takes the closest heavy-atom
distance of every (antibody row, row) pair in float64 - 228 x 352 residue pairs of up to 196 atom pairs per structure, about 1.6 10^9
distances per call - and writes them to a (Lab, L) float64 plane that the last kernel reads once.
    python tools/kb_patches.py [--B 100] [--workload L352] [--points 128]"""
import argparse
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, '..'))
sys.path.insert(0, os.path.join(HERE, 'probes'))
from abx_amd import developability, interface, ops, patches, synthetic  # noqa: E402
from kb_polar import timeit  # noqa: E402

DEV = 'cuda:0'


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
    it = interface.InterfaceScorer(cx, region=cx['cdr_def'] == 5, n_points=a.points)
    dv = developability.DevelopabilityScorer(cx, interface=it)
    pa = patches.PatchScorer(cx, interface=it)
    iout, dout, pout, pts = it.new_table(B), dv.new_table(B), pa.new_table(B), pa.new_points(B)
    ws = torch.empty(ops.patch_workspace_bytes(B, L, Lab), dtype=torch.uint8, device=DEV)
    it.score(xa, sa, out=iout, points=pts)
    t_i = timeit(lambda: it.score(xa, sa, out=iout, points=pts))
    t_d = timeit(lambda: dv.score(xa, sa, out=dout, points=pts))
    t_p = timeit(lambda: pa.score(xa, sa, out=pout, points=pts, workspace=ws))
    t_a = timeit(lambda: pa.score(xa, sa, out=pout, points=pts))
    h = pout.cpu()
    print(f'B = {B}, L = {L}, Lab = {Lab}, P = {a.points}, workspace {ws.numel() / 2 ** 20:.1f} MiB')
    print(f'abx_interface_scores                      {t_i[0]:8.3f} ms per call (windows {t_i[1]:.3f} .. {t_i[2]:.3f})')
    print(f'abx_developability_scores (points given)  {t_d[0]:8.3f} ms per call (windows {t_d[1]:.3f} .. {t_d[2]:.3f})')
    print(f'abx_patch_scores (points given)           {t_p[0]:8.3f} ms per call (windows {t_p[1]:.3f} .. {t_p[2]:.3f}); ratio to '
          f'abx_interface_scores {t_p[0] / t_i[0]:.2f}; {100 * t_p[0] / a.step_ms:.4f} % of a {a.step_ms:.0f} ms step')
    print(f'abx_patch_scores, workspace allocated     {t_a[0]:8.3f} ms per call (windows {t_a[1]:.3f} .. {t_a[2]:.3f})')
    print(f'psh {float(h[:, 0].min()):.2f} .. {float(h[:, 0].max()):.2f}, ppc {float(h[:, 1].min()):.3f} .. {float(h[:, 1].max()):.3f}, pnc '
          f'{float(h[:, 2].min()):.3f} .. {float(h[:, 2].max()):.3f}, n_vicinity {int(h[:, 13].min())} .. {int(h[:, 13].max())}, n_pairs '
          f'{int(h[:, 14].min())} .. {int(h[:, 14].max())}, n_cross {int(h[:, 16].min())} .. {int(h[:, 16].max())}')


if __name__ == '__main__':
    main()
