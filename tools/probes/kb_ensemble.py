#!/usr/bin/env python
"""abx_ensemble_pairs and abx_ensemble_cluster at N = 100 and N = 1000 designs (M = 13 and M = 64 compared residues, backbone: P = 52 and
256 points) beside abx_design_scores at the headline shape (B = 100 designs, L = 352) in one process: HIP events around windows of R
calls, median of the windows.
    python tools/probes/kb_ensemble.py [--workload L352]"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..'))
from abx_amd import ensemble, metrics, ops, synthetic  # noqa: E402

DEV = 'cuda:0'


def timeit(fn, calls=20, windows=7):
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
    ap.add_argument('--workload', default='L352')
    a = ap.parse_args()
    cx = {k: v.to(DEV) for k, v in synthetic.make_complex(seed=2, **synthetic.WORKLOADS[a.workload]).items()}
    L, Lab = cx['seq'].shape[0], cx['anchor_flag'].shape[0]
    g = torch.Generator().manual_seed(23)
    print(f'L = {L}, Lab = {Lab}')
    for N in (100, 1000):
        for M in (13, 64):
            # designs: a handful of base loops + 0.3 A noise, so that the clusters are neither one nor N
            base = cx['atom14_gt_positions'][None, :Lab] + 2.0 * torch.randn(7, Lab, 14, 3, generator=g).to(DEV)
            x = base[torch.arange(N, device=DEV) % 7] + 0.3 * torch.randn(N, Lab, 14, 3, generator=g).to(DEV)
            sq = cx['seq'][None, :Lab].repeat(N, 1)
            region = torch.zeros(Lab, dtype=torch.uint8, device=DEV)
            region[97:97 + M] = 1
            planes = torch.empty(3, N, N, dtype=torch.float64, device=DEV)
            t_p = timeit(lambda: ops.ensemble_pairs(x, sq, region, atoms=4, n_region=M, out=planes))
            t_c = timeit(lambda: ops.ensemble_cluster(planes, metric=0, cutoff=1.0))
            n = int(ops.ensemble_cluster(planes, metric=0, cutoff=1.0)[2])
            print(f'N = {N:4d}, M = {M:2d} (P = {4 * M:3d}), {n:3d} clusters: abx_ensemble_pairs {t_p[0]:8.3f} ms (windows {t_p[1]:.3f} .. {t_p[2]:.3f}), '
                  f'abx_ensemble_cluster {t_c[0]:8.3f} ms (windows {t_c[1]:.3f} .. {t_c[2]:.3f})')
    B = 100
    xs = cx['atom14_gt_positions'][None] + 0.7 * torch.randn(B, L, 14, 3, generator=g).to(DEV)
    sq = cx['seq'][None].repeat(B, 1)
    scorer = metrics.DesignScorer(cx)
    table = scorer.new_table(B)
    t_s = timeit(lambda: scorer.score(xs[:, :Lab], sq[:, :Lab], out=table))
    print(f'abx_design_scores  B = {B}, L = {L}: {t_s[0]:8.3f} ms per call (windows {t_s[1]:.3f} .. {t_s[2]:.3f})')
    assert ensemble.MAX_N >= 1000


if __name__ == '__main__':
    main()
