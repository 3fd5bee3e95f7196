#!/usr/bin/env python
"""abx_design_scores against abx_clash_grad at the headline shape (B = 100 designs, L = 352, Lab = 228) in one process: HIP events around
windows of R calls, median of the windows.  abx_clash_grad walks the same atom pairs (each from both atoms) and forms gradients as well.
    python tools/probes/kb_design_scores.py [--B 100] [--workload L352]"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..'))
from abx_amd import metrics, ops, synthetic  # noqa: E402

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
    ap.add_argument('--B', type=int, default=100)
    ap.add_argument('--workload', default='L352')
    a = ap.parse_args()
    cx = {k: v.to(DEV) for k, v in synthetic.make_complex(seed=2, **synthetic.WORKLOADS[a.workload]).items()}
    B, L, Lab = a.B, cx['seq'].shape[0], cx['anchor_flag'].shape[0]
    g = torch.Generator().manual_seed(23)
    x = cx['atom14_gt_positions'][None] + 0.7 * torch.randn(B, L, 14, 3, generator=g).to(DEV)
    sq = cx['seq'][None].repeat(B, 1)
    scorer = metrics.DesignScorer(cx)
    table = scorer.new_table(B)
    rep = lambda k: cx[k][None].expand(B, *cx[k].shape).contiguous()
    exists, chain, residx, ft = rep('atom14_gt_exists'), rep('chain_id'), rep('residx'), x[:, :, 1].contiguous()
    t_s = timeit(lambda: scorer.score(x[:, :Lab], sq[:, :Lab], out=table))
    t_g = timeit(lambda: ops.clash_grad(x, exists, sq, chain, ft, residx=residx))
    n = table[:, 17].cpu()
    print(f'B = {B}, L = {L}, Lab = {Lab}: clashing pairs per design {float(n.min()):.0f} .. {float(n.max()):.0f}')
    print(f'abx_design_scores  {t_s[0]:8.3f} ms per call (windows {t_s[1]:.3f} .. {t_s[2]:.3f})')
    print(f'abx_clash_grad     {t_g[0]:8.3f} ms per call (windows {t_g[1]:.3f} .. {t_g[2]:.3f})')
    print(f'ratio scores / clash_grad = {t_s[0] / t_g[0]:.3f}')


if __name__ == '__main__':
    main()
