#!/usr/bin/env python
"""abx_contact_grad beside abx_clash_grad at the headline shape (B = 100 designs, L = 352, Lab = 228) in one process: HIP events around
windows of R calls, median of the windows.  12 moved rows per design (the CDR-H3 window placed beside the antigen), all three terms on:
contacts, 6 hotspots, 24 restraints.  abx_clash_grad walks all atom pairs of the complex; abx_contact_grad only moved x partner atoms.
    python tools/probes/kb_contact.py [--B 100] [--workload L352]"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..'))
from abx_amd import ops, synthetic  # noqa: E402

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
    cx = synthetic.make_complex(seed=2, **synthetic.WORKLOADS[a.workload])
    B, L, Lab = a.B, cx['seq'].shape[0], cx['anchor_flag'].shape[0]
    g = torch.Generator().manual_seed(23)
    rows = list(range(98, 110))                                          # 12 moved rows
    x = cx['atom14_gt_positions'][None].repeat(B, 1, 1, 1)
    centre = cx['atom14_gt_positions'][Lab:, 1].mean(0)
    x[:, rows] = centre + 4.0 * torch.randn(B, len(rows), 1, 3, generator=g) + 1.5 * torch.randn(B, len(rows), 14, 3, generator=g)
    moved = torch.zeros(B, L, dtype=torch.bool)
    moved[:, rows] = True
    target = torch.arange(L) >= Lab
    near = torch.cdist(cx['atom14_gt_positions'][Lab:, 1], centre[None])[:, 0].argsort()[:6] + Lab
    idx = torch.tensor([[rows[k % 12], 1, Lab + 5 * k, 1] for k in range(24)], dtype=torch.int32)
    par = torch.tensor([[4.0, 8.0, 1.0]] * 24)
    tables = ops.ContactTables(DEV, near.tolist(), (idx, par))
    rep = lambda k: cx[k][None].expand(B, *cx[k].shape).contiguous().to(DEV)
    x, moved, target = x.to(DEV), moved.to(DEV), target.to(DEV)
    exists, chain, residx, sq, ft = rep('atom14_gt_exists'), rep('chain_id'), rep('residx'), rep('seq'), x[:, :, 1].contiguous()
    kw = dict(w_contact=1.0, d0=4.0, d1=8.0, w_hot=1.0, d_hot=8.0, beta=1.0)
    t_c = timeit(lambda: ops.contact_grad(x, exists, moved, target, ft, tables, **kw))
    t_g = timeit(lambda: ops.clash_grad(x, exists, sq, chain, ft, residx=residx))
    e = ops.contact_grad(x, exists, moved, target, ft, tables, **kw)[0].cpu()
    print(f'B = {B}, L = {L}, Lab = {Lab}, {len(rows)} moved rows, {tables.H} hotspots, {tables.R} restraints: mean energies '
          f'contact {float(e[:, 0].mean()):.1f}, hotspot {float(e[:, 1].mean()):.2f}, restraint {float(e[:, 2].mean()):.1f}')
    print(f'abx_contact_grad   {t_c[0]:8.3f} ms per call (windows {t_c[1]:.3f} .. {t_c[2]:.3f})')
    print(f'abx_clash_grad     {t_g[0]:8.3f} ms per call (windows {t_g[1]:.3f} .. {t_g[2]:.3f})')
    print(f'ratio contact_grad / clash_grad = {t_c[0] / t_g[0]:.3f}')


if __name__ == '__main__':
    main()
