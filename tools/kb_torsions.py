#!/usr/bin/env python
"""abx_torsion_scores beside abx_design_scores at the headline shape (B = 100 designs, L = 352, Lab = 228) in one process: HIP events
around windows of R calls, the two kernels in alternating windows, median of the windows.  abx_design_scores walks half of the (14 L)^2
atom pairs of every design in fp32; abx_torsion_scores reads N, CA, C and the chi atoms of the Lab antibody rows of the design and of
the wild type once, in float64: 3 backbone and up to 4 chi dihedrals per row and structure, one workgroup per design.
    python tools/kb_torsions.py [--B 100] [--workload L352] [--calls 200] [--windows 9]"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from abx_amd import metrics, ops, synthetic, torsions  # noqa: E402

DEV = 'cuda:0'


def window(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls


def alternate(fns, calls, windows):
    """{name: (median, fastest, slowest window)} in ms per call: every shape warmed up first, then one window of each in turn."""
    for fn in fns.values():
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(windows):
        for k, fn in fns.items():
            ts[k].append(window(fn, calls))
    return {k: (sorted(v)[len(v) // 2], min(v), max(v)) for k, v in ts.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--B', type=int, default=100)
    ap.add_argument('--workload', default='L352')
    ap.add_argument('--calls', type=int, default=200, help='calls per window')
    ap.add_argument('--windows', type=int, default=9)
    a = ap.parse_args()
    cx = {k: v.to(DEV) for k, v in synthetic.make_complex(seed=2, **synthetic.WORKLOADS[a.workload]).items()}
    B, L, Lab = a.B, cx['seq'].shape[0], cx['anchor_flag'].shape[0]
    g = torch.Generator().manual_seed(23)
    # designs that still look like the complex: residues moved as a whole by 0.3 A, atoms by 0.05 A
    x = (cx['atom14_gt_positions'][None, :Lab] + (0.3 * torch.randn(B, Lab, 1, 3, generator=g) + 0.05 * torch.randn(B, Lab, 14, 3, generator=g)).to(DEV)).contiguous()
    sq = cx['seq'][None, :Lab].repeat(B, 1)
    scorer = metrics.DesignScorer(cx)
    stab = scorer.new_table(B)
    tor = torsions.TorsionScorer(cx, region=cx['cdr_def'] == 5)
    ttab, rows, classes = tor.new_table(B), tor.new_rows(B), tor.new_classes(B)
    ws = torch.empty(ops.torsion_workspace_bytes(B, Lab), dtype=torch.uint8, device=DEV)
    t = alternate({'design': lambda: scorer.score(x, sq, out=stab),
                   'torsion': lambda: tor.score(x, sq, out=ttab, workspace=ws),
                   'torsion_rows': lambda: tor.score(x, sq, out=ttab, rows=rows, classes=classes, workspace=ws),
                   'torsion_alloc': lambda: tor.score(x, sq, out=ttab)}, a.calls, a.windows)
    ms = lambda v: f'{v[0]:8.4f} ms per call (windows {v[1]:.4f} .. {v[2]:.4f})'
    h = ttab.cpu()
    col = torsions.TORSIONS_COLUMNS.index
    print(f'B = {B}, L = {L}, Lab = {Lab}, {a.windows} windows of {a.calls} calls each, workspace {ws.numel() / 2 ** 20:.1f} MiB')
    print(f'abx_design_scores                          {ms(t["design"])}')
    print(f'abx_torsion_scores                         {ms(t["torsion"])}; ratio to abx_design_scores {t["torsion"][0] / t["design"][0]:.3f}')
    print(f'abx_torsion_scores + rows, classes         {ms(t["torsion_rows"])}')
    print(f'abx_torsion_scores, workspace allocated    {ms(t["torsion_alloc"])}')
    print(f'n_links {int(h[0, col("n_links")])}, twisted {int(h[:, col("twisted")].min())} .. {int(h[:, col("twisted")].max())}, phi_pos '
          f'{int(h[:, col("phi_pos")].min())} .. {int(h[:, col("phi_pos")].max())}, abego_same {int(h[:, col("abego_same")].min())} .. '
          f'{int(h[:, col("abego_same")].max())} of {int(h[0, col("n_abego")])}, chi1_ok {int(h[:, col("chi1_ok")].min())} .. {int(h[:, col("chi1_ok")].max())} of '
          f'{int(h[0, col("n_chi1")])}')


if __name__ == '__main__':
    main()
