#!/usr/bin/env python
"""abx_secondary_scores beside abx_torsion_scores and abx_design_scores at the headline shape (B = 100 designs, L = 352, Lab = 228) in
one process: HIP events around windows of R calls, the kernels in alternating windows, median of the windows.  abx_design_scores walks
half of the (14 L)^2 atom pairs of every design in fp32; abx_torsion_scores measures 3 backbone and up to 4 chi dihedrals per row;
abx_secondary_scores evaluates the C-alpha prefilter of all Lab^2 (donor, acceptor) pairs of the design and of the wild type in
float64, the four-distance energy of the pairs within 9 A, and the pattern logic on the bond bits - one workgroup per design.
    python tools/kb_secondary.py [--B 100] [--workload L352] [--calls 200] [--windows 9]"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from abx_amd import metrics, ops, secondary, synthetic, torsions  # noqa: E402

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
    ttab = tor.new_table(B)
    tws = torch.empty(ops.torsion_workspace_bytes(B, Lab), dtype=torch.uint8, device=DEV)
    sec = secondary.SecondaryScorer(cx, region=cx['cdr_def'] == 5)
    ctab, rows, classes = sec.new_table(B), sec.new_rows(B), sec.new_classes(B)
    ws = torch.empty(ops.secondary_workspace_bytes(B, Lab), dtype=torch.uint8, device=DEV)
    t = alternate({'design': lambda: scorer.score(x, sq, out=stab),
                   'torsion': lambda: tor.score(x, sq, out=ttab, workspace=tws),
                   'secondary': lambda: sec.score(x, sq, out=ctab, workspace=ws),
                   'secondary_rows': lambda: sec.score(x, sq, out=ctab, rows=rows, classes=classes, workspace=ws),
                   'secondary_alloc': lambda: sec.score(x, sq, out=ctab)}, a.calls, a.windows)
    ms = lambda v: f'{v[0]:8.4f} ms per call (windows {v[1]:.4f} .. {v[2]:.4f})'
    h = ctab.cpu()
    col = secondary.SECONDARY_COLUMNS.index
    rng = lambda c: f'{int(h[:, col(c)].min())} .. {int(h[:, col(c)].max())}'
    print(f'B = {B}, L = {L}, Lab = {Lab}, {a.windows} windows of {a.calls} calls each, workspace {ws.numel() / 2 ** 20:.1f} MiB')
    print(f'abx_design_scores                            {ms(t["design"])}')
    print(f'abx_torsion_scores                           {ms(t["torsion"])}; ratio to abx_design_scores {t["torsion"][0] / t["design"][0]:.3f}')
    print(f'abx_secondary_scores                         {ms(t["secondary"])}; ratio to abx_design_scores {t["secondary"][0] / t["design"][0]:.3f}, '
          f'to abx_torsion_scores {t["secondary"][0] / t["torsion"][0]:.2f}')
    print(f'abx_secondary_scores + rows, classes         {ms(t["secondary_rows"])}')
    print(f'abx_secondary_scores, workspace allocated    {ms(t["secondary_alloc"])}')
    print(f'n_hb {rng("n_hb")}, hb_wild_region {int(h[0, col("hb_wild_region")])}, hb_kept_region {rng("hb_kept_region")}, n_bridge_region '
          f'{rng("n_bridge_region")}, q8_same {rng("q8_same")} of {int(h[0, col("n_ss")])}, strand_ab {rng("strand_ab")}, helix_ab {rng("helix_ab")}')


if __name__ == '__main__':
    main()
