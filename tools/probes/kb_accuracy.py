#!/usr/bin/env python
"""abx_accuracy_scores beside abx_design_scores and abx_interface_scores at the headline shape (B = 100 designs, L = 352, Lab = 228) in
one process: HIP events around windows of R calls, median of the windows.  All three walk the (14 L)^2 atom pairs of every design:
abx_design_scores half of them in fp32, abx_interface_scores with the float64 point loop over each atom's neighbours, abx_accuracy_scores
all ordered pairs of two structures in float64 with two square roots per included pair.
    python tools/probes/kb_accuracy.py [--B 100] [--workload L352] [--step_ms MS]
--step_ms: the step time of a bench.py run on the same box; the share of a step is printed only when it is given."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..'))
from abx_amd import accuracy, interface, metrics, synthetic  # noqa: E402

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
    ap.add_argument('--step_ms', type=float, default=None, help='time of one sampler step at this shape on this box (bench.py), for the share')
    a = ap.parse_args()
    cx = {k: v.to(DEV) for k, v in synthetic.make_complex(seed=2, **synthetic.WORKLOADS[a.workload]).items()}
    B, L, Lab = a.B, cx['seq'].shape[0], cx['anchor_flag'].shape[0]
    g = torch.Generator().manual_seed(23)
    # designs that still look like the complex: residues moved as a whole by 0.3 A, atoms by 0.05 A
    x = (cx['atom14_gt_positions'][None, :Lab] + (0.3 * torch.randn(B, Lab, 1, 3, generator=g) + 0.05 * torch.randn(B, Lab, 14, 3, generator=g)).to(DEV)).contiguous()
    sq = cx['seq'][None, :Lab].repeat(B, 1)
    pl = (40.0 + 55.0 * torch.rand(B, L, generator=g)).to(DEV)
    region = cx['cdr_def'] == 5
    scorer = metrics.DesignScorer(cx)
    table = scorer.new_table(B)
    t_s = timeit(lambda: scorer.score(x, sq, out=table))
    isc = interface.InterfaceScorer(cx, region=region)
    itab = isc.new_table(B)
    t_i = timeit(lambda: isc.score(x, sq, out=itab))
    asc = accuracy.AccuracyScorer(cx, region=region)
    atab = asc.new_table(B)
    t_a = timeit(lambda: asc.score(x, sq, plddt=pl, out=atab))
    t_r = timeit(lambda: asc.score(x, sq, plddt=pl, out=atab, rows=True, counts=True, contacts=True))
    h = atab.cpu()
    bare = accuracy.AccuracyScorer(cx, region=region, radius=0.1)       # no pair inside the radius: the walk without the included-pair branch
    btab = bare.new_table(B)
    t_b = timeit(lambda: bare.score(x, sq, plddt=pl, out=btab))
    col = accuracy.ACCURACY_COLUMNS.index
    ms = lambda t: f'{t[0]:8.3f} ms per call (windows {t[1]:.3f} .. {t[2]:.3f})'
    print(f'B = {B}, L = {L}, Lab = {Lab}')
    print(f'abx_design_scores                  {ms(t_s)}')
    print(f'abx_interface_scores P = 128       {ms(t_i)}')
    print(f'abx_accuracy_scores                {ms(t_a)}; ratio to abx_design_scores {t_a[0] / t_s[0]:.2f}, to abx_interface_scores '
          f'{t_a[0] / t_i[0]:.2f}' + (f'; {100 * t_a[0] / a.step_ms:.3f} % of a {a.step_ms:.1f} ms step' if a.step_ms else ''))
    print(f'abx_accuracy_scores + rows, counts, contacts {ms(t_r)}')
    print(f'abx_accuracy_scores radius 0.1 A   {ms(t_b)}: the pair walk without an included pair (no square roots, no counters); '
          f'the included pairs cost {t_a[0] - t_b[0]:.3f} ms = {100 * (t_a[0] - t_b[0]) / t_a[0]:.0f} % of the call')
    pairs = float(h[:, col('n_pairs_region')].mean())
    print(f'scored atoms {int(h[0, col("n_atoms_scored")])} of {14 * L} slots: {(14 * L) ** 2 * B / 1e9:.2f} G pair visits per call; lddt_all '
          f'{float(h[:, col("lddt_all")].min()):.4f} .. {float(h[:, col("lddt_all")].max()):.4f}, lddt_region {float(h[:, col("lddt_region")].min()):.4f} .. '
          f'{float(h[:, col("lddt_region")].max()):.4f} ({pairs:.0f} region pairs), tm_score >= {float(h[:, col("tm_score")].min()):.4f}, native contacts '
          f'{int(h[0, col("n_native")])}, kept {int(h[:, col("n_kept")].min())} .. {int(h[:, col("n_kept")].max())}')


if __name__ == '__main__':
    main()
