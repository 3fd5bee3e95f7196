#!/usr/bin/env python
"""abx_distogram_scores beside abx_design_scores and abx_interface_scores in one process, at the headline shape (B = 100 designs,
L = 352) and at the cropped 6ct7 shape: HIP events around windows of R calls, median of the windows.  The kernel reads the pair
representation twice (row slices and column slices: 2 x 4 B L^2 192 bytes); the achieved rate against that is printed beside the rate of
a plain streaming read of the same buffer in the same run (a float4 sum over the tensor by torch).
    python tools/probes/kb_distogram.py [--B 100] [--workloads L352 6ct7like]"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..'))
from abx_amd import confidence, interface, metrics, synthetic  # noqa: E402

DEV = 'cuda:0'


def timeit(fn, calls=5, windows=7):
    for _ in range(2):
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
    ap.add_argument('--workloads', nargs='+', default=['L352', '6ct7like'])
    ap.add_argument('--step_ms', type=float, default=596.0, help='time of one sampler step at the headline shape, for the share')
    a = ap.parse_args()
    for wl in a.workloads:
        cx = {k: v.to(DEV) for k, v in synthetic.make_complex(seed=2, **synthetic.WORKLOADS[wl]).items()}
        B, L, Lab = a.B, cx['seq'].shape[0], cx['anchor_flag'].shape[0]
        g = torch.Generator().manual_seed(23)
        x = cx['atom14_gt_positions'][None] + (0.3 * torch.randn(B, L, 1, 3, generator=g) + 0.05 * torch.randn(B, L, 14, 3, generator=g)).to(DEV)
        sq = cx['seq'][None].repeat(B, 1)
        pair = torch.randn(B, L, L, 192, device=DEV)
        sd = {'impl.distogram.proj.weight': torch.randn(64, 192, generator=g) / 192 ** 0.5, 'impl.distogram.proj.bias': 0.1 * torch.randn(64, generator=g)}
        region = cx['cdr_def'] == 5
        conf = confidence.DistogramScorer(cx, sd, region=region)
        scorer = metrics.DesignScorer(cx)
        table = scorer.new_table(B)
        iface = interface.InterfaceScorer(cx, region=region)
        itab = iface.new_table(B)
        ctab = torch.empty(B, len(confidence.CONFIDENCE_COLUMNS), dtype=torch.float64, device=DEV)
        nbytes = pair.numel() * 4
        t_c = timeit(lambda: conf.score(pair, x[:, :Lab], sq[:, :Lab], out=ctab))
        t_p = timeit(lambda: conf.score(pair, x[:, :Lab], sq[:, :Lab], out=ctab, planes=True))
        t_r = timeit(lambda: pair.sum())
        t_s = timeit(lambda: scorer.score(x[:, :Lab], sq[:, :Lab], out=table))
        t_i = timeit(lambda: iface.score(x[:, :Lab], sq[:, :Lab], out=itab))
        h = ctab.cpu()
        print(f'{wl}: B = {B}, L = {L}, Lab = {Lab}, pair tensor {nbytes / 1e9:.2f} GB')
        print(f'  abx_distogram_scores           {t_c[0]:9.3f} ms per call (windows {t_c[1]:.3f} .. {t_c[2]:.3f}); {2 * nbytes / t_c[0] / 1e9:.2f} TB/s of the '
              f'2 x {nbytes / 1e9:.2f} GB it reads; {100 * t_c[0] / a.step_ms:.2f} % of a {a.step_ms:.0f} ms step')
        print(f'  abx_distogram_scores + planes  {t_p[0]:9.3f} ms per call (windows {t_p[1]:.3f} .. {t_p[2]:.3f})')
        print(f'  streaming read (torch sum)     {t_r[0]:9.3f} ms per call (windows {t_r[1]:.3f} .. {t_r[2]:.3f}); {nbytes / t_r[0] / 1e9:.2f} TB/s of {nbytes / 1e9:.2f} GB')
        print(f'  abx_design_scores              {t_s[0]:9.3f} ms per call (windows {t_s[1]:.3f} .. {t_s[2]:.3f})')
        print(f'  abx_interface_scores P = 128   {t_i[0]:9.3f} ms per call (windows {t_i[1]:.3f} .. {t_i[2]:.3f})')
        print(f'  nll_all {float(h[:, 0].min()):.3f} .. {float(h[:, 0].max()):.3f}, n_pairs_region {int(h[0, 9])}, exp contacts {float(h[:, 6].min()):.2f} .. {float(h[:, 6].max()):.2f}')
        del pair
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
