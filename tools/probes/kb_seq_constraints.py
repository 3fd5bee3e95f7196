#!/usr/bin/env python
"""abx_reverse_step and the sequence-head launch (abx_seq_head_atoms / abx_seq_head_atoms_biased) with and without a sequence-constraint
table at the headline shape (B = 100 samples, L = 352) in one process: HIP events around windows of R calls, median of the windows.
The table forbids C and M everywhere, keeps 5 letters at every 6th residue and carries a soft bias elsewhere.
    python tools/probes/kb_seq_constraints.py [--B 100] [--L 352]
    python tools/ab_lib.py <the parent commit's libabx_hip.so> tools/probes/kb_seq_constraints.py --plain_only     (the same launches
        on a library from before the table existed: the unconstrained lines only)
--table_only: the constrained lines only (both variants run one kernel name: a kernel trace tells them apart by the run)"""
import argparse
import ctypes as C
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..'))
from abx_amd import _lib, residue_constants as rc  # noqa: E402

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
    ap.add_argument('--L', type=int, default=352)
    ap.add_argument('--plain_only', action='store_true', help='the library has no abx_seq_head_atoms_biased (a build of the parent commit)')
    ap.add_argument('--table_only', action='store_true', help='the launches with a table only')
    a = ap.parse_args()
    if a.plain_only:
        _lib._PROTOS.pop('abx_seq_head_atoms_biased', None)
    from abx_amd import ops
    from abx_amd.config import default_config
    from abx_amd.diffuser.full_diffuser import FullDiffuser
    B, L = a.B, a.L
    n = B * L
    g = torch.Generator().manual_seed(5)
    D = FullDiffuser(default_config().diffuser)
    D.set_tables(torch.zeros(1000, 1000), torch.zeros(1000, 1000), torch.zeros(1000, 1000), DEV)
    q = torch.randn(B, L, 4, generator=g, dtype=torch.float64)
    rig = torch.cat([q / q.norm(dim=-1, keepdim=True), 10 * torch.randn(B, L, 3, generator=g, dtype=torch.float64)], -1).to(DEV)
    x_t = torch.randint(0, 20, (B, L), generator=g).to(DEV)
    lg = (3.0 * torch.randn(B, L, 20, generator=g)).to(DEV)
    rs, ts = torch.randn(B, L, 3, generator=g).to(DEV), torch.randn(B, L, 3, generator=g, dtype=torch.float64).to(DEV)
    t = torch.full((B,), 0.5, dtype=torch.float64, device=DEV)
    dm = torch.ones(B, L, dtype=torch.int32, device=DEV)
    ids = torch.arange(B, device=DEV)
    table = 0.5 * torch.randn(L, 20, generator=g)
    table[:, [rc.restypes.index('C'), rc.restypes.index('M')]] = float('-inf')
    for l in range(0, L, 6):
        table[l, torch.randperm(20, generator=g)[5:]] = float('-inf')
    table = table.to(DEV).contiguous()
    fixed = torch.zeros(n, dtype=torch.int32, device=DEV)
    ang = torch.randn(B, L, 7, 2, generator=g)
    ang = (ang / ang.norm(dim=-1, keepdim=True)).to(DEV)
    rg32 = rig.float().contiguous()
    a37 = torch.as_tensor(rc.restype_atom37_to_atom14)[x_t.cpu()].long().to(DEV).contiguous()
    dframes = torch.as_tensor(rc.restype_rigid_group_default_frame).float().to(DEV).contiguous()
    gidx = torch.as_tensor(rc.restype_atom14_to_rigid_group).to(torch.int32).to(DEV).contiguous()
    lit = torch.as_tensor(rc.restype_atom14_rigid_group_positions).float().to(DEV).contiguous()
    seq0 = torch.empty(n, dtype=torch.int64, device=DEV)
    a14, a37o = torch.empty(n, 14, 3, device=DEV), torch.empty(n, 37, 3, device=DEV)

    out_r, out_s = torch.empty(B, L, 7, dtype=torch.float64, device=DEV), torch.empty(B, L, dtype=torch.int64, device=DEV)
    lib = _lib.load()

    def reverse(bias):
        # the argument block of FullDiffuser.reverse, filled once: the window times the launch, not the host's tensor plumbing
        kw = dict(rigid_in=rig, rigid_is_f64=1, seq_in=x_t, rot_score=rs, trans_score=ts, ts_is_f32=0, logits=lg, diffuse_mask=dm, t=t, dt=0.01,
                  seed=1, sample_ids=ids, step=3, exp_max_sigma=D.exp_max_sigma, exp_min_sigma=D.exp_min_sigma, min_b=D.min_b_f32,
                  bdiff=D.bdiff_f32, coord_scale=D.coord_scale_f32, rate_const=D.rate_const, noise_scale=1.0, center=1, rigid_out=out_r,
                  seq_out=out_s, B=B, L=L, **({} if bias is None else dict(seq_bias=bias)))
        args = _lib.AbxReverseArgs()
        for k, v in kw.items():
            setattr(args, k, ops._p(v) if torch.is_tensor(v) else v)
        return lambda: ops.check(lib.abx_reverse_step(C.byref(args), ops._stream()), 'abx_reverse_step')

    def head(bias):
        kw = {} if bias is None else dict(seq_bias=bias, L=L)
        return lambda: ops.seq_head_atoms(lg, fixed, x_t, rg32, ang, a37, dframes, gidx, lit, seq0, a14, a37o, n, **kw)

    print(f'B = {B}, L = {L}, library {_lib.library_path()}')
    cases = [] if a.table_only else [('abx_reverse_step            no table', reverse(None)), ('abx_seq_head_atoms          no table', head(None))]
    if not a.plain_only:
        cases += [('abx_reverse_step            table   ', reverse(table)), ('abx_seq_head_atoms_biased   table   ', head(table))]
    for name, fn in cases:
        med, lo, hi = timeit(fn)
        print(f'{name} {1e3 * med:9.1f} us per call (windows {1e3 * lo:.1f} .. {1e3 * hi:.1f})')


if __name__ == '__main__':
    main()
