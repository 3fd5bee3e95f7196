"""tests/analysis_gpu_cases.py on a machine without a GPU: importing it initialises none, the headline-size batch is the one the GPU tests
have always drawn, and the port helper hands out a port that can be bound."""
import os
import socket
import subprocess
import sys

import torch

import analysis_gpu_cases as G


def test_import_initialises_no_gpu():
    code = 'import conftest, torch, analysis_gpu_cases; assert not torch.cuda.is_initialized(); print("clean")'
    out = subprocess.run([sys.executable, '-c', code], cwd=os.path.dirname(__file__), capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == 'clean', out.stderr
    assert not torch.cuda.is_initialized()


def test_l352_designs_draws_what_the_tests_always_drew():
    """The formula of the batch-independence tests written out: coordinates first (one draw per residue, one per atom), then the
    accuracy test's pLDDT from the same generator."""
    from abx_amd import synthetic
    cx = synthetic.make_complex(seed=2, **synthetic.WORKLOADS['L352'])
    B, L, Lab = 100, cx['seq'].shape[0], cx['anchor_flag'].shape[0]
    g = torch.Generator().manual_seed(23)
    xh = (cx['atom14_gt_positions'][None, :Lab] + 0.3 * torch.randn(B, Lab, 1, 3, generator=g) + 0.05 * torch.randn(B, Lab, 14, 3, generator=g)).float()
    pl = (40.0 + 55.0 * torch.rand(B, L, generator=g)).float()
    cx2, xh2, x2, sq2, g2 = G.l352_designs(device=None)
    assert (cx2['seq'].shape[0], xh2.shape[1]) == (L, Lab) == (352, 228)
    assert xh2.dtype == torch.float32 and torch.equal(xh2.view(torch.int32), xh.view(torch.int32)) and x2 is xh2
    assert torch.equal(sq2, cx['seq'][None, :Lab].repeat(B, 1)) and all(torch.equal(cx2[k], cx[k]) for k in cx)
    pl2 = (40.0 + 55.0 * torch.rand(B, L, generator=g2)).float()
    assert torch.equal(pl2.view(torch.int32), pl.view(torch.int32))
    # the masks of the host twin of structure 57: every slot / the typed atoms of the antibody rows, the antigen's own atoms
    from abx_amd import residue_constants as rc
    plain, typed = G.typed_or_gt(cx, Lab), G.typed_or_gt(cx, Lab, typed=True)
    assert bool(plain[:Lab].all()) and torch.equal(typed[:Lab], torch.as_tensor(rc.restype_atom14_mask)[cx['seq'][:Lab]].bool())
    assert torch.equal(plain[Lab:], cx['atom14_gt_exists'][Lab:].bool()) and torch.equal(typed[Lab:], plain[Lab:])
    assert len(G.IDX13) == 13 == len(set(G.IDX13)) and set(G.ALONE) <= set(G.IDX13)


def test_free_port_can_be_bound():
    port = G.free_port()
    assert 1024 <= port < 65536
    with socket.socket() as s:
        s.bind(('127.0.0.1', port))
