"""What the GPU tests of the per-design analyses share (test_gpu_{design_scores,relax,interface,ensemble,distogram,accuracy,polar,
design_tables}.py): the library and model fixtures, the headline-size batch of the batch-independence tests, the device arguments of a
shipped complex, the sampler pair on the tiny workload and the pair of design-driver runs.  Importing it touches no GPU."""
import copy
import os
import socket

import numpy as np
import pytest
import torch

from conftest import GOLDEN

DEV = 'cuda:0'
CODES = ['6ct7_H_L_S', '6qd7_X_Z_F|E']                      # the shipped complexes, L = 231 and 259
IDX13 = [1, 57, 2, 3, 99, 4, 5, 0, 6, 7, 8, 9, 10]          # a chunk of the L352 batch, out of order
ALONE = (0, 57, 99)
TODAY = {'seq', 'atom14_results', 'pLDDT', 'time', 'rigids_t', 'seq_t'}
SHARED = ('rigids_t', 'seq', 'atom14_results', 'pLDDT', 'seq_t')


@pytest.fixture(scope='module')
def ops():
    from abx_amd import ops as _ops, _lib
    lib = _lib.load()
    assert lib.abx_init(0) == 0, lib.abx_last_error_string()
    return _ops


@pytest.fixture(scope='module')
def gpu_model(params, cfg, tmp_path_factory):
    """Score network with the seeded test weights and the product's own IGSO(3) tables (built by abx_igso3_tables into a fresh cache).
    One per importing module: max_chunk and the range history are mutable."""
    from abx_amd.model.abx import ScoreNetwork
    from abx_amd.diffuser.full_diffuser import FullDiffuser
    dc = copy.deepcopy(cfg.diffuser)
    dc.so3.cache_dir = str(tmp_path_factory.mktemp('igso3_cache'))
    D = FullDiffuser(dc).to(DEV)
    m = ScoreNetwork(cfg.model, D)
    m.load_state_dict(params, strict=True)
    return m.to(DEV).eval(), D


def free_port():
    """A port the OS has just found free."""
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        return s.getsockname()[1]


def set_master_port(monkeypatch):
    monkeypatch.setenv('MASTER_PORT', str(free_port()))


def l352_designs(device=DEV):
    """The L = 352 synthetic complex and B = 100 perturbed copies of its antibody -> (cx, xh, x, sq, g): xh (B,Lab,14,3) float32 on
    the host, x and sq on `device` (None: no copies), g the generator after the coordinate draws."""
    from abx_amd import synthetic
    cx = synthetic.make_complex(seed=2, **synthetic.WORKLOADS['L352'])
    B, L, Lab = 100, cx['seq'].shape[0], cx['anchor_flag'].shape[0]
    assert (L, Lab) == (352, 228)
    g = torch.Generator().manual_seed(23)
    xh = (cx['atom14_gt_positions'][None, :Lab] + 0.3 * torch.randn(B, Lab, 1, 3, generator=g) + 0.05 * torch.randn(B, Lab, 14, 3, generator=g)).float()
    sq = cx['seq'][None, :Lab].repeat(B, 1)
    return (cx, xh, xh, sq, g) if device is None else (cx, xh, xh.to(device), sq.to(device), g)


def typed_or_gt(cx, Lab, typed=False):
    """(L,14) mask of the host twin of a design of l352_designs(): every slot (typed: the atoms of the residue type) of the antibody
    rows, the ground truth's atoms of the others."""
    from abx_amd import residue_constants as rc
    ab = torch.as_tensor(rc.restype_atom14_mask)[cx['seq'][:Lab]].bool() if typed else torch.ones(Lab, 14, dtype=torch.bool)
    return torch.cat([ab, cx['atom14_gt_exists'][Lab:].bool()]) & cx['mask'].bool()[:, None]


def structure_inputs(c, xs, Lp=None, mask='gt'):
    """Device arguments of structures xs (B,L,14,3) of complex c (tests/relax_cases.py; rows >= Lp come from the crystal structure, which
    xs holds there) -> (x, sq, (gt_x, gt_aa, gt_mask), pred_mask, region).  mask: 'gt', a (B,L,14) tensor or None."""
    B, L = xs.shape[0], c['aa'].shape[0]
    Lp = L if Lp is None else Lp
    d = lambda t: t.to(DEV)
    m = d(c['mask'][None].repeat(B, 1, 1)) if isinstance(mask, str) else (None if mask is None else d(mask))
    return d(xs[:, :Lp].float()), d(c['aa'][None, :c['Lab']].repeat(B, 1)), (d(c['x'].float()), d(c['aa']), d(c['mask'])), m, d(c['mov'])


def assert_row(got, want, equal_cols, close_cols, rtol, what):
    """equal_cols equal; close_cols to rtol relative to max(|want|, 1)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got[equal_cols].tolist() == want[equal_cols].tolist(), (what, got[equal_cols], want[equal_cols])
    err = np.abs(got[close_cols] - want[close_cols]) / np.maximum(np.abs(want[close_cols]), 1.0)
    assert float(err.max(initial=0.0)) <= rtol, (what, got[close_cols], want[close_cols])


def tiny_batch(gpu_model):
    """The featurised tiny workload, B = 3 -> (batch, sample ids 5..7)."""
    from abx_amd import features, synthetic
    model, D = gpu_model
    B = 3
    cx = synthetic.make_complex(seed=3, **synthetic.WORKLOADS['tiny'])
    raw = {k: v.to(DEV) for k, v in synthetic.replicate(cx, B).items()}
    torch.manual_seed(11)
    b = features.build_features(raw, D)
    b['_shared_context'] = True
    model.max_chunk = None
    return b, torch.arange(B, device=DEV) + 5


def sample_tiny(gpu_model, cfg, batch, sid, mode='trajectory', **kw):
    """sample_fn on tiny_batch() from the diffuser seed every sampler test starts at."""
    from abx_amd import sampler
    model, D = gpu_model
    D.seed = 21
    return sampler.sample_fn(batch, cfg, D, model, mode=mode, num_t=5, sample_ids=sid, **kw)


def sampler_pair(gpu_model, cfg, batch, sid, new_keys, **scorers):
    """A plain and a scored trajectory of tiny_batch(): the plain records have exactly today's keys, the shared tensors are equal record
    by record, new_keys sit on the last record only -> (plain, scored)."""
    plain = sample_tiny(gpu_model, cfg, batch, sid)
    scored = sample_tiny(gpu_model, cfg, batch, sid, **scorers)
    assert len(plain) == len(scored) == 5
    for k, (p, q) in enumerate(zip(plain, scored)):
        assert set(p) - {'range_fallbacks', 'range_sticky_ops'} == TODAY, (k, sorted(p))
        for key in SHARED:
            assert torch.equal(p[key], q[key]), (k, key)
        assert all((key in q) == (k == 4) for key in new_keys), k
    return plain, scored


def pdb_args(codes):
    return ['--pdb_file'] + [os.path.join(GOLDEN, 'pdb', c + '.pdb') for c in codes]


def names(files):
    return sorted(os.path.basename(f) for f in files)


def assert_same_bytes(files, other_dir):
    """Every file of `files` has the bytes of the file of its name in other_dir."""
    for f in files:
        assert open(f, 'rb').read() == open(os.path.join(other_dir, os.path.basename(f)), 'rb').read(), (f, other_dir)


def spy_on_sampler(monkeypatch, record):
    """sampler.sample_fn runs as it is; record(batch, keywords, trajectory) of every call is kept, unless it is None -> the list."""
    from abx_amd import sampler
    seen = []
    real = sampler.sample_fn

    def spy(batch, *a, **kw):
        traj = real(batch, *a, **kw)
        rec = record(batch, kw, traj)
        if rec is not None:
            seen.append(rec)
        return traj

    monkeypatch.setattr(sampler, 'sample_fn', spy)
    return seen


def driver_pair(tmp_path, monkeypatch, kw, flags, collective, plain_extra=(), extra_files=()):
    """`abx_amd.design` with and without `flags` (which turn on the analysis the sampler takes as keyword kw): 6ct7 with plain_extra, or
    (collective) the 1-rank RCCL path on both shipped complexes.  The flagged run adds <complex>_<kw>.tsv and extra_files, nothing else,
    and every file of the plain run keeps its bytes -> (output directory, codes, N, seen): seen = (L, scorer, trajectory) per sampler call."""
    from abx_amd import design
    codes = CODES if collective else CODES[:1]
    N = 2 if collective else 4
    seen = spy_on_sampler(monkeypatch, lambda batch, k, traj: (batch['seq'].shape[1], k[kw], traj) if kw in k else None)
    set_master_port(monkeypatch)
    common = pdb_args(codes) + ['--num_samples', str(N), '--num_t', '4']
    common += ['--force_collective', '--min_block', '1'] if collective else list(plain_extra)
    out = tmp_path / kw
    files = design.main(common + list(flags) + ['--output_dir', str(out)])
    plain_files = design.main(common + ['--output_dir', str(tmp_path / 'plain')])
    assert names(files) == sorted(names(plain_files) + [f'{c}_{kw}.tsv' for c in codes] + list(extra_files))
    assert sorted(os.listdir(out)) == names(files) and sorted(os.listdir(tmp_path / 'plain')) == names(plain_files)
    assert_same_bytes(plain_files, out)
    return out, codes, N, seen


def table_lines(dir, code, kind):
    return [ln.split('\t') for ln in open(os.path.join(dir, f'{code}_{kind}.tsv')).read().splitlines()]


def runs_of(seen, code, collective):
    """The (scorer, trajectory) of the sampler calls on complex `code`: one per work unit, two on the set-level schedule."""
    runs = [(sc, tr) for L, sc, tr in seen if L == (231 if code.startswith('6ct7') else 259)]
    assert len(runs) == (2 if collective else 1)
    return runs
