"""The z-row touch schedules of the row-fused triangle attention (TriRowArgs.touch, csrc/tri_row_touch.h; ops.tri_row_touch): 0 = no touch,
1 = the whole next row at the start of the attention phase, 2 = per k-group just ahead of the projection's walk.  A touch only warms the
L2: whatever the setting, the output equals the two launches it replaces (ops.gemm exact=2 + ops.tri_attn on the projected rows) bit for
bit, and the three settings equal each other.  With touch = 2 the issuing wave's counted waits for the weight groups include its touch
loads: a wrong count lets a wave read weights that have not landed, which shows here as differing bits.
Shapes: the smallest rows at which the last computing wave has a partial tile (33), the positions are an exact multiple of the touch
stride of 64 (64) and are ragged against it (97); B L 4 slots against the grid (256 workgroups on an MI355X: 396, 512 and 776 slots), so
workgroups have one, two, three or four slots and every one a last slot without a successor.  Needs an MI355X: `pytest -m gpu`."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
H, D, C = 4, 48, 192
SHAPES = [(33, 3), (64, 2), (97, 2)]


@pytest.fixture(scope='module')
def ops():
    from abx_amd import ops as _ops, _lib
    lib = _lib.load()
    assert lib.abx_init(0) == 0, lib.abx_last_error_string()
    before = _ops.tri_row_touch()
    yield _ops
    _ops.tri_row_touch(before)


def _pack(ops, seed):
    ge = torch.Generator().manual_seed(seed)
    W = lambda: (torch.randn(C, C, generator=ge) / C ** 0.5).to(DEV)
    b = lambda: (torch.randn(C, generator=ge) * 0.3).to(DEV)
    ln = ((1.0 + 0.2 * torch.randn(C, generator=ge)).to(DEV), (0.1 * torch.randn(C, generator=ge)).to(DEV))
    return ops.LinearPack([(W(), b(), 0), (W(), b(), 0), (W(), b(), 0)], C, ln=ln)


def _inputs(L, B, seed):
    ge = torch.Generator().manual_seed(seed)
    Lp = (L + 3) // 4 * 4
    z = (torch.randn(B, L * L, C, generator=ge) * 1.3 + 0.2).to(DEV)
    bias = torch.zeros(B, H, L, Lp)
    bias[..., :L] = torch.randn(B, H, L, L, generator=ge) * 150.0
    mask = (torch.rand(B, L, generator=ge) > 0.15).float()
    mask[:, 0] = 1
    mask[0, L - 5:] = 0
    return z, bias.to(DEV), mask.to(DEV)


@pytest.fixture(scope='module')
def cases(ops):
    """Per shape: the pack, the inputs and the two-launch reference of both orientations, computed once."""
    out = {}
    for L, B in SHAPES:
        qkv = _pack(ops, 7000 + L)
        z, bias, mask = _inputs(L, B, 7100 + L)
        M = B * L * L
        rows = torch.full((M, 3 * C), float('nan'), device=DEV)
        ops.gemm(z.view(M, C), qkv.Wt, rows, bias=qkv.bias, ln=(None, qkv.csum), B3=qkv.planes, exact=2, range_class='tri_attn')
        ref = {}
        for per_row in (True, False):
            o = torch.full((M, C), float('nan'), device=DEV)
            ops.tri_attn(rows, bias, mask, o, B, L, per_row, bias_is_qk=True, bias_log2=True)
            assert torch.isfinite(o).all()
            ref[per_row] = o
        out[(L, B)] = (ops.TriRowPack(qkv), z, bias, mask, ref)
    return out


def test_switch_roundtrip(ops):
    """ops.tri_row_touch sets 0 | 1 | 2, returns the previous setting and ignores anything else."""
    start = ops.tri_row_touch()
    assert start in (0, 1, 2)
    for v in (0, 1, 2):
        ops.tri_row_touch(v)
        assert ops.tri_row_touch() == v
        assert ops.tri_row_touch(3) == v and ops.tri_row_touch(-7) == v and ops.tri_row_touch() == v
    assert ops.tri_row_touch(start) == 2


@pytest.mark.parametrize('per_row', [True, False])
@pytest.mark.parametrize('L,B', SHAPES)
def test_touch_settings_equal_two_launches(ops, cases, L, B, per_row):
    rowp, z, bias, mask, ref = cases[(L, B)]
    M = B * L * L
    outs = {}
    for touch in (0, 1, 2):
        ops.tri_row_touch(touch)
        assert ops.tri_row_touch() == touch
        o = torch.full((M, C), float('nan'), device=DEV)
        ops.tri_attn(z.view(M, C), bias, mask, o, B, L, per_row, bias_is_qk=True, bias_log2=True, rowpack=rowp)
        n = int((o != ref[per_row]).sum())
        print(f'L={L} B={B} per_row={per_row} touch={touch}: differing elements = {n} of {o.numel()}')
        assert torch.equal(o, ref[per_row]), (L, B, per_row, touch, n)
        outs[touch] = o
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[1], outs[2])
