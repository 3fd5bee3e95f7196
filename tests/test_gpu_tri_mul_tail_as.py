"""The TriangleMultiplication tail as an A-stationary dual GEMM (csrc/gemm_as.hip gemm_as_dual_kernel: one block per 64 pair rows and all
192 columns, z walked once).  The yardstick is the tile kernel it replaces above its launch-size threshold (gemm3_dual_kernel<128, 96, ...>,
AbxGemm.tune bit 11) and the demand is equal bits: the dispatch depends on how many samples share a launch, so batch / chunk invariance
of the network rests on it.  AbxGemm.tune bit 14 forces the new kernel below the threshold.  Needs an MI355X: `pytest -m gpu`."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
TILE, FORCED = 2048, 16384


@pytest.fixture(scope='module')
def ops():
    from abx_amd import ops as _ops, _lib
    lib = _lib.load()
    assert lib.abx_init(0) == 0, lib.abx_last_error_string()
    return _ops


def g(seed):
    return torch.Generator().manual_seed(seed)


def fold_ln(W, b, gamma, beta):
    """LayerNorm folded into the Linear: Wt' = gamma * Wt, its column sums, bias' = beta @ Wt + b."""
    wt = W.double().t()
    wts = gamma.double()[:, None] * wt
    bias = beta.double() @ wt + b.double()
    return wts.float().contiguous().to(DEV), wts.sum(0).float().contiguous().to(DEV), bias.float().contiguous().to(DEV)


class Tail:
    """Inputs of test_gemm_dual_walk_variants_bit_identical: z = randn * 2 + 0.5, product = randn (channel-major, padded pair rows),
    both LayerNorms folded.  The host copies stay as they were drawn."""

    def __init__(self, ops, L, Bc, seed):
        self.ops, self.L, self.Bc = ops, L, Bc
        self.LL, self.Lp = L * L, (L + 3) // 4 * 4
        ge = g(seed)
        self.z = torch.randn(Bc, self.LL, 192, generator=ge) * 2 + 0.5
        self.tt = torch.randn(Bc, 128, L, self.Lp, generator=ge)
        self.Wo, self.bo = torch.randn(128, 192, generator=ge) / 11, torch.randn(192, generator=ge) * 0.1
        self.Wg, self.bg = torch.randn(192, 192, generator=ge) / 14, torch.randn(192, generator=ge) * 0.1
        self.g1, self.b1 = 1 + 0.1 * torch.randn(128, generator=ge), 0.1 * torch.randn(128, generator=ge)
        self.g2, self.b2 = 1 + 0.1 * torch.randn(192, generator=ge), 0.1 * torch.randn(192, generator=ge)
        self.wo, self.cso, self.bio = fold_ln(self.Wo.t().contiguous(), self.bo, self.g1, self.b1)
        self.wg, self.csg, self.big = fold_ln(self.Wg.t().contiguous(), self.bg, self.g2, self.b2)
        self.wo3, self.wg3 = ops.split_weights(self.wo), ops.split_weights(self.wg)

    def run(self, tune, z=None, tt=None, Bc=None):
        """One launch on the first Bc samples; the output rows sit in a NaN-filled buffer with eight guard rows behind every sample.
        Returns (output rows, guard rows)."""
        Bc = self.Bc if Bc is None else Bc
        zd = (self.z if z is None else z)[:Bc].to(DEV)
        td = (self.tt if tt is None else tt)[:Bc].reshape(Bc, 128, self.L * self.Lp).to(DEV)
        buf = torch.full((Bc, self.LL + 8, 192), float('nan'), device=DEV)
        pad = (self.L, self.Lp) if self.Lp != self.L else None
        self.ops.gemm(td.transpose(1, 2), self.wo, buf[:, :self.LL], bias=self.bio, ln=(None, self.cso), B3=self.wo3, resid=zd, pair=pad,
                      c_pair=pad is not None, dual=(zd, self.wg3, self.csg, self.big), exact=2, tune=tune)
        torch.cuda.synchronize()
        return buf[:, :self.LL], buf[:, self.LL:]

    def fp64(self):
        x = self.tt[..., :self.L].permute(0, 2, 3, 1).reshape(self.Bc, self.LL, 128).double()
        ln = lambda v, ga, be: (v - v.mean(-1, keepdim=True)) / torch.sqrt(v.var(-1, unbiased=False, keepdim=True) + 1e-5) * ga.double() + be.double()
        return ((ln(x, self.g1, self.b1) @ self.Wo.double() + self.bo.double()) * torch.sigmoid(ln(self.z.double(), self.g2, self.b2) @ self.Wg.double() + self.bg.double())
                + self.z.double())


def bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize('L,Bc', [(64, 3), (70, 3), (118, 2), (128, 2)])
def test_equal_bits_with_the_tile_kernel(ops, L, Bc):
    """An exact multiple of 64 rows (64); L % 4 != 0 with padded pair rows and a ragged last block (70: 5040 rows = 78.75 blocks; 118:
    Lp = 120); several blocks per pair row (128).  Nothing but the real pair rows is written."""
    t = Tail(ops, L, Bc, 9100 + L)
    ref, guard_ref = t.run(TILE)
    out, guard = t.run(FORCED)
    assert torch.isfinite(ref).all() and torch.isfinite(out).all()
    assert torch.equal(bits(out), bits(ref)), float((out - ref).abs().max())
    assert torch.isnan(guard).all() and torch.isnan(guard_ref).all()


def test_forced_kernel_against_fp64(ops):
    """The expression and the tolerance of test_gemm_dual_proj_out_times_gate (tests/test_gpu_kernels.py), padded pair rows."""
    t = Tail(ops, 70, 3, 9200)
    out, _ = t.run(FORCED)
    ref = t.fp64()
    e = float((out.cpu().double() - ref).abs().max() / ref.abs().max())
    assert e == e and e <= 3e-6, f'dual tail (A-stationary) vs fp64: rel err {e:.3e}'


def test_shifted_statistics_keep_the_bits(ops):
    """|mean| >> sigma in one z row and one product row (test_gemm_fused_transition's input): the statistics are shifted by the row's
    first element in both kernels, in the same order."""
    t = Tail(ops, 70, 3, 9300)
    ge = g(9301)
    z, tt = t.z.clone(), t.tt.clone()
    z[1, 70 * 13 + 5] = 1e3 + torch.randn(192, generator=ge)
    tt[2, :, 41, 17] = 1e3 + torch.randn(128, generator=ge)
    ref, _ = t.run(TILE, z, tt)
    out, _ = t.run(FORCED, z, tt)
    assert torch.isfinite(ref).all()
    assert torch.equal(bits(out), bits(ref)), float((out - ref).abs().max())


@pytest.mark.parametrize('which', ['product', 'z'])
def test_range_contract(ops, which):
    """One operand element beyond the split-f16 range (2^20): NaN in the same positions as the tile kernel gives, the same bit of the
    range word, every other row untouched."""
    t = Tail(ops, 70, 3, 9400)
    word = ops.range_word(DEV)
    word.zero_()
    clean, _ = t.run(FORCED)
    assert int(word.item()) == 0
    z, tt = t.z.clone(), t.tt.clone()
    if which == 'product':
        tt[1, 77, 33, 21] = 3.0e6
        row = (1, 33 * 70 + 21)
    else:
        z[2, 70 * 50 + 9, 100] = 3.0e6
        row = (2, 70 * 50 + 9)
    got = []
    for tune in (TILE, FORCED):
        word.zero_()
        out, guard = t.run(tune, z, tt)
        got.append((out, int(word.item())))
        assert torch.isnan(guard).all()
    (ref, wref), (out, wout) = got
    word.zero_()
    assert wref & ops.RANGE_TAGS['tri_mul_tail'] and wout == wref, (wref, wout)
    assert torch.equal(torch.isnan(out), torch.isnan(ref))
    bad = torch.isnan(out).any(-1)
    assert torch.equal(bits(out[~bad]), bits(ref[~bad]))
    assert bool(bad[row]) and int(bad.sum()) == 1, int(bad.sum())
    assert torch.equal(bits(out[~bad]), bits(clean[~bad]))


@pytest.mark.parametrize('L,Bc', [(128, 4), (118, 5)])
def test_launch_size_threshold_is_bit_invariant(ops, L, Bc):
    """The default dispatch on either side of its threshold of 1 024 blocks of 64 rows: Bc samples take the new kernel, Bc - 1 the tile
    kernel, and the samples they share are equal bit for bit."""
    t = Tail(ops, L, Bc, 9500 + L)
    M = L * t.Lp
    assert ((M + 63) // 64) * Bc >= 1024 > ((M + 63) // 64) * (Bc - 1)
    assert ops.gemm_kernel_name(M, 192, 128, Bc, a_kcontig=False, split=True, exact=2, dual=True) == 'gemm_as_dual_kernel'
    assert ops.gemm_kernel_name(M, 192, 128, Bc - 1, a_kcontig=False, split=True, exact=2, dual=True).startswith('gemm3_dual_kernel')
    big, _ = t.run(0)
    small, _ = t.run(0, Bc=Bc - 1)
    assert torch.isfinite(big).all()
    assert torch.equal(bits(big[:Bc - 1]), bits(small))


@pytest.mark.parametrize('outgoing', [True, False])
def test_block_entry_equals_the_descriptor_sequence(ops, outgoing):
    """ops.tri_mul_fwd (abx_tri_mul_fwd: its tail takes the new kernel at 1 024 blocks) against the three descriptor-level launches of
    model/forward.py with the tail pinned to the tile kernel."""
    L, B, C = 128, 4, 192
    LL = L * L
    ge = g(9600)
    W = lambda n, k: (torch.randn(n, k, generator=ge) / k ** 0.5).to(DEV)
    b = lambda n: (torch.randn(n, generator=ge) * 0.1).to(DEV)
    ln = lambda k: ((1.0 + 0.1 * torch.randn(k, generator=ge)).to(DEV), (0.1 * torch.randn(k, generator=ge)).to(DEV))
    ln_z = ln(C)
    glu = ops.LinearPack([(W(128, C), b(128), 1), (W(128, C), b(128), 1), (W(128, C), b(128), 2), (W(128, C), b(128), 2)], C, ln=ln_z)
    out = ops.LinearPack([(W(C, 128), b(C), 0)], 128, ln=ln(128))
    gate = ops.LinearPack([(W(C, C), b(C), 0)], C, ln=ln_z)
    pack = ops.tri_mul_pack(glu, out, gate)
    z = (torch.randn(B, LL, C, generator=ge) * 2 + 0.5).to(DEV)
    mask = (torch.rand(B, L, generator=ge) > 0.1).float().to(DEV)
    got = torch.full_like(z, float('nan'))
    ops.tri_mul_fwd(pack, z, got, mask, B, L, outgoing, ops.tri_mul_workspace(B, L, DEV))
    # the descriptor-level sequence (L % 16 == 0: no padded pair rows, no pad k-tiles)
    pm = torch.empty(B * LL, device=DEV)
    ops.pair_mask(mask, pm, B, L)
    lrp = torch.empty(B, 256, L // 16, 2, L, 16, dtype=torch.int16, device=DEV)
    ops.gemm(z, glu.Wt, lrp, bias=glu.bias, ln=(None, glu.csum), B3=glu.planes, rowscale=pm, glu=True, c_split_nA=128, c_split_tile=True,
             a_pair_transpose=0 if outgoing else L, pair=(L, L), a_pair=True, exact=2)
    tt = torch.empty(B, 128, LL, device=DEV)
    ops.gemm(lrp[:, 0:128], lrp[:, 128:256], tt.view(B * 128, L, L), exact=2)
    ref = torch.full_like(z, float('nan'))
    ops.gemm(tt.transpose(1, 2), out.Wt, ref, bias=out.bias, ln=(None, out.csum), B3=out.planes, resid=z, dual=(z, gate.planes, gate.csum, gate.bias),
             exact=2, tune=TILE)
    torch.cuda.synchronize()
    assert torch.isfinite(ref).all()
    assert torch.equal(bits(got), bits(ref)), float((got - ref).abs().max())
