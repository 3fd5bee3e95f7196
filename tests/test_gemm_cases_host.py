"""The case table of tests/gemm_cases.py, checked without a GPU: every case plans to the kernel written next to it (abx_gemm_plan on
placeholder addresses), the names reached cover every tile-kernel instantiation the dispatch can launch, and the bound of
tests/test_gpu_gemm_cases.py tells a right kernel from a subtly wrong one: float64 restatements with one deliberate mistake each leave it
by a wide margin, and so does a float32 restatement of the unshifted one-pass LayerNorm statistic at rows of mean 3 and 30 sigma."""
import itertools

import pytest
import torch
import torch.nn.functional as F

import gemm_cases as G

MARGIN = 8.0         # "a wide margin": a mistake must miss one of the two assertions of the bound by this factor on at least one case


def test_every_case_plans_to_its_kernel():
    bad = []
    for c in G.CASES:
        rc, name = G.plan(G.descriptor(c))
        if rc != 0 or name != c.kernel:
            bad.append((c.name, rc, name, c.kernel))
    assert not bad, bad


def test_required_instantiations_are_covered():
    assert len(set(G.REQUIRED)) == len(G.REQUIRED) == 40
    reached = {c.kernel for c in G.CASES}
    assert reached == set(G.REQUIRED), (sorted(set(G.REQUIRED) - reached), sorted(reached - set(G.REQUIRED)))


def test_dispatch_launches_nothing_outside_the_table():
    """A sweep of descriptors over shapes, layouts, stores, arithmetic classes and alignments: whatever the dispatch names is in REQUIRED,
    so a route added to the dispatch and not to the table fails here."""
    seen, outside = set(), set()
    shapes = itertools.product((1, 4, 64, 65, 130, 132, 32641, 49025), (1, 32, 33, 64, 65, 128, 190, 192, 256, 448, 768), (16, 17, 192))
    for (M, N, K) in shapes:
        for a, b, store, exact, oln, mis in itertools.product(('k', 'm', 'planes'), ('n', 'k', 'weights', 'planes'), ('plain', 'transposed'),
                                                               (0, 1, 2), (False, True), ((), ('A',))):
            if (a == 'planes') != (b == 'planes') or (a == 'planes' and (K % 16 or mis)):
                continue
            c = G.Case('sweep', M, N, K, 1, a, b, store, exact, frozenset(('out_ln',) if oln else ()), frozenset(mis), 0, None, 'sweep')
            rc, name = G.plan(G.descriptor(c))
            if rc == 0:
                seen.add(name)
                if name not in G.REQUIRED:
                    outside.add((name, M, N, K, a, b, store, exact, oln))
    assert not outside, sorted(outside)[:8]
    assert len(seen) >= 36, sorted(set(G.REQUIRED) - seen)         # the sweep itself reaches the table (batch and size edges aside)


def test_names_are_unique_and_seeds_depend_on_the_case_alone():
    assert len({c.name for c in G.CASES}) == len(G.CASES)
    assert all(c.name == G.case_id(c) and G.BY_NAME[c.name] is c for c in G.CASES)
    for c in G.CASES[:40]:
        assert G.case_seed(c) == G.case_seed(c._replace(name='x', kernel='y', misalign=frozenset(), a_layout='k' if c.a_layout != 'planes' else 'planes'))
    c = G.BY_NAME['x-small-130x65x52-Ak-Bn-e1']
    a, b = G.inputs(c)['A'].clone(), G._inputs.__wrapped__(G._data_key(c), G.case_seed(c))['A']
    assert torch.equal(a, b) and G.case_seed(c) != G.case_seed(c._replace(K=53))


def test_every_family_has_a_case_with_a_mean_bound():
    fam = {}
    for c in G.CASES:
        fam[c.family] = max(fam.get(c.family, 0), G.outputs(c))
    assert all(n >= G.MEAN_FROM for n in fam.values()), fam


SMALL = [c for c in G.CASES if c.M <= 600 and c.batch <= 3]


def test_reference_is_float64_and_baseline_float32_of_the_same_text():
    for c in (G.BY_NAME['x-epi-130x65x52-Ak-Bn-e1+alpha+bias+gate+relu+resid+rowscale'], G.BY_NAME['s-planes-65x65x80-b3-Aplanes-Bplanes-e2'],
              G.BY_NAME['s-oln-130x100x192-Ak-Bweights-e2+bias+out_ln'], G.BY_NAME['x-ln-300x192x192-Am-Bn-e1+bias+ln_inline-off30']):
        ref, base = G.reference(c), G.baseline(c)
        assert ref.dtype == torch.float64 and base.dtype == torch.float32 and ref.shape == base.shape == (c.batch, c.M, c.N)
        assert torch.equal(ref, G.evaluate(c.epi, G.inputs(c), torch.float64)) and torch.equal(base, G.evaluate(c.epi, G.inputs(c), torch.float32))
        e32 = G.baseline_err(c)
        assert 0 < e32[0] < 2e-5 * float(ref.abs().max()) and e32 == G.err(base, c)
        assert G.within_bound(c, e32, e32)


def test_plane_cases_are_the_product_of_the_values_the_images_stand_for():
    c = G.BY_NAME['s-planes-65x65x80-b3-Aplanes-Bplanes-e2']
    x = G.inputs(c)
    a, b = G._planes_to_f64(x['A_planes'], True), G._planes_to_f64(x['B_planes'], False)
    assert x['A_planes'].shape == (3, 5, 2, 65, 16) and bool((a[..., 65:] == 0).all()) and bool((b[..., 65:] == 0).all())
    assert torch.equal(G.reference(c), a @ b.transpose(1, 2))


# ---- sensitivity ------------------------------------------------------------------------------------------------------------------------
def restate(c, mistake):
    """The operation of `evaluate` once more in float64, with one deliberate mistake."""
    x = {k: v.double() for k, v in G.inputs(c).items() if v.dtype == torch.float32}
    A, B, epi = x['A'], x['B'], c.epi
    if 'a_relu' in epi:
        A = torch.relu(A)
    if 'ln_stats' in epi or 'ln_inline' in epi:
        mean, var = A.mean(-1, keepdim=True), A.var(-1, unbiased=False, keepdim=True)
        A = (A - mean) / torch.sqrt(var + (0.0 if mistake == 'variance without eps' else G.EPS))
    if mistake == 'last k dropped':
        A, B = A[..., :-1], B[..., :-1, :]
    v = A @ B
    if mistake == 'bias after alpha':
        v = v * G.ALPHA + x['bias']
    else:
        v = (v + x['bias']) if 'bias' in epi else v
        v = v * G.ALPHA if 'alpha' in epi else v
    v = torch.relu(v) if 'relu' in epi else torch.sigmoid(v) if 'sigmoid' in epi else v
    if 'out_ln' in epi:
        v = F.layer_norm(v, (c.N,), x['oln_w'], x['oln_b'], G.EPS)
    late = mistake == 'rowscale after the residual'
    if 'rowscale' in epi and not late:
        v = v * x['rowscale'][..., None]
    if 'gate' in epi:
        v = v * (x['gate'] if mistake == 'gate without the sigmoid' else torch.sigmoid(x['gate']))
    if 'gate_raw' in epi:
        v = v * x['gate']
    if 'resid' in epi:
        v = v + x['resid']
    if late:
        v = v * x['rowscale'][..., None]
    if mistake == 'last row tile shifted by one':
        r0 = (c.M - 1) // _tile_rows(c) * _tile_rows(c)
        v = torch.cat([v[:, :r0], torch.roll(v[:, r0:], 1, dims=1)], 1)
    if mistake == 'transposed store written as plain':       # element (m, n) lands at m N + n of a buffer that is read as [n][m]
        v = v.reshape(c.batch, c.N, c.M).transpose(1, 2)
    return v


def _tile_rows(c):
    return int(c.kernel.split('<')[1].split(',')[0])


NEEDS = {'last k dropped': lambda c: not c.epi, 'last row tile shifted by one': lambda c: (c.M - 1) % _tile_rows(c) >= 1,      # two rows or more in it
         'bias after alpha': lambda c: {'bias', 'alpha'} <= c.epi, 'rowscale after the residual': lambda c: {'rowscale', 'resid'} <= c.epi,
         'gate without the sigmoid': lambda c: 'gate' in c.epi, 'variance without eps': lambda c: 'ln_inline' in c.epi and c.offset == 0,
         'transposed store written as plain': lambda c: c.store == 'transposed'}


def test_restatement_without_a_mistake_is_the_reference():
    for c in SMALL[::7]:
        e = G.err(restate(c, None), c)
        assert e[0] <= 1e-12 * max(1.0, float(G.reference(c).abs().max())), (c.name, e)


@pytest.mark.parametrize('mistake', sorted(NEEDS))
def test_a_deliberate_mistake_leaves_the_bound(mistake):
    """Each mistake, in float64 (no rounding to hide behind), misses the bound by MARGIN on at least one case; and by itself on every
    case of 1024 or more outputs it applies to, K = 1 aside."""
    cases = [c for c in SMALL if NEEDS[mistake](c)][:12]
    assert cases
    wide = 0
    for c in cases:
        e, e32 = G.err(restate(c, mistake), c), G.baseline_err(c)
        if G.outputs(c) >= G.MEAN_FROM and c.K > 1:
            assert not G.within_bound(c, e, e32), (mistake, c.name, e, e32)
        wide += e[0] > MARGIN * G.K_MAX * e32[0] or e[1] > MARGIN * G.K_MEAN * e32[1]
    assert wide, mistake


def one_pass_fold(c, shifted):
    """The LayerNorm fold of the exact kernel with inline statistics, in float32: rstd (acc - (mean - shift) csum) + bias with the one-pass
    statistic sum(d), sum(d d) of d = x - shift; shift = 0 (the m-contiguous path before it was made to shift) or the row's first element."""
    x = G.inputs(c)
    A, B = x['A'], x['B']
    d = A - (A[..., :1] if shifted else 0.0)
    s, q = torch.zeros_like(d[..., 0]), torch.zeros_like(d[..., 0])
    for k in range(c.K):                                         # the ordered chain of the kernel: one fma per element
        s, q = s + d[..., k], q + d[..., k] * d[..., k]
    dm = s / c.K
    rstd = 1.0 / torch.sqrt(torch.clamp(q / c.K - dm * dm, min=0.0) + G.EPS)
    return rstd[..., None] * (d @ B - dm[..., None] * x['csum']) + x['bias']


@pytest.mark.parametrize('offset', [0, 3, 30])
def test_bound_tells_the_unshifted_statistic_from_the_shifted(offset):
    c = G.BY_NAME['x-ln-300x192x192-Am-Bn-e1+bias+ln_inline' + (f'-off{offset}' if offset else '')]
    e32 = G.baseline_err(c)
    e_un, e_sh = G.err(one_pass_fold(c, False), c), G.err(one_pass_fold(c, True), c)
    print(f'GEMM-CASES-HOST offset {offset}: e32 {e32}; unshifted ratio {e_un[0] / e32[0]:.2f} {e_un[1] / e32[1]:.2f}; '
          f'shifted ratio {e_sh[0] / e32[0]:.2f} {e_sh[1] / e32[1]:.2f}')
    assert G.within_bound(c, e_sh, e32), (e_sh, e32)
    assert G.within_bound(c, e_un, e32) == (offset == 0), (e_un, e32)
