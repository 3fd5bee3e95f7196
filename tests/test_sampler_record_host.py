"""Host checks of the one record path of sampler.sample_fn: what every scorer keyword adds to the last record, the order in which the
scorers run, and who shares the point counts of the surface kernel.  No device: the scorers are the real classes with `score` replaced
(their `record`, `side_outputs`, `new_points`, `new_rows` and `new_classes` run as they are), the network a stand-in on CPU tensors."""
import inspect
from types import SimpleNamespace

import pytest
import torch

from abx_amd import accuracy, confidence, developability, interface, metrics, patches, polar, relax, sampler, secondary, shape, torsions

B, LAB, L = 2, 5, 8
TODAY = {'seq', 'atom14_results', 'pLDDT', 'time', 'rigids_t', 'seq_t'}
ORDER = ['interface', 'polar', 'developability', 'shape', 'patches', 'torsions', 'secondary', 'confidence', 'accuracy']
CLASSES = dict(interface=interface.InterfaceScorer, polar=polar.PolarScorer, developability=developability.DevelopabilityScorer,
               shape=shape.ShapeScorer, patches=patches.PatchScorer, torsions=torsions.TorsionScorer, secondary=secondary.SecondaryScorer,
               confidence=confidence.DistogramScorer, accuracy=accuracy.AccuracyScorer)
# the keys of the last record, by keyword: always, only with a relaxer, only with want_rows / want_planes
KEYS = dict(interface=(['interface'], ['interface_relaxed'], []),
            polar=(['polar'], ['polar_relaxed'], ['polar_bonds', 'polar_rows']),
            developability=(['developability'], ['developability_relaxed'], ['developability_rows']),
            shape=(['shape'], ['shape_relaxed'], []),
            patches=(['patches'], ['patches_relaxed'], ['patches_rows']),
            torsions=(['torsions', 'torsions_classes'], ['torsions_relaxed'], ['torsions_rows']),
            secondary=(['secondary', 'secondary_classes'], ['secondary_relaxed'], ['secondary_rows']),
            confidence=(['confidence', 'confidence_rows', 'confidence_wild'], ['confidence_relaxed'], ['confidence_planes']),
            accuracy=(['accuracy', 'accuracy_rows'], ['accuracy_relaxed'], []))


def fake(kw, log, built_on=None, want=False):
    """The scorer class of keyword kw with the attributes its record path reads and a `score` that logs (kw, structures, keywords and
    `first`, its first argument)."""
    cls = CLASSES[kw]

    class Fake(cls):
        def __init__(self):
            self.Lab, self.L, self.device = LAB, L, torch.device('cpu')
            self.region = torch.ones(L, dtype=torch.uint8)
            self.gt_atom14, self.gt_seq = torch.zeros(L, 14, 3), torch.zeros(L, dtype=torch.int64)
            self.want_rows = self.want_planes = want
            if built_on is not None:
                self.interface = built_on

        def score(self, *args, **kwargs):
            atoms = args[-2]
            log.append((kw, atoms, dict(kwargs, first=args[0])))
            table = torch.full((atoms.shape[0], len(cls.COLUMNS)), float(len(log)), dtype=torch.float64)
            if kw == 'confidence':
                return (table, torch.zeros(atoms.shape[0], L, 4), ('p_contact', 'exp_dist'))[:3 if kwargs.get('planes') else 2]
            if kw == 'accuracy' and kwargs.get('rows'):
                return table, torch.zeros(atoms.shape[0], L, 4, dtype=torch.float64), None, None
            return table

    return Fake()


class Relaxer:
    def __init__(self, log):
        self.log = log

    def relax(self, x, seq):
        self.log.append(('relaxer', x, {}))
        return x + 1.0, torch.zeros(x.shape[0], len(relax.RELAX_COLUMNS), dtype=torch.float64)


class Scorer:
    def __init__(self, log):
        self.log = log

    def new_table(self, *lead):
        return torch.empty(*lead, len(metrics.SCORE_COLUMNS), dtype=torch.float64)

    def score(self, x, seq, out=None):
        self.log.append(('scorer', x, {}))
        return torch.zeros(x.shape[0], len(metrics.SCORE_COLUMNS), dtype=torch.float64)


def sample(**kw):
    """sampler.sample_fn on one grid point of a stand-in network: one record, the last."""
    g = torch.Generator().manual_seed(1)
    out = {'heads': {'folding': {'rigids': torch.randn(B, L, 7, generator=g), 'final_atom14_positions': torch.randn(B, L, 14, 3, generator=g)},
                     'sequence_module': {'seq_0': torch.randint(0, 20, (B, L), generator=g)},
                     'predicted_lddt': {'pLDDT': torch.rand(B, L, generator=g)}},
           'representations': {'pair': torch.randn(B, L, L, 4, generator=g)}}
    batch = {'rigids_t': torch.randn(B, L, 7, generator=g), 'seq_t': torch.zeros(B, L, dtype=torch.int64), 'anchor_flag': torch.zeros(B, LAB),
             'atom14_gt_exists': torch.ones(B, L, 14), 'fixed_mask': torch.zeros(B, L)}
    embed = SimpleNamespace(embed_self_conditioning=False)
    cfg = SimpleNamespace(model=SimpleNamespace(heads=SimpleNamespace(diffusion_module=SimpleNamespace(embed=embed))))
    traj = sampler.sample_fn(batch, cfg, None, lambda b: out, num_t=1, self_condition=False, **kw)
    assert len(traj) == 1
    return traj[0], out


def test_no_scorer_leaves_the_record_as_it_is():
    rec, out = sample()
    assert set(rec) == TODAY
    assert torch.equal(rec['atom14_results'], out['heads']['folding']['final_atom14_positions'][:, :LAB])
    assert torch.equal(rec['seq'], out['heads']['sequence_module']['seq_0'][:, :LAB]) and torch.equal(rec['rigids_t'], out['heads']['folding']['rigids'])
    params = inspect.signature(sampler.sample_fn).parameters
    assert all(params[k].default is None for k in ORDER + ['scorer', 'relaxer'])
    assert list(inspect.signature(sampler._analyse_last).parameters) == ['rec', 'out', 'pl_res', 'scorer', 'relaxer', 'scorers']


@pytest.mark.parametrize('want', [False, True], ids=['rows_off', 'rows_on'])
@pytest.mark.parametrize('relaxed', [False, True], ids=['plain', 'relaxer'])
def test_every_keyword_adds_its_keys_in_order(relaxed, want):
    log = []
    scorers = {kw: fake(kw, log, want=want) for kw in reversed(ORDER)}          # (passed by name: their order is sample_fn's, not the caller's)
    for kw in ('polar', 'developability', 'shape', 'patches'):
        scorers[kw].interface = scorers['interface']
    rec, out = sample(scorer=Scorer(log), relaxer=Relaxer(log) if relaxed else None, **scorers)
    expected = TODAY | {'scores'} | ({'atom14_relaxed', 'relax', 'scores_relaxed'} if relaxed else set())
    for always, with_relaxer, with_rows in KEYS.values():
        expected |= set(always) | (set(with_relaxer) if relaxed else set()) | (set(with_rows) if want else set())
    assert set(rec) == expected
    x, xr = rec['atom14_results'], rec.get('atom14_relaxed')
    assert not relaxed or torch.equal(xr, x + 1.0)
    # scorer on the record, the relaxer and the scorer on its structures, then every analysis: the design before the relaxed structure
    calls = [(kw, 'wild' if k.get('wild') else 'relaxed' if atoms is xr else 'design' if torch.equal(atoms, x) else '?') for kw, atoms, k in log]
    per = lambda kw: [(kw, 'design')] + ([(kw, 'wild')] if kw == 'confidence' else []) + ([(kw, 'relaxed')] if relaxed else [])
    assert calls == [('scorer', 'design')] + ([('relaxer', 'design'), ('scorer', 'relaxed')] if relaxed else []) + [c for kw in ORDER for c in per(kw)]
    conf = [k for kw, _, k in log if kw == 'confidence']
    assert conf[0].get('planes') is want and conf[1].get('wild') is True            # confidence: the designs, then the wild type under the same pair
    assert len(conf) == (3 if relaxed else 2) and all(k['first'] is out['representations']['pair'] for k in conf)
    for kw, (always, with_relaxer, _) in KEYS.items():
        n = len(CLASSES[kw].COLUMNS)
        assert rec[kw].shape == (B, n) and rec[kw].dtype == torch.float64 and (not relaxed or rec[kw + '_relaxed'].shape == (B, n)), kw
    assert rec['torsions_classes'].shape == rec['secondary_classes'].shape == (B, LAB) and rec['torsions_classes'].dtype == torch.int32
    if want:
        assert rec['polar_bonds'].shape == (B, L, 14, 2) and rec['polar_rows'].shape == (B, L, 4) and rec['polar_rows'].dtype == torch.int32
        assert rec['developability_rows'].shape == rec['patches_rows'].shape == (B, L, 4) and rec['patches_rows'].dtype == torch.float64
        assert rec['torsions_rows'].shape == (B, LAB, 8) and rec['secondary_rows'].shape == (B, LAB, 6) and rec['confidence_planes'] == ('p_contact', 'exp_dist')
    # the side outputs go to the call on the designs only, and are the record's own tensors
    for kw, atoms, k in log:
        side = {s: v for s, v in k.items() if s in ('rows', 'bonds', 'classes') and v is not None and v is not True}
        assert not side or atoms is not xr, kw
        assert all(rec[f'{kw}_{s}'] is v for s, v in side.items()), kw
    acc = [k for kw, _, k in log if kw == 'accuracy']
    assert all(k['plddt'] is out['heads']['predicted_lddt']['pLDDT'] for k in acc) and acc[0].get('rows') is True


@pytest.mark.parametrize('relaxed', [False, True], ids=['plain', 'relaxer'])
def test_point_counts_are_shared_with_the_scorers_built_on_the_interface_scorer(relaxed):
    log = []
    it = fake('interface', log)
    pol, pat = fake('polar', log, built_on=it), fake('patches', log, built_on=it)
    own = fake('shape', log, built_on=fake('interface', log))
    rec, _ = sample(relaxer=Relaxer(log) if relaxed else None, interface=it, polar=pol, shape=own, patches=pat)
    sets = ['design'] + (['relaxed'] if relaxed else [])
    by = {kw: [k.get('points') for name, _, k in log if name == kw] for kw in ('interface', 'polar', 'shape', 'patches')}
    assert all(len(v) == len(sets) for v in by.values())                        # interface.score once per structure set
    for k, _ in enumerate(sets):
        buf = by['interface'][k]
        assert buf.shape == (B, L, 14, 2) and buf.dtype == torch.int32
        assert by['polar'][k] is buf and by['patches'][k] is buf and by['shape'][k] is None
    assert not relaxed or by['interface'][0] is not by['interface'][1]
    # without a user no buffer is made: the interface scorer is called as it was before there were any
    log.clear()
    sample(relaxer=Relaxer(log) if relaxed else None, interface=it, shape=own)
    assert [k.get('points') for name, _, k in log if name in ('interface', 'shape')] == [None] * (2 * len(sets))
