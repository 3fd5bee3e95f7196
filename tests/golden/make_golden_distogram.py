"""Golden vectors for the distogram head (abx/model/head.py:26-44) and the contact definition its metric head consumes
(head.py:90-113), produced by the UNMODIFIED reference:

    python tests/golden/make_golden_distogram.py          -> tests/golden/distogram_head.npz

The reference's DistogramHead is instantiated with the shipped config (config/config_model.json, heads.distogram); its projection is
zero-initialised (init='final'), so weight and bias are overwritten with seeded normal values.  Input: a seeded, asymmetric pair
tensor (2, 11, 11, 192) with entries of both signs.  Stored: the inputs, `logits` and `breaks` of DistogramHead.forward, and for one
seeded coordinate set what MetricDictHead.forward hands to contact_precision (`pred` = sum softmax(logits)[..., :t+1], `truth`) and
the (range, ratio, precision) triples it gets back (read from the function's frame when it returns: nothing in the reference is
edited).  Data only.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import ref_shims  # noqa: E402

ref_shims.install()
import torch  # noqa: E402
from ref_shims import ConfigDict  # noqa: E402

from abx.model import head as ref_head  # noqa: E402

assert ref_head.__file__.startswith(ref_shims.REF)

cfg = ConfigDict(json.load(open(os.path.join(ref_shims.REF, 'config', 'config_model.json'))))
dconf = cfg.model.heads.distogram
pair_channel = cfg.model.embeddings_and_seqformer.pair_channel
B, L = 2, 11

torch.manual_seed(0)
head = ref_head.DistogramHead(dconf, pair_channel)
C = head.proj.weight.shape[1]
assert tuple(head.proj.weight.shape) == (dconf.num_bins, 192) and float(head.proj.weight.detach().abs().max()) == 0.0     # init='final'
g = torch.Generator().manual_seed(41)
with torch.no_grad():
    head.proj.weight.copy_(0.1 * torch.randn(dconf.num_bins, C, generator=g))
    head.proj.bias.copy_(0.5 * torch.randn(dconf.num_bins, generator=g))
z = torch.randn(B, L, L, C, generator=g)
assert float((z - z.transpose(1, 2)).abs().max()) > 1.0 and float(z.min()) < 0 < float(z.max())
with torch.no_grad():
    ret = head(None, {'pair': z}, None)
logits, breaks = ret['logits'], ret['breaks']

# MetricDictHead on a seeded coordinate set: pred / truth / the precision triples
pos = 6.0 * torch.randn(B, L, 3, generator=g)
mask = torch.ones(B, L)
mask[1, 4] = 0.0
grabbed = {}


def prof(frame, event, arg):
    if event == 'return' and frame.f_code.co_name == 'forward' and 'precision_list' in frame.f_locals:
        for k in ('pred', 'truth', 'precision_list', 'cutoff', 't'):
            grabbed[k] = frame.f_locals[k]


metric = ref_head.MetricDictHead(ConfigDict({}))
sys.setprofile(prof)
try:
    with torch.no_grad():
        out = metric({'distogram': {'logits': logits, 'breaks': breaks}}, None, {'pseudo_beta': pos, 'pseudo_beta_mask': mask})
finally:
    sys.setprofile(None)
triples = []
for (i, j), ratio, precision in grabbed['precision_list'] if isinstance(grabbed['precision_list'], list) else []:
    triples.append((float(i if i is not None else 0), float(j if j is not None else -1), float(ratio), float(precision)))
if not triples:          # (a generator: consumed by the reference itself; its values travel in the returned metrics)
    for key, precision in out['loss']['contact'].items():
        rng, ratio = key.split('_')
        i, j = rng.strip('[)').split(',')
        triples.append((float(i), -1.0 if j == 'inf' else float(j), float(ratio), float(precision)))
assert len(triples) == 12, triples

# the twin's logits against the reference's own, under the fp32 dot-product bound of tests/test_distogram_host.py
from abx_amd.confidence import distogram_host  # noqa: E402

tw = distogram_host(z, head.proj.weight, head.proj.bias, breaks, pos, np.ones(L, np.uint8), mask, 8.0)
err = np.abs(tw['logits'] - logits.numpy().astype(np.float64))
bound = (192 + 2) * 2.0 ** -24 * tw['bound_scale']
print('max |twin - reference| logits', err.max(), 'largest share of the bound', (err / bound).max())
assert (err <= bound).all()
print('t =', int(grabbed['t']), 'cutoff', grabbed['cutoff'], 'pred in', float(grabbed['pred'].min()), float(grabbed['pred'].max()))
for tr in triples:
    print('range [%g,%g) ratio %g precision %g' % tr)

path = os.path.join(HERE, 'distogram_head.npz')
np.savez_compressed(path, pair=z.numpy(), weight=head.proj.weight.detach().numpy(), bias=head.proj.bias.detach().numpy(),
                    logits=logits.numpy(), breaks=breaks.numpy(), positions=pos.numpy(), mask=mask.numpy(),
                    pred=grabbed['pred'].numpy(), truth=grabbed['truth'].numpy(), cutoff=np.float64(grabbed['cutoff']),
                    t=np.int64(int(grabbed['t'])), triples=np.array(triples, dtype=np.float64))
print('wrote distogram_head.npz', os.path.getsize(path) // 1024, 'KiB')
