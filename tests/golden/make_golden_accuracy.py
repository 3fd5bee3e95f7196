"""Golden vectors for the accuracy analysis (abx_amd.accuracy), produced by the UNMODIFIED reference:

    python tests/golden/make_golden_accuracy.py          -> tests/golden/accuracy.npz

`lddt` (abx/model/utils.py:102-155) on the C-alpha atoms with per_residue True and False, `lddt_ca_torch` (abx/utils.py:623-666) and the
loop of TMscoreHead.forward (abx/model/head.py:131-138: Kabsch -> TMscore, plus GDT TS / HA and RMSD of the same aligned sets) on two
seeded perturbations of the first 40 antibody residues of the shipped 6qd7 complex (pdb_6qd7.npz): a mask with holes, one residue
moved out of every other residue's inclusion radius, a rigid motion on top of the noise.
The reference decides in fp32 (and lddt_ca_torch with <= where lddt uses <), so the fixture keeps every pair at least 1e-3 A away
from the inclusion radius and from the four thresholds: asserted here in float64.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_shims  # noqa: E402

ref_shims.install()
from abx import utils as ref_utils  # noqa: E402
from abx.model import utils as ref_model_utils  # noqa: E402

assert ref_utils.__file__.startswith(ref_shims.REF) and ref_model_utils.__file__.startswith(ref_shims.REF)
N = 40
z = np.load(os.path.join(HERE, 'pdb_6qd7.npz'))
true = z['batch.atom14_gt_positions'][0, :N].astype(np.float32).copy()
exists = z['batch.atom14_gt_exists'][0, :N].astype(bool).copy()
seq = z['batch.seq'][0, :N].astype(np.int64)
true[17] += np.float32(80.0)                        # a residue without neighbours inside the radius
exists[[3, 22, 23]] = False                         # holes: whole residues ...
exists[9, 1] = False                                # ... and a residue without its C-alpha
rng = np.random.default_rng(2026)
out = dict(true=true, exists=exists, seq=seq, radius=np.float64(15.0))
cases = []
for ci, sigma in enumerate((0.4, 1.6)):
    # redrawn from the one seeded stream until no decision of the case is near a boundary (float64 from the stored float32 values):
    # ~1000 included pairs x 4 thresholds leave a draw about one chance in ten
    for attempt in range(1000):
        q = rng.normal(size=4)
        a, b, c, d = q / np.linalg.norm(q)
        R = np.array([[a * a + b * b - c * c - d * d, 2 * (b * c - a * d), 2 * (b * d + a * c)],
                      [2 * (b * c + a * d), a * a - b * b + c * c - d * d, 2 * (c * d - a * b)],
                      [2 * (b * d - a * c), 2 * (c * d + a * b), a * a - b * b - c * c + d * d]])
        noise = sigma * rng.normal(size=(N, 1, 3)) + 0.3 * sigma * rng.normal(size=true.shape)
        pred = ((true.astype(np.float64) + noise) @ R.T + rng.normal(size=3) * 10).astype(np.float32)
        m = exists[:, 1]
        ct, cp = true[m, 1].astype(np.float64), pred[m, 1].astype(np.float64)
        dt = np.sqrt(((ct[:, None] - ct[None]) ** 2).sum(-1))
        dp = np.sqrt(((cp[:, None] - cp[None]) ** 2).sum(-1))
        off = ~np.eye(len(ct), dtype=bool)
        assert np.abs(dt[off] - 15.0).min() > 1e-3, np.abs(dt[off] - 15.0).min()
        inc = off & (dt < 15.0)
        margin = min(np.abs(np.abs(dt - dp)[inc] - t).min() for t in (0.5, 1.0, 2.0, 4.0))
        if margin > 1e-3:
            break
    assert margin > 1e-3, margin
    tt, tp, tm = torch.from_numpy(true[:, 1]), torch.from_numpy(pred[:, 1]), torch.from_numpy(m.astype(np.float32))
    key = f'c{ci}'
    out[key + '.pred'] = pred
    out[key + '.lddt_per_residue'] = ref_model_utils.lddt(tp[None], tt[None], tm[None, :, None], per_residue=True)[0].numpy()
    out[key + '.lddt_pooled'] = ref_model_utils.lddt(tp[None], tt[None], tm[None, :, None], per_residue=False)[0].numpy()
    out[key + '.lddt_ca_torch'] = ref_utils.lddt_ca_torch(torch.from_numpy(true)[None], torch.from_numpy(pred)[None],
                                                          torch.from_numpy(exists)[None])[0].numpy()
    # TMscoreHead.forward, head.py:131-138
    mask = torch.from_numpy(m)
    pred_aligned, label_aligned = ref_utils.Kabsch(tp[mask].t(), tt[mask].t())
    L = int(mask.sum())
    out[key + '.tm_score'] = ref_utils.TMscore(pred_aligned[None], label_aligned[None], L=L).numpy()
    out[key + '.gdt_ts'] = ref_utils.GDT(pred_aligned[None], label_aligned[None], mode='TS').numpy()
    out[key + '.gdt_ha'] = ref_utils.GDT(pred_aligned[None], label_aligned[None], mode='HA').numpy()
    out[key + '.rmsd'] = ref_utils.RMSD(pred_aligned[None], label_aligned[None]).numpy()
    cases.append(key)
    print(key, 'margin', margin, {k[len(key) + 1:]: np.round(np.asarray(v, np.float64).reshape(-1)[:4], 4).tolist()
                                  for k, v in out.items() if k.startswith(key + '.') and k != key + '.pred'})
out['cases'] = np.array(cases)
path = os.path.join(HERE, 'accuracy.npz')
np.savez_compressed(path, **out)
print('wrote', path, os.path.getsize(path) // 1024, 'KiB')
