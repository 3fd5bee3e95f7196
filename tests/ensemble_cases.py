"""Inputs shared by the ensemble tests (tests/test_ensemble_host.py, tests/test_gpu_ensemble.py): a seeded synthetic ensemble whose
clusters are known by construction, and the float64 host twin's answer for it, computed once per (arguments) and never modified."""
import functools

import numpy as np


def random_walk(rng, M, step=3.8):
    """(M,3) C-alpha trace: steps of `step` Angstrom in uniformly random directions."""
    d = rng.normal(size=(M, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.cumsum(step * d, axis=0)


def make_ensemble(seed=0, N=24, M=8, L=None, rows=None, n_base=3, sigma=0.15, special=True):
    """N designs of an L-row antibody whose M region rows carry one of n_base base loops (design k: base k % n_base) plus N(0, sigma^2)
    noise per coordinate, everything rounded to float32.  A base loop: a 3.8 A C-alpha random walk with N, C, O placed 1.46, 1.52 and
    2.40 A from their C-alpha in random directions.  Rows outside the region differ from design to design (they must not matter).  special (N >= 8):
    design 5 is a copy of design 4 (coordinates and tokens); design 7 is design 6 rotated by 0.7 rad about z and shifted by (3, -2, 1),
    rounded to float32.  rows: the region rows (default: M contiguous rows starting at 3).
    -> x (N, L, 14, 3) float32, seq (N, L) int64, region (L) bool."""
    rng = np.random.default_rng(seed)
    rows = np.arange(3, 3 + M) if rows is None else np.asarray(rows)
    assert rows.shape[0] == M
    L = int(rows.max()) + 4 if L is None else L
    bases, tokens = [], []
    for _ in range(n_base):
        ca = random_walk(rng, M)
        off = rng.normal(size=(M, 4, 3))
        off /= np.linalg.norm(off, axis=2, keepdims=True)
        bb = ca[:, None] + np.array([1.46, 0.0, 1.52, 2.40])[None, :, None] * off       # |CA-N|, |CA-C|, |CA-O|
        bases.append(bb)
        tokens.append(rng.integers(0, 20, M))
    x = rng.normal(scale=8.0, size=(N, L, 14, 3))
    seq = rng.integers(0, 20, (N, L))
    for k in range(N):
        x[k, rows, :4] = bases[k % n_base] + rng.normal(scale=sigma, size=(M, 4, 3))
        seq[k, rows] = tokens[k % n_base]
        mut = rng.random(M) < 0.25
        seq[k, rows[mut]] = rng.integers(0, 20, int(mut.sum()))
    x = x.astype(np.float32)
    if special and N >= 8:
        x[5], seq[5] = x[4], seq[4]
        c, s = np.cos(0.7), np.sin(0.7)
        Rz = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
        x[7] = (x[6].astype(np.float64) @ Rz.T + np.array([3.0, -2.0, 1.0])).astype(np.float32)
        seq[7] = seq[6]
    region = np.zeros(L, bool)
    region[rows] = True
    return x, seq.astype(np.int64), region


@functools.lru_cache(maxsize=None)
def case(seed=0, N=24, M=8, atoms='backbone', metric='fit', cutoff=1.0, rows=None, kind='walk'):
    """(x, seq, region, host answer) of a named case; cached, shared between tests, read-only.
    kind: 'walk' (make_ensemble), 'collinear' / 'planar' (M = 3 C-alpha on a line / in general position, per-design noise),
    'mirror' (design 1 is design 0 with x -> -x)."""
    from abx_amd import ensemble
    x, seq, region = make_ensemble(seed, N, M, rows=None if rows is None else np.array(rows))
    r = np.nonzero(region)[0]
    if kind == 'collinear':                             # exactly collinear in float32: multiples of one representable direction
        rng = np.random.default_rng(seed + 100)
        for k in range(N):
            o, d = rng.integers(-8, 9, 3).astype(np.float32), np.array([1.0, 0.5, -0.25], np.float32) * (1 + k % 3)
            for m in range(M):
                x[k, r[m], 1] = o + d * np.float32(m * (1 + 0.5 * (k % 2)))
    elif kind == 'mirror':
        x[1] = x[0] * np.array([-1.0, 1.0, 1.0], np.float32)
    for a in (x, seq, region):
        a.setflags(write=False)
    host = ensemble.ensemble_host(x, seq, region, atoms=atoms, metric=metric, cutoff=cutoff)
    for a in (host['planes'], host['table'], host['centres']):
        a.setflags(write=False)
    return x, seq, region, host
