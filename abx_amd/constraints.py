"""Opt-in sequence constraints of the reverse process: forbid, fix and bias residue letters where a token is decided.  The reference
samples WITHOUT them (discrete_diffuser.py:150-188 and head.py:166-167 take what the network and the tau-leaping step produce), so this
is an extension: default off, and with `constraints=None` the sampler executes exactly the unconstrained code path (bit-identical, tested).

One table carries all three controls: `seq_bias`, float32 (L, 20) on the device, shared by all samples of the complex.  An entry is a
finite logit bias (0: no opinion) or -inf (this letter is forbidden at this residue).  Rows of residues that are not designed are zero and
every designed row keeps a finite entry; +inf and NaN are refused.  The two kernels that decide a token read it (include/abx_hip.h):
`abx_reverse_step` (AbxReverseArgs.seq_bias: softmax over logits + bias, no Poisson rate towards a forbidden letter, a leap that lands on
one is rejected) and `abx_seq_head_atoms_biased` (seq_0 = argmax(logits + bias), from which the side-chain atoms are built).  The logits
a caller sees stay the network's own.

Grammar.  A residue is named as in the guidance, `<chain letter>:<residue index as featurised>` (guidance._find_row).
    bias file   lines `RES|* LETTERS VALUE`; VALUE a float or -inf; `*` = every designed residue; `#` starts a comment; lines apply in
                order, a later one overwrites an earlier one
    forbid      letters forbidden at every designed residue (the same as `* LETTERS -inf` after the file)
    fix         `RES=LETTERS`: only these letters at RES; applied last, it wins over a global forbid, and the kept letters keep their
                file bias
The host twins of the device rules (numpy, no GPU needed): `masked_argmax_host`, `project_host`, `token_step_host`."""
import numpy as np
import torch

from abx_amd import residue_constants as rc
from abx_amd.guidance import _find_row, _rows_of

LETTERS = ''.join(rc.restypes)                         # the token order of the network: ARNDCQEGHILKMFPSTWYV
NEG_INF = float('-inf')


# -------------------------------------------------------------------------------------------------------------------
# host twins
# -------------------------------------------------------------------------------------------------------------------
def masked_argmax_host(logits, bias):
    """argmax(logits + bias) in float32, first maximum wins.  logits (..., L, 20), bias (L, 20) -> int64 (..., L)."""
    v = np.asarray(logits, np.float32) + np.asarray(bias, np.float32)
    return np.argmax(v, axis=-1).astype(np.int64)


def nearest_allowed(allowed):
    """(L, 20) bool -> (L, 20) int64: for every letter the allowed letter nearest in index, the lower on a tie (itself when it is
    allowed, or when the row allows nothing)."""
    allowed = np.asarray(allowed, bool)
    idx = np.arange(20)
    d = np.abs(idx[None, :, None] - idx[None, None, :]).astype(np.int64)             # (1, from, to)
    d = np.where(allowed[:, None, :], d, 1 << 20)
    near = np.argmin(d, axis=-1)                                                     # first minimum: the lower index on a tie
    return np.where(allowed.any(-1)[:, None], near, idx[None, :]).astype(np.int64)


def project_host(seq_t, allowed, diffuse_mask):
    """The start-state rule: a designed residue's forbidden token becomes the allowed letter nearest in index, the lower on a tie;
    every other token stays.  seq_t (..., L) int, allowed (L, 20) bool, diffuse_mask (..., L) or (L) -> int64 (..., L)."""
    seq_t = np.asarray(seq_t, np.int64)
    allowed = np.asarray(allowed, bool)
    c = np.clip(seq_t, 0, 19)
    rows = np.broadcast_to(np.arange(allowed.shape[0]), seq_t.shape)
    bad = (np.broadcast_to(np.asarray(diffuse_mask), seq_t.shape) != 0) & ~allowed[rows, c]
    return np.where(bad, nearest_allowed(allowed)[rows, c], seq_t)


def token_step_host(x_t, jumps, allowed):
    """The landing-and-rejection rule of the constrained token step on given jump counts: the ordinal landing token
    clamp(x_t + sum_s jumps[s] * (s - x_t)) (discrete_diffuser.py:184-188; two jumps can land on a letter neither aimed at), and when
    that letter is forbidden the leap is rejected and the (clamped) token stays.  x_t (..., L) int, jumps (..., L, 20), allowed (L, 20)
    bool -> int64 (..., L)."""
    xt = np.clip(np.asarray(x_t, np.int64), 0, 19)
    allowed = np.asarray(allowed, bool)
    diffs = (np.arange(20)[None, :] - xt[..., None]).astype(np.float32)
    overall = np.zeros(xt.shape, np.float32)
    for s in range(20):                                                              # the kernel's fp32 accumulation order
        overall = overall + np.asarray(jumps, np.float32)[..., s] * diffs[..., s]
    land = np.clip(xt.astype(np.float32) + overall, 0.0, 19.0).astype(np.int64)
    rows = np.broadcast_to(np.arange(allowed.shape[0]), xt.shape)
    return np.where(allowed[rows, land], land, xt)


# -------------------------------------------------------------------------------------------------------------------
# the table
# -------------------------------------------------------------------------------------------------------------------
def _letters(text, where):
    out = []
    for c in text:
        if c not in LETTERS:
            raise SystemExit(f'{where}: unknown residue letter {c!r} (the 20 letters: {"".join(sorted(LETTERS))})')
        out.append(LETTERS.index(c))
    if not out:
        raise SystemExit(f'{where}: no residue letter given')
    return out


def _value(text, where):
    try:
        v = float(text)
    except ValueError:
        raise SystemExit(f'{where}: expected a number or -inf, not {text!r}')
    if np.isnan(v) or v == float('inf'):
        raise SystemExit(f'{where}: the bias must be finite or -inf, not {text!r}')
    return v


def check_table(table, diffuse_mask, names=None):
    """The host checks of a (L, 20) table against the (L) mask of the designed residues; SystemExit names the residue."""
    t = np.asarray(table, np.float32)
    dm = np.asarray(diffuse_mask) != 0
    if t.ndim != 2 or t.shape[1] != 20 or t.shape[0] != dm.shape[0]:
        raise SystemExit(f'sequence bias: expected a ({dm.shape[0]}, 20) table, not {t.shape}')
    name = (lambda r: names[r]) if names is not None else (lambda r: f'row {r}')
    for r in range(t.shape[0]):
        if np.isnan(t[r]).any() or (t[r] == np.inf).any():
            raise SystemExit(f'residue {name(r)}: the sequence bias must be finite or -inf (found NaN or +inf)')
        if not dm[r] and (t[r] != 0).any():
            raise SystemExit(f'residue {name(r)} is not designed: its row of the sequence bias must be zero')
        if dm[r] and not np.isfinite(t[r]).any():
            raise SystemExit(f'residue {name(r)}: no allowed letter left')


class SequenceConstraints:
    """The sequence-constraint table of one featurised complex.  batch_one: a featurised batch (its sample 0 is read: the complex and
    the designed residues are the same in every sample); chains: the chain letters in the order of the chain ids (heavy 0, light 1,
    the k-th antigen chain 2 + k); bias_file: path of a bias file or None; forbid: letters (strings of letters); fix: `RES=LETTERS`
    tokens.  -> .table float32 (L, 20) on the batch's device, .host its numpy copy, .allowed (L, 20) bool numpy."""

    def __init__(self, batch_one, chains, bias_file=None, forbid=(), fix=(), device=None):
        chain_id, residx, seq = _rows_of(batch_one)
        first = lambda k: (batch_one[k][0] if batch_one[k].dim() > (2 if k == 'atom14_gt_exists' else 1) else batch_one[k])
        dm = ((1 - first('fixed_mask').cpu().long()) * first('atom14_gt_exists')[..., 0].cpu().long()).numpy() != 0
        L = len(seq)
        chains = list(chains)
        self.names = [f'{chains[c] if 0 <= c < len(chains) else "?"}:{n}' for c, n in zip(chain_id, residx)]
        self.wild = ''.join(LETTERS[a] if 0 <= a < 20 else 'X' for a in seq)
        self.diffuse_mask = dm
        designed = np.nonzero(dm)[0]

        def rows_of(token, where):
            if token == '*':
                return designed
            r = _find_row(token, batch_one, chains)
            if not dm[r]:
                raise SystemExit(f'{where}: residue {token!r} is not designed (the designed residues: '
                                 f'{" ".join(self.names[i] for i in designed)})')
            return np.array([r])

        table = np.zeros((L, 20), np.float32)
        if bias_file:
            with open(bias_file) as f:
                for ln, line in enumerate(f, 1):
                    w = line.split('#')[0].split()
                    if not w:
                        continue
                    where = f'{bias_file}:{ln}'
                    if len(w) != 3:
                        raise SystemExit(f'{where}: expected `RES|* LETTERS VALUE`')
                    rows, cols, v = rows_of(w[0], where), _letters(w[1], where), _value(w[2], where)
                    table[np.ix_(rows, cols)] = v
        from_file = table.copy()
        cols = sorted({c for text in forbid for c in _letters(text, '--seq_forbid')})
        if cols:
            table[np.ix_(designed, cols)] = NEG_INF
        for token in fix:
            where = f'--seq_fix {token}'
            if token.count('=') != 1:
                raise SystemExit(f'{where}: expected RES=LETTERS')
            res, text = token.split('=')
            if res == '*':
                raise SystemExit(f'{where}: name one residue')
            r, keep = rows_of(res, where)[0], _letters(text, where)
            row = np.full(20, NEG_INF, np.float32)
            row[keep] = from_file[r, keep]
            table[r] = row
        check_table(table, dm, self.names)
        self._set(table, device if device is not None else batch_one['seq'].device)

    @classmethod
    def from_table(cls, table, diffuse_mask, names=None, wild=None, device='cpu'):
        """Constraints of a caller's own (L, 20) table, after the same host checks."""
        self = cls.__new__(cls)
        t = np.array(torch.as_tensor(table).cpu().numpy() if torch.is_tensor(table) else table, np.float32)
        dm = np.asarray(torch.as_tensor(diffuse_mask).cpu().numpy()) != 0
        self.names = list(names) if names is not None else [f'row {r}' for r in range(t.shape[0])]
        self.wild = wild if wild is not None else 'X' * t.shape[0]
        self.diffuse_mask = dm
        check_table(t, dm, self.names)
        self._set(t, device)
        return self

    def _set(self, table, device):
        self.host = np.ascontiguousarray(table, np.float32)
        self.allowed = self.host != NEG_INF
        self.table = torch.from_numpy(self.host.copy()).to(device).contiguous()
        self._allowed_dev = torch.from_numpy(self.allowed.copy()).to(device)
        self._nearest_dev = torch.from_numpy(nearest_allowed(self.allowed)).to(device)

    def project(self, seq_t, diffuse_mask):
        """The start state on the device (project_host's rule): elementwise operations, no random number, no host synchronisation.
        seq_t (B, L) int64, diffuse_mask (B, L) -> (B, L) int64."""
        L = self.host.shape[0]
        assert seq_t.shape[-1] == L, (tuple(seq_t.shape), L)
        c = torch.clamp(seq_t, 0, 19).long()
        rows = torch.arange(L, device=seq_t.device).expand_as(c)
        bad = diffuse_mask.bool() & ~self._allowed_dev.to(seq_t.device)[rows, c]
        return torch.where(bad, self._nearest_dev.to(seq_t.device)[rows, c].to(seq_t.dtype), seq_t)

    def describe(self):
        """One entry per designed residue: (row, name, wild letter, allowed letters in token order)."""
        return [(int(r), self.names[r], self.wild[r], ''.join(LETTERS[s] for s in range(20) if self.allowed[r, s]))
                for r in np.nonzero(self.diffuse_mask)[0]]

    def report_lines(self, seq):
        """The lines of <complex>_sequence.tsv from the designed sequences seq (N, >= last designed row + 1) int: a header, then per
        designed residue its name, the wild letter, the allowed letters, the count of each of the 20 letters among the N designs and
        `violations`, the number of designs that carry a forbidden letter there."""
        seq = np.asarray(torch.as_tensor(seq).cpu().numpy() if torch.is_tensor(seq) else seq, np.int64)
        lines = ['\t'.join(['residue', 'wild', 'allowed'] + list(LETTERS) + ['violations'])]
        for r, name, wild, letters in self.describe():
            col = np.clip(seq[:, r], 0, 19)
            counts = np.bincount(col, minlength=20)
            bad = int((~self.allowed[r, col]).sum())
            lines.append('\t'.join([name, wild, letters] + [str(int(c)) for c in counts] + [str(bad)]))
        return lines

    def write_report(self, path, seq):
        with open(path, 'w') as f:
            f.write('\n'.join(self.report_lines(seq)) + '\n')
        return path
