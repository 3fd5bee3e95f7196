"""Sequence constraints on the host (abx_amd.constraints): the grammar and its error texts, the table built from file + forbid + fix with
the precedence rule, the start-state projection, the landing-and-rejection rule of the token step on hand-made jump counts, the
masked argmax and the report writer.  No GPU."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

PDB = os.path.join(GOLDEN, 'pdb', '6ct7_H_L_S.pdb')
CHAINS = ['H', 'L', 'S']
NINF = float('-inf')


@pytest.fixture(scope='module')
def one():
    """The shipped 6ct7 complex with the H3 residues designed as the feature pipeline marks them (features.make_diffuser_features:
    the columns opening anchor + 1 ... closing anchor - 2)."""
    from abx_amd import residue_constants as rc
    from abx_amd.data.antibody import load_complex
    cb = load_complex(PDB, seed=0)
    b = {k: v for k, v in cb.items() if torch.is_tensor(v)}
    pos = torch.nonzero(b['anchor_flag'][0] == rc.cdr_str_to_enum['H3'])[:, 0].tolist()
    assert len(pos) == 2
    fixed = torch.ones_like(b['mask'], dtype=torch.int32)
    fixed[0, pos[0] + 1:pos[1] - 1] = 0
    b['fixed_mask'] = fixed
    return b


def _cons(one, **kw):
    from abx_amd.constraints import SequenceConstraints
    return SequenceConstraints(one, CHAINS, **kw)


def _designed(one):
    return np.nonzero((1 - one['fixed_mask'][0].numpy()) * one['atom14_gt_exists'][0, :, 0].numpy())[0]


def test_table_from_file_forbid_and_fix(one, tmp_path):
    from abx_amd.constraints import LETTERS
    assert LETTERS == 'ARNDCQEGHILKMFPSTWYV'
    rows = _designed(one)
    assert rows.tolist() == [98, 99, 100]
    c0 = _cons(one)
    name = c0.names
    assert name[98] == 'H:98' and all(name[r].startswith('H:') for r in rows)
    assert c0.host.shape == (one['seq'].shape[1], 20) and not c0.host.any() and c0.allowed.all()
    assert c0.table.dtype == torch.float32 and tuple(c0.table.shape) == c0.host.shape
    r0, r1, r2 = (int(r) for r in rows[:3])
    f = tmp_path / 'bias.txt'
    f.write_text(f'# soft preferences\n* SGY 1.5\n{name[r0]} Y 3   # the anchor\n\n{name[r1]} W -inf\n{name[r0]} C 0.25\n* G 0.5\n')
    ix = lambda s: [LETTERS.index(c) for c in s]
    c1 = _cons(one, bias_file=str(f))
    want = np.zeros_like(c0.host)
    want[np.ix_(rows, ix('SY'))] = 1.5
    want[np.ix_(rows, ix('G'))] = 0.5                                   # a later line overwrites an earlier one
    want[r0, ix('Y')] = 3.0
    want[r0, ix('C')] = 0.25
    want[r1, ix('W')] = NINF
    assert np.array_equal(c1.host, want) and np.array_equal(c1.table.numpy(), want)
    assert np.array_equal(c1.allowed, want != NINF)
    # forbid = `* LETTERS -inf` after the file; two spellings of the same set
    c2 = _cons(one, bias_file=str(f), forbid=['C', 'M'])
    want2 = want.copy()
    want2[np.ix_(rows, ix('CM'))] = NINF
    assert np.array_equal(c2.host, want2)
    assert np.array_equal(_cons(one, bias_file=str(f), forbid=['CM']).host, want2)
    # fix is applied last and wins over the global forbid; the kept letters keep their FILE bias (C 0.25 at r0, not -inf)
    c3 = _cons(one, bias_file=str(f), forbid=['C', 'M'], fix=[f'{name[r0]}=CY', f'{name[r2]}=M'])
    want3 = want2.copy()
    want3[r0] = NINF
    want3[r0, ix('C')], want3[r0, ix('Y')] = 0.25, 3.0
    want3[r2] = NINF
    want3[r2, ix('M')] = 0.0
    assert np.array_equal(c3.host, want3)
    d = {nm: (wild, letters) for _, nm, wild, letters in c3.describe()}
    assert list(d) == [name[r] for r in rows]
    assert d[name[r0]][1] == 'CY' and d[name[r2]][1] == 'M' and d[name[r1]][1] == ''.join(c for c in LETTERS if c not in 'CMW')
    assert d[name[r0]][0] == LETTERS[int(one['seq'][0, r0])]
    # rows of residues that are not designed stay zero
    fixed_rows = np.setdiff1d(np.arange(want.shape[0]), rows)
    assert not c3.host[fixed_rows].any()


def test_every_error_names_its_cause(one, tmp_path):
    rows = _designed(one)
    c0 = _cons(one)
    r0 = c0.names[int(rows[0])]
    f = tmp_path / 'bias.txt'

    def file_error(text, match):
        f.write_text(text)
        with pytest.raises(SystemExit, match=match):
            _cons(one, bias_file=str(f))

    file_error(f'{r0} SB 1\n', "unknown residue letter 'B'")
    file_error(f'\n{r0} S 1\n{r0} S\n', r'bias.txt:3: expected `RES\|\* LETTERS VALUE`')
    file_error(f'{r0} S high\n', "expected a number or -inf, not 'high'")
    file_error(f'{r0} S inf\n', "must be finite or -inf, not 'inf'")
    file_error(f'{r0} S nan\n', "must be finite or -inf, not 'nan'")
    file_error('S:77 S 1\n', 'S:77')                                      # not in the featurised complex
    file_error('X:3 S 1\n', "no chain 'X'")
    file_error('H:3 S 1\n', "residue 'H:3' is not designed")               # featurised, but outside the designed loop
    file_error(f'{r0} ARNDCQEGHILKMFPSTWYV -inf\n', f'residue {r0}: no allowed letter left')
    with pytest.raises(SystemExit, match="--seq_forbid: unknown residue letter 'Z'"):
        _cons(one, forbid=['C', 'Z'])
    with pytest.raises(SystemExit, match="not designed"):
        _cons(one, fix=['H:3=Y'])
    with pytest.raises(SystemExit, match='expected RES=LETTERS'):
        _cons(one, fix=[r0])
    with pytest.raises(SystemExit, match='name one residue'):
        _cons(one, fix=['*=Y'])
    with pytest.raises(SystemExit, match="unknown residue letter 'J'"):
        _cons(one, fix=[f'{r0}=J'])
    # fix keeps the file's value: a letter the file forbids at that residue stays forbidden, and nothing is left
    f.write_text(f'{r0} Y -inf\n')
    with pytest.raises(SystemExit, match=f'residue {r0}: no allowed letter left'):
        _cons(one, bias_file=str(f), fix=[f'{r0}=Y'])
    with pytest.raises(SystemExit, match='no allowed letter left'):
        _cons(one, forbid=['ARNDCQEGHILKMFPSTWYV'])


def test_check_table_refuses_what_the_kernels_do_not_handle():
    from abx_amd.constraints import SequenceConstraints, check_table
    dm = np.array([0, 1, 1, 0])
    t = np.zeros((4, 20), np.float32)
    check_table(t, dm)
    for r, v, match in ((1, np.inf, 'row 1: the sequence bias must be finite or -inf'), (2, np.nan, 'row 2: the sequence bias must be finite'),
                        (0, 1.0, 'row 0 is not designed'), (3, NINF, 'row 3 is not designed')):
        bad = t.copy()
        bad[r, 5] = v
        with pytest.raises(SystemExit, match=match):
            check_table(bad, dm)
    bad = t.copy()
    bad[2] = NINF
    with pytest.raises(SystemExit, match='H:2: no allowed letter left'):
        check_table(bad, dm, names=['H:0', 'H:1', 'H:2', 'H:3'])
    with pytest.raises(SystemExit, match='expected a'):
        check_table(t[:3], dm)
    c = SequenceConstraints.from_table(t, dm)
    assert c.allowed.all() and tuple(c.table.shape) == (4, 20)


def test_project_host_and_device_twin():
    from abx_amd.constraints import SequenceConstraints, nearest_allowed, project_host
    allowed = np.zeros((5, 20), bool)
    allowed[0, [3, 9]] = True            # 6 is equally far from both: the lower wins
    allowed[1, [19]] = True
    allowed[2, [0, 1]] = True
    allowed[3, :] = True
    allowed[4, :] = True                 # not designed
    near = nearest_allowed(allowed)
    assert near[0].tolist() == [3] * 7 + [9] * 13
    assert near[1].tolist() == [19] * 20 and near[2].tolist() == [0] + [1] * 19 and near[3].tolist() == list(range(20))
    dm = np.array([1, 1, 1, 1, 0])
    seq = np.array([[6, 0, 19, 7, 5], [7, 19, 0, 25, 25], [3, 4, 1, 0, 0]])
    got = project_host(seq, allowed, dm)
    assert got.tolist() == [[3, 19, 1, 7, 5], [9, 19, 0, 25, 25], [3, 19, 1, 0, 0]]      # allowed tokens and fixed rows stay as they are
    table = np.where(allowed, 0.0, NINF).astype(np.float32)
    table[4] = 0
    c = SequenceConstraints.from_table(table, dm)
    dev = c.project(torch.from_numpy(seq), torch.from_numpy(np.broadcast_to(dm, seq.shape).copy()))
    assert dev.dtype == torch.int64 and dev.tolist() == got.tolist()


def test_token_step_host_on_hand_made_jumps():
    from abx_amd.constraints import token_step_host
    allowed = np.ones((6, 20), bool)
    allowed[1, 10] = False               # the landing letter of the double jump below
    allowed[4, [4, 6]] = False           # row 4 starts on a forbidden letter
    allowed[5, [4, 6]] = False
    x_t = np.array([[5, 5, 2, 17, 4, 4]])
    j = np.zeros((1, 6, 20), np.float32)
    j[0, 0, 9] = 1                       # a single jump lands: 5 -> 9
    j[0, 1, 7] = 1; j[0, 1, 8] = 1       # two jumps, 5 + 2 + 3 = 10: a letter neither aimed at, forbidden here -> rejected
    j[0, 2, 0] = 2                       # 2 - 4 -> the clamp at 0
    j[0, 3, 19] = 3                      # 17 + 6 -> the clamp at 19
    j[0, 4, 6] = 1                       # from a forbidden letter onto a forbidden letter: stays
    j[0, 5, 9] = 1                       # from a forbidden letter onto an allowed one: leaves
    assert token_step_host(x_t, j, allowed).tolist() == [[9, 5, 0, 19, 4, 9]]
    assert token_step_host(x_t, j, np.ones((6, 20), bool)).tolist() == [[9, 10, 0, 19, 6, 9]]
    assert token_step_host(x_t, 0 * j, allowed).tolist() == x_t.tolist()         # no jump: the token stays, forbidden or not
    assert token_step_host(np.array([[25, -3, 2, 17, 4, 4]]), 0 * j, allowed).tolist() == [[19, 0, 2, 17, 4, 4]]
    # a row without any allowed letter keeps its token whatever the jumps say
    none = np.zeros((6, 20), bool)
    assert token_step_host(x_t, j, none).tolist() == x_t.tolist()


def test_masked_argmax_host_first_maximum_wins():
    from abx_amd.constraints import masked_argmax_host
    lg = np.zeros((2, 3, 20), np.float32)
    lg[0, 0, [4, 11]] = 2.0              # a tie: the first
    lg[0, 1, 7] = 5.0
    lg[1, 1, 7] = 5.0
    lg[1, 2, 19] = 1.0
    bias = np.zeros((3, 20), np.float32)
    assert masked_argmax_host(lg, bias).tolist() == [[4, 7, 0], [0, 7, 19]]
    bias[0, 4] = NINF
    bias[1, 7] = -5.0                    # brings letter 7 down to the others: first maximum is letter 0
    bias[2, :19] = NINF
    assert masked_argmax_host(lg, bias).tolist() == [[11, 0, 19], [0, 0, 19]]


def test_report_writer(one, tmp_path):
    from abx_amd.constraints import LETTERS
    rows = _designed(one)
    names = _cons(one).names
    r0 = int(rows[0])
    c = _cons(one, forbid=['C', 'M'], fix=[f'{names[r0]}=Y'])
    N, Lab = 5, one['anchor_flag'].shape[1]
    seq = one['seq'][0, :Lab].repeat(N, 1).clone()
    y, s, cys = LETTERS.index('Y'), LETTERS.index('S'), LETTERS.index('C')
    seq[:, rows] = s
    seq[:, r0] = y
    seq[3, int(rows[1])] = cys           # one design breaks the rule at the second residue
    path = c.write_report(str(tmp_path / 'x_sequence.tsv'), seq)
    lines = [ln.split('\t') for ln in open(path).read().splitlines()]
    assert lines[0] == ['residue', 'wild', 'allowed'] + list(LETTERS) + ['violations']
    assert len(lines) == 1 + len(rows) and all(len(ln) == 24 for ln in lines)
    assert [ln[0] for ln in lines[1:]] == [names[int(r)] for r in rows]
    first, second = lines[1], lines[2]
    assert first[1] == LETTERS[int(one['seq'][0, r0])] and first[2] == 'Y'
    assert first[3 + y] == str(N) and sum(int(v) for v in first[3:23]) == N and first[23] == '0'
    assert second[2] == ''.join(ch for ch in LETTERS if ch not in 'CM')
    assert second[3 + s] == str(N - 1) and second[3 + cys] == '1' and second[23] == '1'
    assert all(ln[23] == '0' for ln in lines[3:])


def test_options_of_the_driver_and_the_struct_field():
    from abx_amd import _lib, design
    a = design.build_parser().parse_args(['--seq_forbid', 'C', 'M', '--seq_fix', 'H:100=Y', 'H:101=ST', '--seq_bias', 'b.txt'])
    assert a.seq_forbid == ['C', 'M'] and a.seq_fix == ['H:100=Y', 'H:101=ST'] and a.seq_bias == 'b.txt'
    d = design.build_parser().parse_args([])
    assert d.seq_forbid is None and d.seq_fix is None and d.seq_bias is None
    assert _lib.AbxReverseArgs._fields_[-1][0] == 'seq_bias'             # appended at the end: earlier offsets are unchanged
    assert 'abx_seq_head_atoms_biased' in _lib.EXPORTED
