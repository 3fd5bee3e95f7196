"""GPU check of the design driver with every analysis on at once (abx_amd.analyses): the two shipped complexes complex by complex and
through the set-level schedule, whose rows carry every table - the relaxed columns included - in one gather."""
import os

import pytest

from analysis_gpu_cases import CODES, names, pdb_args, set_master_port, table_lines

pytestmark = pytest.mark.gpu

SURFACE = ('interface', 'polar', 'developability', 'shape', 'patches')      # the users of one buffer of point counts per structure set


def run_6ct7(out, flags):
    """The driver on 6ct7 with `flags` and the per-residue option of every flag that has one -> the files by name."""
    from abx_amd import analyses, design
    on = [an for an in analyses.ANALYSES if an.flag in flags]
    argv = pdb_args(CODES[:1]) + ['--num_samples', '2', '--num_t', '4', '--output_dir', str(out)]
    argv += ['--' + an.flag for an in on] + ['--' + an.extra for an in on if an.extra] + (['--ensemble_matrix'] if 'ensemble' in flags else [])
    files = design.main(argv)
    assert names(files) == sorted(os.listdir(out))
    return {os.path.basename(f): f for f in files}


@pytest.fixture(scope='module')
def all_on(tmp_path_factory):
    """One run with all twelve analyses and every _rows / _planes / _matrix option: four scorers read the point counts that the
    interface scorer fills, of the designs and of the relaxed structures."""
    from abx_amd import analyses
    return run_6ct7(tmp_path_factory.mktemp('all_on'), [an.flag for an in analyses.ANALYSES])


@pytest.mark.parametrize('flag', SURFACE)
def test_a_surface_analysis_alone_writes_the_bytes_of_the_run_with_all(all_on, tmp_path, flag):
    """Alone, a scorer of the surface runs the surface kernel itself (or, --interface, hands its counts to nobody); with all analyses on,
    one call per structure set serves the five of them: the table with its _relaxed columns and the per-residue file are the same bytes."""
    alone = run_6ct7(tmp_path, [flag, 'relax'])
    mine = [n for n in alone if n.startswith(f'{CODES[0]}_{flag}')]
    assert f'{CODES[0]}_{flag}.tsv' in mine and len(mine) == (1 if flag in ('interface', 'shape') else 2)
    for n in mine:
        assert open(alone[n], 'rb').read() == open(all_on[n], 'rb').read(), n
    relaxed = table_lines(tmp_path, CODES[0], flag)
    assert any(h.endswith('_relaxed') for h in relaxed[0]) and [r[0] for r in relaxed[1:]] == ['wild', '0', '1']


def test_all_analyses_write_the_same_tables_on_both_schedules(tmp_path, monkeypatch):
    """A sample's result does not depend on its batch mates (test_gpu_ensemble.py relies on that too), so the run with both samples
    of a complex in one batch and the set-level run of one-sample units write the same tables byte for byte."""
    from abx_amd import accuracy, analyses, confidence, design, interface, polar
    set_master_port(monkeypatch)
    codes = CODES
    common = pdb_args(codes) + ['--num_samples', '2', '--num_t', '3', '--relax_iters', '20']
    common += ['--' + an.flag for an in analyses.ANALYSES[:7]]
    one = design.main(common + ['--output_dir', str(tmp_path / 'one')])
    two = design.main(common + ['--force_collective', '--min_block', '1', '--output_dir', str(tmp_path / 'set')])
    tables = ['designs', 'relax', 'interface', 'confidence', 'accuracy', 'polar', 'ensemble']
    assert names(one) == names(two) and sorted(os.listdir(tmp_path / 'set')) == names(two)
    assert [n for n in names(two) if n.endswith('.tsv')] == sorted(f'{c}_{t}.tsv' for c in codes for t in tables)
    for n in names(two):
        if n.endswith('.tsv'):
            assert open(tmp_path / 'one' / n, 'rb').read() == open(tmp_path / 'set' / n, 'rb').read(), n
    for c in codes:
        for t, columns in (('interface', interface.INTERFACE_COLUMNS), ('confidence', confidence.CONFIDENCE_COLUMNS),
                           ('accuracy', accuracy.ACCURACY_COLUMNS), ('polar', polar.POLAR_COLUMNS)):
            lines = table_lines(tmp_path / 'set', c, t)
            relaxed = [lines[0].index(h + '_relaxed') for h in columns]
            assert len(lines) == 2 + 2 and all(len(r) == len(lines[0]) for r in lines) and [r[0] for r in lines[1:]] == ['wild', '0', '1'], (c, t)
            assert all(lines[1][k] == 'nan' for k in relaxed) and all(any(r[k] != 'nan' for k in relaxed) for r in lines[2:]), (c, t)
