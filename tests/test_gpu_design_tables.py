"""GPU check of the design driver with every analysis on at once (abx_amd.analyses): the two shipped complexes complex by complex and
through the set-level schedule, whose rows carry every table - the relaxed columns included - in one gather."""
import os

import pytest

from analysis_gpu_cases import CODES, names, pdb_args, set_master_port, table_lines

pytestmark = pytest.mark.gpu


def test_all_analyses_write_the_same_tables_on_both_schedules(tmp_path, monkeypatch):
    """A sample's result does not depend on its batch mates (test_gpu_ensemble.py relies on that too), so the run with both samples
    of a complex in one batch and the set-level run of one-sample units write the same tables byte for byte."""
    from abx_amd import accuracy, analyses, confidence, design, interface, polar
    set_master_port(monkeypatch)
    codes = CODES
    common = pdb_args(codes) + ['--num_samples', '2', '--num_t', '3', '--relax_iters', '20']
    common += ['--' + an.flag for an in analyses.ANALYSES]
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
