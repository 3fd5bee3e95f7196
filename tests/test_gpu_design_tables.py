"""GPU check of the design driver with every analysis on at once (abx_amd.analyses): the two shipped complexes complex by complex and
through the set-level schedule, whose rows carry every table - the relaxed columns included - in one gather."""
import os

import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu


def test_all_analyses_write_the_same_tables_on_both_schedules(tmp_path, monkeypatch):
    """A sample's result does not depend on its batch mates (test_gpu_ensemble.py relies on that too), so the run with both samples
    of a complex in one batch and the set-level run of one-sample units write the same tables byte for byte."""
    from abx_amd import accuracy, analyses, confidence, design, interface, polar
    monkeypatch.setenv('MASTER_PORT', '29569')
    codes = ['6ct7_H_L_S', '6qd7_X_Z_F|E']
    common = ['--pdb_file'] + [os.path.join(GOLDEN, 'pdb', c + '.pdb') for c in codes] + ['--num_samples', '2', '--num_t', '3', '--relax_iters', '20']
    common += ['--' + an.flag for an in analyses.ANALYSES]
    one = design.main(common + ['--output_dir', str(tmp_path / 'one')])
    two = design.main(common + ['--force_collective', '--min_block', '1', '--output_dir', str(tmp_path / 'set')])
    names = lambda fs: sorted(os.path.basename(f) for f in fs)
    tables = ['designs', 'relax', 'interface', 'confidence', 'accuracy', 'polar', 'ensemble']
    assert names(one) == names(two) and sorted(os.listdir(tmp_path / 'set')) == names(two)
    assert [n for n in names(two) if n.endswith('.tsv')] == sorted(f'{c}_{t}.tsv' for c in codes for t in tables)
    for n in names(two):
        if n.endswith('.tsv'):
            assert open(tmp_path / 'one' / n, 'rb').read() == open(tmp_path / 'set' / n, 'rb').read(), n
    for c in codes:
        for t, columns in (('interface', interface.INTERFACE_COLUMNS), ('confidence', confidence.CONFIDENCE_COLUMNS),
                           ('accuracy', accuracy.ACCURACY_COLUMNS), ('polar', polar.POLAR_COLUMNS)):
            lines = [ln.split('\t') for ln in open(tmp_path / 'set' / f'{c}_{t}.tsv').read().splitlines()]
            relaxed = [lines[0].index(h + '_relaxed') for h in columns]
            assert len(lines) == 2 + 2 and all(len(r) == len(lines[0]) for r in lines) and [r[0] for r in lines[1:]] == ['wild', '0', '1'], (c, t)
            assert all(lines[1][k] == 'nan' for k in relaxed) and all(any(r[k] != 'nan' for k in relaxed) for r in lines[2:]), (c, t)
