"""CPU-only check of the residue rules that developability.hip and patches.hip share: abx_amd/csrc/residue_rules.h compiled with g++
against the stand-in headers of tests/relax_emu into a stand-alone program, its answers against the Python side of the two analyses."""
import os
import subprocess

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))

PROGRAM = r'''
#include "common.h"
#include "residue_rules.h"

int main() {
    for (int c = 0; c < 14; ++c) printf("cdr %d %d\n", c, is_cdr(c) ? 1 : 0);
    for (int aa = 0; aa < 21; ++aa) printf("charge %d %d\n", aa, type_charge(aa));
    printf("one %.17g\n", FIXED_ONE);
    double rel, ref, exposed;
    while (scanf("%lf %lf %lf", &rel, &ref, &exposed) == 3) printf("exposed %d\n", row_exposed(rel, ref, exposed) ? 1 : 0);
    return 0;
}
'''


def test_residue_rules_agree_with_the_python_side(tmp_path):
    """is_cdr for the 14 values of cdr_def against developability.CDR_CODES; type_charge for the 21 types against the unit charges of
    developability_host (Lys / Arg +1, Asp / Glu -1) and the sign of patches.charge_table's full charges; FIXED_ONE; row_exposed at rel
    just below, at and just above exposed * ref, and at ref = 0, against the comparison of the host twins."""
    from abx_amd import developability, patches, residue_constants as rc
    emu = os.path.join(ROOT, 'tests', 'relax_emu')
    src, exe = tmp_path / 'rules.cpp', tmp_path / 'rules'
    src.write_text(PROGRAM)
    subprocess.check_call(['g++', '-std=c++20', '-O1', '-w', '-I' + emu, '-I' + os.path.join(ROOT, 'abx_amd', 'csrc'), str(src), '-o', str(exe)])
    cases = []
    for ref, exposed in ((113.7, 0.075), (1.0, 1.0), (87.25, 0.3), (0.0, 0.075)):
        at = exposed * ref
        cases += [(np.nextafter(at, -np.inf), ref, exposed), (at, ref, exposed), (np.nextafter(at, np.inf), ref, exposed)]
    cases += [(0.0, 50.0, 0.0), (5.0, 0.0, 0.0)]
    stdin = ''.join('%r %r %r\n' % (float(a), float(b), float(c)) for a, b, c in cases)
    run = subprocess.run([str(exe)], input=stdin, capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    lines = [l.split() for l in run.stdout.splitlines()]
    cdr = {int(l[1]): int(l[2]) for l in lines if l[0] == 'cdr'}
    assert cdr == {c: int(c in developability.CDR_CODES) for c in range(14)}
    charge = {int(l[1]): int(l[2]) for l in lines if l[0] == 'charge'}
    unit = {'K': 1, 'R': 1, 'D': -1, 'E': -1}
    types = list(rc.restypes) + ['X']
    assert len(types) == 21 and charge == {i: unit.get(t, 0) for i, t in enumerate(types)}
    q10 = patches.charge_table()
    assert all(charge[i] == (int(q10[i]) // 10 if abs(int(q10[i])) == 10 else 0) for i in range(21))
    assert [float(l[1]) for l in lines if l[0] == 'one'] == [float(developability.FIXED_ONE)] == [2.0 ** 30]
    got = [int(l[1]) for l in lines if l[0] == 'exposed']
    want = [int(ref > 0 and rel >= float(exposed) * ref) for rel, ref, exposed in cases]      # developability_host's is_exposed
    assert got == want and len(got) == len(cases)
    assert want[:3] == [0, 1, 1] and want[9:12] == [0, 0, 0] and want[12:] == [1, 0]
