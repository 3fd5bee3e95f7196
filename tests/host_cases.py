"""What the host tests of the per-design analyses share (test_{design_scores,relax,interface,ensemble,accuracy,polar}_host.py): the
library for the argument checks that need no GPU, and the C layout of a descriptor as gcc sees include/abx_hip.h."""
import ctypes
import os
import subprocess
import tempfile

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
HEADER = os.path.join(ROOT, 'include', 'abx_hip.h')


def load_lib():
    """libabx_hip.so bound by ctypes, built first when it is missing."""
    import __graft_entry__ as ge
    from abx_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        ge.build()
    return _lib.load()


def assert_c_layout(structs, macros):
    """structs {C name: ctypes.Structure}: asserts sizeof and the offsetof of every field against a C program compiled from the header.
    -> {macro: its integer value in the header} for the caller to compare with the Python side."""
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', 'int main(){']
    lines += [f'printf("{m} %d\\n", {m});' for m in macros]
    for name, st in structs.items():
        lines.append(f'printf("{name}.size %zu\\n", sizeof({name}));')
        for f, _ in st._fields_:
            lines.append(f'printf("{name}.{f} %zu\\n", offsetof({name}, {f}));')
    lines.append('return 0;}')
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, 'l.c'), os.path.join(d, 'l')
        open(src, 'w').write('\n'.join(lines))
        subprocess.check_call(['gcc', src, '-o', exe])
        c_layout = dict(l.split() for l in subprocess.check_output([exe]).decode().split('\n') if l)
    for name, st in structs.items():
        assert int(c_layout[name + '.size']) == ctypes.sizeof(st), name
        for f, _ in st._fields_:
            assert int(c_layout[f'{name}.{f}']) == getattr(st, f).offset, (name, f)
    return {m: int(c_layout[m]) for m in macros}
