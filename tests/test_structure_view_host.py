"""CPU-only check of the structure conventions of the per-design analyses: abx_amd/csrc/structure_dev.h compiled with g++ against the
stand-in headers of tests/relax_emu into a stand-alone program that reads a 3-row toy structure through StructureView."""
import os
import subprocess

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))

PROGRAM = r'''
#include "common.h"
#include "abx_hip.h"
#include "structure_dev.h"

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { printf("line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

int main() {
    // L = 3 rows, the first two predicted (Lab = Lpred = 2), two structures in the batch
    static float pred[2][2][14][3], gt[3][14][3], radius[21][14];
    long long pseq[2][2] = {{-5, 37}, {0, 20}}, gseq[3] = {1, 2, 3};
    unsigned char pmask[2][3][14], gexists[3][14], rmask[3] = {1, 0, 1};
    memset(pmask, 1, sizeof(pmask));
    memset(gexists, 1, sizeof(gexists));
    pmask[0][0][3] = 0;                        // structure 0: slot 3 of row 0 is absent in pred_mask
    gexists[2][5] = 0;                         // slot 5 of the ground-truth row is absent in gt_exists
    radius[20][0] = 1.7f;                      // the unknown type has slot 0 only
    radius[3][4] = radius[3][5] = 1.7f;
    AbxInterfaceArgs a;
    memset(&a, 0, sizeof(a));
    a.pred_atom14 = &pred[0][0][0][0]; a.pred_sb = 2 * 42; a.Lpred = 2;
    a.pred_seq = &pseq[0][0]; a.pred_seq_sb = 2;
    a.gt_atom14 = &gt[0][0][0]; a.gt_exists = &gexists[0][0]; a.gt_seq = gseq;
    a.radius = &radius[0][0];
    a.B = 2; a.L = 3; a.Lab = 2;
    using View = StructureView<AbxInterfaceArgs>;
    {
        const View s(a, 0);
        EXPECT(s.aatype(0) == 20);             // a negative token
        EXPECT(s.aatype(1) == 20);             // a token above 20
        EXPECT(s.aatype(2) == 3);              // rows >= Lab: the ground truth's token
        EXPECT(View::clamp_aa(20) == 20 && View::clamp_aa(21) == 20 && View::clamp_aa(-1) == 20 && View::clamp_aa(0) == 0);
        EXPECT(s.xyz(0, 1) == &pred[0][0][1][0] && s.xyz(1, 13) == &pred[0][1][13][0]);
        EXPECT(s.xyz(2, 4) == &gt[2][4][0]);   // rows >= Lpred: the ground truth's coordinates
        EXPECT(View(a, 1).xyz(1, 2) == &pred[1][1][2][0] && View(a, 1).aatype(0) == 0 && View(a, 1).aatype(1) == 20);
        // no res_mask, no pred_mask: the radius table for a predicted row (whatever gt_exists says), gt_exists for the others
        EXPECT(s.kept(0) && s.kept(1) && s.kept(2));
        EXPECT(s.exists(0, 0, 20) && !s.exists(0, 1, 20));
        EXPECT(s.exists(2, 4, 3) && !s.exists(2, 5, 3));
    }
    a.pred_mask = &pmask[0][0][0];
    {
        // pred_mask decides when it is given, for every row, before the radius table and gt_exists
        const View s(a, 0);
        EXPECT(!s.exists(0, 3, 20) && s.exists(0, 2, 20) && s.exists(0, 1, 20));
        EXPECT(s.exists(2, 5, 3));
        EXPECT(View(a, 1).exists(0, 3, 0));    // (the mask of the second structure)
    }
    a.res_mask = rmask;
    {
        // res_mask removes a row before anything else is asked
        const View s(a, 0);
        EXPECT(s.kept(0) && !s.kept(1) && s.kept(2));
        for (int slot = 0; slot < 14; ++slot) EXPECT(!s.exists(1, slot, 20));
        EXPECT(s.exists(0, 2, 20) && !s.exists(0, 3, 20) && s.exists(2, 4, 3));
        EXPECT(s.aatype(1) == 20 && s.xyz(1, 0) == &pred[0][1][0][0]);
    }
    a.pred_mask = nullptr;
    EXPECT(!View(a, 0).exists(1, 0, 20) && View(a, 0).exists(0, 0, 20) && !View(a, 0).exists(2, 5, 3));
    printf("%d failures\n", failures);
    return failures != 0;
}
'''


def test_structure_view_conventions_on_a_toy_structure(tmp_path):
    """Token clamp (negative, above 20), the source of xyz (prediction below Lpred, ground truth beyond), and the order of existence:
    res_mask, then pred_mask, then the radius table (predicted rows) or gt_exists - against literal expectations."""
    emu = os.path.join(ROOT, 'tests', 'relax_emu')
    src, exe = tmp_path / 'view.cpp', tmp_path / 'view'
    src.write_text(PROGRAM)
    subprocess.check_call(['g++', '-std=c++20', '-O1', '-w', '-I' + emu, '-I' + os.path.join(ROOT, 'abx_amd', 'csrc'),
                           '-I' + os.path.join(ROOT, 'include'), str(src), '-o', str(exe), '-lpthread'])
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout == '0 failures\n', run.stdout + run.stderr
