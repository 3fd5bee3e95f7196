"""End-to-end driver in the shape of the reference's design.py / inference.py main (design.py:277-375, inference.py:59-82,
275-392): build the diffuser and the score network, featurise each complex, run the reverse diffusion for `num_samples` samples
and write the PDB files (per step in trajectory mode, asynchronously).

    python -m abx_amd.design --pdb_file 6ct7_H_L_S.pdb --num_samples 100 --mode design --output_dir out/      (raw PDB, 8f-1)
    python -m abx_amd.design --workload L256 --num_samples 4 --mode trajectory --num_t 10 --output_dir out/   (synthetic complex)
    python -m abx_amd.design --pdb_file 6ct7_H_L_S.pdb --mode optimize --optimize_steps 10 --guidance --num_samples 100     (config 4)
    python -m abx_amd.design --pdb_file 6ct7_H_L_S.pdb --num_samples 100 --score --output_dir out/     (+ per-CDR RMSD / AAR, violation and clash counts)
    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 -m abx_amd.design \
        --pdb_list diffab_test.txt --pdb_dir pdbs/ --num_samples 100 --output_dir out/                        (a test set on 8 GPUs)

    python -m abx_amd.design --name_idx diffab_test.idx --data_dir npz/ --model_features config_data_feature.json \
        --model abx_diffab.ckpt --model_config config_model.json --gpu_list 0 1 2 3 4 5 6 7 --num_samples 100 --output_dir out/
                                                                     (inference.py's own command line: BASELINE configs 3 / 4)

--name_idx / --data_dir / --model_features / --gpu_list / --batch_size are the arguments of the reference's inference.py
(inference.py:398-416): one complex name per line, <data_dir>/<name>.npz in the `make_pdb_npz` schema (abx_amd.data.antibody.
load_complex_npz), the feature-pipeline JSON (its make_diffuser_features entry supplies generate_area and, in optimize mode, the
list of optimize_steps that is looped over like inference.py:310-345), and the output layout of inference.py:
<output_dir>/<mode>[/OPT-<step>]/reference/<name>.pdb (the ground truth) and .../<k:04d>/<name>.pdb for sample k.  --gpu_list with
more than one entry starts one rank per listed GPU through torch.distributed.run (the reference spawns one worker per GPU that all
repeat the same work, inference.py:376-381; here the samples are sharded).  --batch_size (complexes per DataLoader batch upstream) is
accepted and ignored: complexes run one after the other with all local samples of a complex in one batch.
--pdb_file follows the reference's naming contract <code>_<heavy>_<light>_<antigen chains joined by |>.pdb (dataset.py:290-293);
it is read by abx_amd.data.antibody (plain-text parser, landmark IMGT locator, 16 A antigen patch, 32-residue window).
Several files (or --pdb_list, one name per line, relative to --pdb_dir) are processed one after the other.
Multi-GPU (one process per GPU under torch.distributed.run): the SAMPLES of every complex are sharded over the ranks
(sampler.shard_sample_ids: contiguous blocks; per-sample noise keys, so a sample's trajectory does not depend on where it runs),
every rank writes the PDB files of its own samples, and the designed sequences / pLDDT are gathered with one RCCL all_gather per
field (sampler.gather_results) for `<output_dir>/<complex>_designs.tsv`, written by rank 0.
--score: every design is scored on the GPU as its record is made (abx_amd.metrics.DesignScorer, one launch pair per record, no host
synchronisation); the scores travel as one more field of the same gathers and become the columns metrics.SCORE_COLUMNS of the TSV.
--relax: every design is relaxed on the GPU after the last step (abx_amd.relax.ViolationRelaxer, abx_relax: one launch per batch): the
violation energy of the designed residues (+ --relax_flank linked neighbours on each side) is minimised over rigid-body motions and chi
angles of those residues; <name>_relaxed.pdb is written beside every design (upstream's naming, which its eval_metric.py skips) and
<output_dir>/<complex>_relax.tsv holds one line per sample: relax.RELAX_COLUMNS and, with --score, the scores of the relaxed structure.
The design files and <complex>_designs.tsv are what they are without --relax.
--interface: every design gets its interface row on the GPU after the last step (abx_amd.interface.InterfaceScorer, abx_interface_scores):
solvent-accessible surface buried between the antibody and the featurised antigen (a cropped patch when the complex was cropped),
interface residues and heavy-atom contacts, with the designed residues as the region.  <output_dir>/<complex>_interface.tsv holds a
`wild` line (the input complex itself) and one line per sample: interface.INTERFACE_COLUMNS, then delta_<column> = design minus wild
type for interface.DELTA_COLUMNS (the geometric analogue of upstream's ddG) and, with --relax, the columns of the relaxed structure
suffixed _relaxed (nan on the wild line).  No other output file changes.
--ensemble: the N designs of a complex are compared with each other on the GPU (abx_amd.ensemble.EnsembleAnalyzer, abx_ensemble_pairs +
abx_ensemble_cluster) by the rank that writes the tables, after the gather: the backbone of the designed antibody travels with the other
fields.  <output_dir>/<complex>_ensemble.tsv holds an `all` line (clusters, unique sequences, mean pairwise RMSD and sequence identity)
and one line per sample: ensemble.ENSEMBLE_COLUMNS and `representative`, the sample id of the centre of the sample's cluster - the few
files worth the expensive evaluation.  --ensemble_matrix also writes <complex>_ensemble_rmsd.npy, the (3, N, N) planes rmsd_fit,
rmsd_frame, seq_diff.  With --relax the analysis still describes the designs as written.  No other output file changes.
--confidence: every design gets its confidence row on the GPU right after the last network call (abx_amd.confidence.DistogramScorer,
abx_distogram_scores): the checkpoint's distogram head on the pair representation of that call - the network's own distribution over
every pseudo-beta distance - against the structure it emitted.  <output_dir>/<complex>_confidence.tsv holds a `wild` line (the input
complex's own coordinates against the same predictions, the mean over the designs), one line per sample: confidence.CONFIDENCE_COLUMNS,
then delta_<column> = design minus the wild type under the SAME design's prediction for confidence.DELTA_COLUMNS and, with --relax, the
columns of the relaxed structure suffixed _relaxed (nan on the wild line).  --confidence_planes also writes
<complex>_confidence_contacts.npy, the mean predicted contact probability over the designs, (L, L) (sample-sharded runs only: the planes
of a set-level schedule would travel as 8 L^2 bytes per sample).  No other output file changes.
--accuracy: every design is compared with the input crystal structure on the GPU after the last step (abx_amd.accuracy.AccuracyScorer,
abx_accuracy_scores): all-atom / backbone / C-alpha lDDT (the quantity pLDDT predicts) with the designed residues as the region, the
calibration of the per-residue pLDDT of the last network call, TM-score / GDT-TS / GDT-HA / RMSD of the C-alpha (upstream's TMscoreHead)
and the native antibody-antigen residue contacts that survive (DockQ's Fnat).  <output_dir>/<complex>_accuracy.tsv holds a `wild` line
(the input complex against itself: every lDDT and fnat 1, rmsd_ca 0) and one line per sample: accuracy.ACCURACY_COLUMNS and, with
--relax, the columns of the relaxed structure suffixed _relaxed (nan on the wild line), then delta_<column> = relaxed minus design for
accuracy.DELTA_COLUMNS.  --accuracy_rows also writes <complex>_accuracy_rows.npy, the per-residue lDDT (N, L, 4: accuracy.ROW_COLUMNS;
sample-sharded runs only).  No other output file changes.
--polar: every design gets its polar row on the GPU after the last step (abx_amd.polar.PolarScorer, abx_polar_scores): heavy-atom hydrogen
bonds and salt bridges between the antibody and the featurised antigen, the hydrogen bonds that hold the designed loop, and the polar
atoms that binding buries without a partner (from the point counts of the interface analysis; with --interface the surface kernel runs
once for both tables).  <output_dir>/<complex>_polar.tsv holds a `wild` line (the input complex itself) and one line per sample:
polar.POLAR_COLUMNS, then delta_<column> = design minus wild type for polar.DELTA_COLUMNS and, with --relax, the columns of the relaxed
structure suffixed _relaxed (nan on the wild line).  --polar_rows also writes <complex>_polar_rows.npy, (N, L, 4) int16 per residue:
cross-side and same-side hydrogen bonds, salt bridges, unsatisfied atoms (polar.ROW_COLUMNS; sample-sharded runs only).  No other output
file changes.
Weights: a checkpoint with the reference's `model_state_dict`, or seeded random weights (no checkpoint ships with the reference)."""
import argparse
import os
from collections import OrderedDict

import torch

from . import features, sampler, synthetic
from .config import default_config, load_config
from .diffuser.full_diffuser import FullDiffuser
from .io import TrajectoryWriter, index_to_str_seq
from .model.abx import ScoreNetwork


def complex_list(pdb_files, pdb_list, pdb_dir):
    """The complexes of a run, in order: --pdb_file entries, then the lines of --pdb_list (blank lines and # comments skipped;
    '.pdb' appended when missing), both relative to --pdb_dir when given."""
    names = list(pdb_files or [])
    if pdb_list:
        with open(pdb_list) as f:
            for line in f:
                line = line.split('#')[0].strip()
                if line:
                    names.append(line if line.endswith('.pdb') else line + '.pdb')
    return [os.path.join(pdb_dir, n) if pdb_dir and not os.path.isabs(n) else n for n in names]


def sample_names(name, ids, num_samples):
    """Output stem of every sample: the complex name for a single sample, <code>-<sample id>_<chains> otherwise (global ids)."""
    if num_samples == 1:
        return [name for _ in ids]
    head, tail = name.split('_')[0], '_'.join(name.split('_')[1:])
    return [f'{head}-{i:03d}_{tail}' for i in ids]


TIMINGS = []      # one dict per complex of the last main() call: seconds spent reading / featurising, sampling, waiting for the writer


def read_model_features(path):
    """The make_diffuser_features entry of a feature-pipeline JSON (config/config_data_feature.json): (generate_area, optimize_steps)."""
    import json
    with open(path, encoding='utf-8') as f:
        feats = json.load(f)
    for name, opts in feats:
        if 'diffuse' in name:
            return opts.get('generate_area', 'H3'), list(opts.get('optimize_steps', []))
    return 'H3', []


def _write_designs(out_dir, cname, rows):
    """<out_dir>/<complex>_designs.tsv: (sample id, mean pLDDT, designed antibody sequence) per sample; with --score a row carries
    a fourth entry, its metrics.SCORE_COLUMNS values, written as further columns."""
    tsv = os.path.join(out_dir, f'{cname}_designs.tsv')
    scored = bool(rows) and len(rows[0]) > 3
    with open(tsv, 'w') as f:
        if scored:
            from .metrics import SCORE_COLUMNS, format_scores
            f.write('sample\tmean_pLDDT\tantibody_sequence\t' + '\t'.join(SCORE_COLUMNS) + '\n')
            for i, pl, toks, sc in rows:
                f.write(f'{i}\t{pl:.3f}\t{index_to_str_seq(toks)}\t' + '\t'.join(format_scores(sc)) + '\n')
        else:
            f.write('sample\tmean_pLDDT\tantibody_sequence\n')
            for i, pl, toks in rows:
                f.write(f'{i}\t{pl:.3f}\t{index_to_str_seq(toks)}\n')
    return tsv


def _write_trajectory_scores(out_dir, cname, table):
    """<out_dir>/<complex>_trajectory_scores.tsv: one line per (sample, record of the trajectory).  table (samples, records, 1 + columns):
    t of the record, then its metrics.SCORE_COLUMNS values."""
    from .metrics import SCORE_COLUMNS, format_scores
    tsv = os.path.join(out_dir, f'{cname}_trajectory_scores.tsv')
    with open(tsv, 'w') as f:
        f.write('sample\tstep\tt\t' + '\t'.join(SCORE_COLUMNS) + '\n')
        for i, recs in enumerate(table.tolist()):
            for k, r in enumerate(recs):
                f.write(f'{i}\t{k}\t{r[0]:.4f}\t' + '\t'.join(format_scores(r[1:])) + '\n')
    return tsv


def _write_relax(out_dir, cname, rows, scored):
    """<out_dir>/<complex>_relax.tsv: (sample id, values) per sample; values = the relax.RELAX_COLUMNS report and, when scored, the
    metrics.SCORE_COLUMNS of the relaxed structure."""
    from .relax import RELAX_COLUMNS, format_report
    from .metrics import SCORE_COLUMNS, format_scores
    NR = len(RELAX_COLUMNS)
    tsv = os.path.join(out_dir, f'{cname}_relax.tsv')
    with open(tsv, 'w') as f:
        f.write('sample\t' + '\t'.join(RELAX_COLUMNS + (SCORE_COLUMNS if scored else ())) + '\n')
        for i, v in rows:
            f.write(f'{i}\t' + '\t'.join(format_report(v[:NR]) + (format_scores(v[NR:]) if scored else [])) + '\n')
    return tsv


def _write_with_wild_deltas(kind, out_dir, cname, wild, rows, relaxed):
    """<out_dir>/<complex>_<kind>.tsv of the analysis module abx_amd.<kind> (interface, polar): the `wild` line, then (sample id, values)
    per sample; values = the module's <KIND>_COLUMNS row and, when relaxed, the row of the relaxed structure.  After the columns:
    delta_<column> = row minus wild for the module's DELTA_COLUMNS."""
    import importlib
    mod = importlib.import_module(f'.{kind}', __package__)
    columns, fmt = getattr(mod, f'{kind.upper()}_COLUMNS'), getattr(mod, f'format_{kind}')
    N = len(columns)
    tsv = os.path.join(out_dir, f'{cname}_{kind}.tsv')
    with open(tsv, 'w') as f:
        f.write('sample\t' + '\t'.join(columns + tuple('delta_' + c for c in mod.DELTA_COLUMNS) +
                                       (tuple(c + '_relaxed' for c in columns) if relaxed else ())) + '\n')
        f.write('wild\t' + '\t'.join(fmt(wild) + mod.format_delta(wild, wild) + (['nan'] * N if relaxed else [])) + '\n')
        for i, v in rows:
            f.write(f'{i}\t' + '\t'.join(fmt(v[:N]) + mod.format_delta(v[:N], wild) + (fmt(v[N:2 * N]) if relaxed else [])) + '\n')
    return tsv


def _write_interface(out_dir, cname, wild, rows, relaxed):
    return _write_with_wild_deltas('interface', out_dir, cname, wild, rows, relaxed)


def _write_polar(out_dir, cname, wild, rows, relaxed):
    return _write_with_wild_deltas('polar', out_dir, cname, wild, rows, relaxed)


def _write_accuracy(out_dir, cname, wild, rows, relaxed):
    """<out_dir>/<complex>_accuracy.tsv: the `wild` line, then (sample id, values) per sample; values = the accuracy.ACCURACY_COLUMNS row
    and, when relaxed, the row of the relaxed structure followed by delta_<column> = relaxed minus design for accuracy.DELTA_COLUMNS."""
    from .accuracy import ACCURACY_COLUMNS, DELTA_COLUMNS, format_accuracy, format_delta
    NA = len(ACCURACY_COLUMNS)
    tsv = os.path.join(out_dir, f'{cname}_accuracy.tsv')
    with open(tsv, 'w') as f:
        f.write('sample\t' + '\t'.join(ACCURACY_COLUMNS + ((tuple(c + '_relaxed' for c in ACCURACY_COLUMNS) +
                                                             tuple('delta_' + c for c in DELTA_COLUMNS)) if relaxed else ())) + '\n')
        f.write('wild\t' + '\t'.join(format_accuracy(wild) + (['nan'] * (NA + len(DELTA_COLUMNS)) if relaxed else [])) + '\n')
        for i, v in rows:
            f.write(f'{i}\t' + '\t'.join(format_accuracy(v[:NA]) +
                                          ((format_accuracy(v[NA:2 * NA]) + format_delta(v[NA:2 * NA], v[:NA])) if relaxed else [])) + '\n')
    return tsv


def _write_confidence(out_dir, cname, rows, relaxed):
    """<out_dir>/<complex>_confidence.tsv: the `wild` line, then (sample id, values) per sample; values = the confidence.CONFIDENCE_COLUMNS
    row, when relaxed the row of the relaxed structure, and last the sample's own wild row (the input complex's coordinates against the
    sample's prediction).  wild line: the mean of the wild rows.  After the columns: delta_<column> = row minus the sample's wild row."""
    from .confidence import CONFIDENCE_COLUMNS, DELTA_COLUMNS, format_confidence, format_delta
    NC = len(CONFIDENCE_COLUMNS)
    tsv = os.path.join(out_dir, f'{cname}_confidence.tsv')
    wilds = [v[len(v) - NC:] for _, v in rows]
    wild = [sum(w[k] for w in wilds) / max(len(wilds), 1) for k in range(NC)]
    with open(tsv, 'w') as f:
        f.write('sample\t' + '\t'.join(CONFIDENCE_COLUMNS + tuple('delta_' + c for c in DELTA_COLUMNS) +
                                       (tuple(c + '_relaxed' for c in CONFIDENCE_COLUMNS) if relaxed else ())) + '\n')
        f.write('wild\t' + '\t'.join(format_confidence(wild) + format_delta(wild, wild) + (['nan'] * NC if relaxed else [])) + '\n')
        for (i, v), w in zip(rows, wilds):
            f.write(f'{i}\t' + '\t'.join(format_confidence(v[:NC]) + format_delta(v[:NC], w) +
                                          (format_confidence(v[NC:2 * NC]) if relaxed else [])) + '\n')
    return tsv


def _write_ensemble(out_dir, cname, summ, rows, centres):
    """<out_dir>/<complex>_ensemble.tsv: the `all` line, then (sample id, ensemble.ENSEMBLE_COLUMNS values) per sample in row order.
    summ: ensemble.summary of the table; centres: the rows' positions of the cluster centres in order of discovery.  Columns: the row,
    `representative` (sample id of the centre of the row's cluster), then the summary's own columns prefixed all_ (nan on sample
    lines); the three means of the summary stand in their ENSEMBLE_COLUMNS on the `all` line."""
    from .ensemble import ENSEMBLE_COLUMNS, format_ensemble, format_summary
    own = [c for c in summ if c not in ENSEMBLE_COLUMNS]
    fs = dict(zip(summ, format_summary(summ)))
    tsv = os.path.join(out_dir, f'{cname}_ensemble.tsv')
    with open(tsv, 'w') as f:
        f.write('sample\t' + '\t'.join(ENSEMBLE_COLUMNS + ('representative',) + tuple('all_' + c for c in own)) + '\n')
        f.write('all\t' + '\t'.join([fs.get(c, 'nan') for c in ENSEMBLE_COLUMNS] + ['nan'] + [fs[c] for c in own]) + '\n')
        for i, v in rows:
            f.write(f'{i}\t' + '\t'.join(format_ensemble(v) + [str(rows[centres[int(v[0])]][0])] + ['nan'] * len(own)) + '\n')
    return tsv


def _relaunch_on_gpus(gpu_list, argv):
    """--gpu_list a b c ... outside torch.distributed.run: one rank per listed GPU on 127.0.0.1."""
    import socket
    import subprocess
    import sys
    with socket.socket() as sk:
        sk.bind(('127.0.0.1', 0))
        port = sk.getsockname()[1]
    env = dict(os.environ, CUDA_VISIBLE_DEVICES=','.join(str(g) for g in gpu_list), HSA_ENABLE_IPC_MODE_LEGACY='0')
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', f'--nproc-per-node={len(gpu_list)}', '--master-addr', '127.0.0.1',
           '--master-port', str(port), '-m', 'abx_amd.design'] + list(argv)
    return subprocess.call(cmd, env=env)


def build_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument('--pdb_file', nargs='*', default=None, help='antibody-antigen complex(es), <code>_<H>_<L>_<antigen chains>.pdb')
    ap.add_argument('--pdb_list', default=None, help='text file with one complex name per line (a test-set index)')
    ap.add_argument('--pdb_dir', default=None, help='directory the names of --pdb_file / --pdb_list are relative to')
    ap.add_argument('--workload', default='L256', choices=sorted(synthetic.WORKLOADS), help='synthetic complex when no PDB is given')
    ap.add_argument('--num_samples', type=int, default=4)
    ap.add_argument('--mode', default='design', choices=['design', 'trajectory', 'optimize'])
    ap.add_argument('--optimize_steps', type=int, default=10, help='optimize mode: start the reverse process at t = steps / 100')
    ap.add_argument('--num_t', type=int, default=100)
    ap.add_argument('--generate_area', default='H3')
    ap.add_argument('--model_config', default=None, help='the reference config/config_model.json (default: built-in copy)')
    ap.add_argument('--ckpt', '--model', dest='ckpt', default=None, help='checkpoint with model_state_dict (default: seeded random weights)')
    ap.add_argument('--output_dir', default='design_out')
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--device', default=None, help='default: cuda:<LOCAL_RANK>')
    ap.add_argument('--guidance', action='store_true', help='structural-violation guidance (clash + C-N bond terms, abx_clash_grad) on')
    ap.add_argument('--guidance_scale', type=float, nargs=2, default=[1.0, 1.0], metavar=('TRANS', 'ROT'),
                    help='step scales of the guidance gradients on the translation / rotation scores')
    ap.add_argument('--debug_one_gpu', action='store_true', help='debugging on a 1-GPU box: every rank uses cuda:0 and the gloo backend')
    # the reference's inference.py arguments (inference.py:398-416)
    ap.add_argument('--name_idx', default=None, help='text file with one complex name per line (entries of --data_dir)')
    ap.add_argument('--data_dir', default=None, help='directory of <name>.npz files in the make_pdb_npz schema')
    ap.add_argument('--model_features', default=None, help='feature-pipeline JSON (config/config_data_feature.json): generate_area, optimize_steps')
    ap.add_argument('--gpu_list', type=int, nargs='+', default=None, help='GPUs to use, one rank each (default: the launcher\'s ranks / GPU 0)')
    ap.add_argument('--batch_size', type=int, default=1, help='accepted for compatibility (complexes per batch upstream); ignored')
    ap.add_argument('--verbose', action='store_true')
    ap.add_argument('--min_block', type=int, default=50, help='set-level schedule: samples per work unit (a complex is split into '
                    'num_samples // min_block blocks)')
    ap.add_argument('--shard_samples', action='store_true', help='several complexes on several ranks: shard the samples of EVERY complex over '
                    'the ranks (one gather per complex) instead of dealing (complex, sample block) units to the ranks')
    ap.add_argument('--force_collective', action='store_true', help='single rank: still initialise RCCL and run the final gather through a '
                    '1-rank all_gather (exercises the collective path on a 1-GPU box; same results)')
    ap.add_argument('--exact_gemm', action='store_true', help='exact fp32-MFMA kernels instead of the split-f16 ones (slower; the remedy when '
                    'the sampler reports non-finite frames: an activation beyond the split kernels\' range)')
    ap.add_argument('--score', action='store_true', help='score every design on the GPU (abx_design_scores): per-CDR RMSD / AAR against the '
                    'input structure, peptide-violation and clash counts as further columns of <complex>_designs.tsv; in trajectory mode also '
                    '<complex>_trajectory_scores.tsv with one line per sample and step')
    ap.add_argument('--relax', action='store_true', help='relax every design on the GPU (abx_relax): rigid-body + chi minimisation of the '
                    'violation energy of the designed residues; writes <name>_relaxed.pdb beside each design and <complex>_relax.tsv')
    ap.add_argument('--relax_iters', type=int, default=200, help='--relax: energy evaluations per design at most')
    ap.add_argument('--relax_flank', type=int, default=0, help='--relax: linked neighbours on each side of the designed residues that move too')
    ap.add_argument('--relax_restraint', type=float, default=0.0, help='--relax: weight of the C-alpha restraint to the design (0: none; k > 0 '
                    'bounds the motion by k * sum |dCA|^2 <= the violation energy of the design)')
    ap.add_argument('--interface', action='store_true', help='interface row of every design on the GPU (abx_interface_scores): buried '
                    'solvent-accessible surface, interface residues and antibody-antigen contacts, and their difference to the input complex; '
                    'writes <complex>_interface.tsv')
    ap.add_argument('--interface_points', type=int, default=128, help='--interface: sphere points per atom (1..1024)')
    ap.add_argument('--interface_probe', type=float, default=1.4, help='--interface: probe radius (Angstrom)')
    ap.add_argument('--interface_cutoff', type=float, default=4.0, help='--interface: heavy-atom contact distance (Angstrom)')
    ap.add_argument('--confidence', action='store_true', help='confidence row of every design on the GPU (abx_distogram_scores): the distogram '
                    'head of the last network call against the emitted structure - negative log-likelihood of the realised distances, entropy, '
                    'expected and realised antigen contacts of the designed residues; writes <complex>_confidence.tsv')
    ap.add_argument('--confidence_cutoff', type=float, default=8.0, help='--confidence: contact distance of the pseudo-beta atoms (Angstrom)')
    ap.add_argument('--confidence_planes', action='store_true', help='--confidence: also write <complex>_confidence_contacts.npy, the mean '
                    'predicted contact probability over the designs, (L, L)')
    ap.add_argument('--accuracy', action='store_true', help='accuracy row of every design on the GPU (abx_accuracy_scores): lDDT against the '
                    'input structure and the calibration of pLDDT, TM-score / GDT / RMSD of the C-alpha, native antibody-antigen residue '
                    'contacts kept (Fnat); writes <complex>_accuracy.tsv')
    ap.add_argument('--accuracy_radius', type=float, default=15.0, help='--accuracy: lDDT inclusion radius (Angstrom)')
    ap.add_argument('--accuracy_contact', type=float, default=5.0, help='--accuracy: heavy-atom distance of a residue contact (Angstrom)')
    ap.add_argument('--accuracy_rows', action='store_true', help='--accuracy: also write <complex>_accuracy_rows.npy, the per-residue lDDT '
                    '(all atoms, backbone, C-alpha) and pair count of every sample, (N, L, 4)')
    ap.add_argument('--polar', action='store_true', help='polar row of every design on the GPU (abx_polar_scores): heavy-atom hydrogen bonds '
                    'and salt bridges across the interface, polar atoms buried by binding without a partner, and their difference to the input '
                    'complex; writes <complex>_polar.tsv')
    ap.add_argument('--polar_hb_max', type=float, default=3.5, help='--polar: largest donor-acceptor distance of a hydrogen bond (Angstrom, >= 2.0)')
    ap.add_argument('--polar_hb_angle', type=float, default=90.0, help='--polar: smallest antecedent-atom...partner angle (degrees, [90, 180))')
    ap.add_argument('--polar_salt', type=float, default=4.0, help='--polar: cation-anion distance of a salt bridge (Angstrom)')
    ap.add_argument('--polar_rows', action='store_true', help='--polar: also write <complex>_polar_rows.npy, (N, L, 4) int16 per residue: '
                    'cross-side and same-side hydrogen bonds, salt bridges, unsatisfied atoms')
    ap.add_argument('--ensemble', action='store_true', help='compare the designs of a complex with each other on the GPU (abx_ensemble_pairs, '
                    'abx_ensemble_cluster): pairwise RMSD of the designed residues, Daura clusters and their centres; writes <complex>_ensemble.tsv')
    ap.add_argument('--ensemble_cutoff', type=float, default=1.0, help='--ensemble: neighbour distance of the clusters (Angstrom)')
    ap.add_argument('--ensemble_metric', default='fit', choices=['fit', 'frame'], help='--ensemble: cluster on the RMSD after superposition '
                    '(fit: shape) or in the frame of the complex (frame: placement)')
    ap.add_argument('--ensemble_atoms', default='backbone', choices=['ca', 'backbone'], help='--ensemble: compared atoms of the designed residues')
    ap.add_argument('--ensemble_matrix', action='store_true', help='--ensemble: also write <complex>_ensemble_rmsd.npy, the (3, N, N) planes '
                    'rmsd_fit, rmsd_frame, seq_diff')
    return ap


def main(argv=None):
    ap = build_parser()
    a = ap.parse_args(argv)
    if a.exact_gemm:
        from abx_amd import ops
        ops.GEMM_EXACT = True
    if a.gpu_list and len(a.gpu_list) > 1 and 'WORLD_SIZE' not in os.environ:
        import sys
        rc_ = _relaunch_on_gpus(a.gpu_list, sys.argv[1:] if argv is None else argv)
        if rc_ != 0:
            raise SystemExit(rc_)
        return []
    if a.name_idx and not a.data_dir:
        ap.error('--name_idx needs --data_dir')
    opt_steps = [a.optimize_steps]
    if a.model_features:
        area, steps = read_model_features(a.model_features)
        if area != a.generate_area and a.generate_area != ap.get_default('generate_area'):
            import warnings
            warnings.warn(f'--generate_area {a.generate_area} is overridden by the make_diffuser_features entry of --model_features ({area})')
        a.generate_area = area
        if a.mode == 'optimize' and steps:
            opt_steps = steps

    rank, world = int(os.environ.get('RANK', 0)), int(os.environ.get('WORLD_SIZE', 1))
    local_rank = int(os.environ.get('LOCAL_RANK', 0))
    if a.gpu_list and len(a.gpu_list) == 1 and not a.device and 'WORLD_SIZE' not in os.environ:
        a.device = f'cuda:{a.gpu_list[0]}'
    if a.device in ('gpu', 'cpu'):                      # the reference's --device choices
        if a.device == 'cpu':
            raise SystemExit('abx_amd runs on an MI355X only: there is no CPU path (the oracle under oracle/ is test infrastructure)')
        a.device = None
    dev = torch.device(a.device if a.device else ('cuda:0' if a.debug_one_gpu else f'cuda:{local_rank}'))
    torch.cuda.set_device(dev)
    group = None
    if world > 1 or a.force_collective:
        import torch.distributed as dist
        if not dist.is_initialized():
            os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
            os.environ.setdefault('MASTER_PORT', '29577')
            if a.debug_one_gpu:
                dist.init_process_group('gloo', rank=rank, world_size=world)
            else:
                dist.init_process_group('nccl', rank=rank, world_size=world, device_id=dev)      # "nccl" is RCCL on ROCm

    cfg = load_config(a.model_config) if a.model_config else default_config()
    diffuser = FullDiffuser.get(cfg.diffuser).to(dev)
    model = ScoreNetwork(cfg.model, diffuser)
    if a.ckpt:
        sd = torch.load(a.ckpt, map_location='cpu')['model_state_dict']
    else:
        sd = synthetic.random_state_dict(OrderedDict((k, tuple(v.shape)) for k, v in model.state_dict().items()), seed=a.seed)
    model.load_state_dict(sd, strict=True)
    model = model.to(dev).eval()

    guide = None
    if a.guidance:
        from .guidance import ViolationGuidance
        guide = ViolationGuidance(scale_trans=a.guidance_scale[0], scale_rot=a.guidance_scale[1])
    N = a.num_samples
    # jobs: (kind, reference to the complex, output directory, optimize step, inference.py layout?, directory of the ground-truth copy)
    jobs = []
    if a.name_idx:
        with open(a.name_idx) as f:
            names = [x.strip() for x in f if x.strip()]
        root = os.path.join(a.output_dir, a.mode)
        for step in (opt_steps if a.mode == 'optimize' else [None]):
            out = os.path.join(root, f'OPT-{step}') if a.mode == 'optimize' else root
            # inference.py:321-322, 354-355: the ground truth goes to <output_dir>/<mode>/reference/ in every mode (in optimize mode it
            # is re-written, unchanged, for every step: once is enough)
            jobs += [('npz', nm, out, step, True, os.path.join(root, 'reference') if step == opt_steps[0] or a.mode != 'optimize' else None)
                     for nm in names]
    else:
        for step in (opt_steps if a.mode == 'optimize' else [None]):
            out = os.path.join(a.output_dir, f'OPT-{step}') if (a.mode == 'optimize' and len(opt_steps) > 1) else a.output_dir
            jobs += [('pdb' if path is not None else 'synthetic', path, out, step, False, None)
                     for path in (complex_list(a.pdb_file, a.pdb_list, a.pdb_dir) or [None])]
    os.makedirs(a.output_dir, exist_ok=True)
    files = []
    import time
    del TIMINGS[:]

    loaded = {}

    def load_job(ji):
        """The complex of job ji (host tensors, read once per complex): dict(cb, cname, L, Lab, kind)."""
        kind, path = jobs[ji][0], jobs[ji][1]
        key = (kind, path)
        if key not in loaded:
            if kind in ('pdb', 'npz'):
                from .data.antibody import load_complex, load_complex_npz
                cb = load_complex(path, seed=a.seed) if kind == 'pdb' else load_complex_npz(a.data_dir, path, seed=a.seed)
                one = {k: v for k, v in cb.items() if torch.is_tensor(v)}
                loaded[key] = dict(cb=cb, one=one, cname=cb['name'][0], L=one['seq'].shape[1], Lab=one['anchor_flag'].shape[1])
            else:
                w = synthetic.WORKLOADS[a.workload]
                cx = synthetic.make_complex(seed=a.seed + 1, **w)
                loaded[key] = dict(cb=None, one={k: v[None] for k, v in cx.items()}, cname=f'{a.workload}_H_L_A', L=cx['seq'].shape[0],
                                   Lab=cx['anchor_flag'].shape[0], w=w, seq=cx['seq'].tolist())
        return loaded[key]

    # ---- who runs what.  One complex, or fewer (complex, 50-sample block) units than ranks: the samples of every complex are sharded
    # over the ranks and gathered per complex.  A set of complexes (BASELINE configs 3 / 4): whole units are dealt to the ranks
    # longest-first (cost ~ L^3 x samples), each GPU runs batches of >= 50 samples (0.98 of the 100-sample rate per GPU instead of the
    # 0.91 of 12-13-sample shards), and ONE gather of the designs table closes the set.  Per-sample noise keys make
    # a sample's trajectory independent of where and with whom it runs, so both schemes write the same files.
    plan = None
    if (world > 1 or a.force_collective) and len(jobs) >= 2 and not a.shard_samples:
        if a.min_block < 1:
            raise SystemExit('--min_block must be >= 1')
        plan = sampler.plan_work_units([float(load_job(ji)['L']) ** 3 for ji in range(len(jobs))], N, world, min_block=a.min_block, force=a.force_collective)
    if plan is None:
        work = [(ji, sampler.shard_sample_ids(N, rank, world)) for ji in range(len(jobs))]
    else:
        work = plan[rank]
        if a.verbose or rank == 0:
            print(f'set-level schedule: {sum(len(p) for p in plan)} units of >= {min(a.min_block, N)} samples over {world} ranks; '
                  f'rank {rank} runs {[(jobs[ji][1], len(ids_)) for ji, ids_ in work]}')
    set_rows = []                                               # set-level mode: (job, sample id, mean pLDDT, Lab, tokens...) rows of this rank
    maxLab = max([load_job(ji)['Lab'] for ji in range(len(jobs))]) if plan is not None else 0
    NS = 0                                                      # --score: score columns per sample (+ (t, scores) of every trajectory record)
    if a.score:
        from .metrics import SCORE_COLUMNS, DesignScorer
        NS = len(SCORE_COLUMNS)
    n_rec = a.num_t if (a.score and a.mode == 'trajectory') else 0
    NR = 0                                                      # --relax: report columns per sample (+ the scores of the relaxed structure)
    if a.relax:
        from .relax import RELAX_COLUMNS, ViolationRelaxer
        NR = len(RELAX_COLUMNS) + NS
    NI = 0                                                      # --interface: the row (+ that of the relaxed structure) + the wild type's row
    if a.interface:
        from .interface import INTERFACE_COLUMNS, InterfaceScorer
        if not 1 <= a.interface_points <= 1024 or a.interface_probe < 0 or a.interface_cutoff <= 0:
            raise SystemExit('--interface_points must be in 1..1024, --interface_probe >= 0, --interface_cutoff > 0')
        NI = len(INTERFACE_COLUMNS) * (3 if a.relax else 2)
    NCF = 0                                                     # --confidence: the row (+ that of the relaxed structure) + the sample's wild row
    if a.confidence:
        from .confidence import CONFIDENCE_COLUMNS, DistogramScorer
        if not a.confidence_cutoff > 0:
            raise SystemExit('--confidence_cutoff must be > 0')
        if a.confidence_planes and plan is not None:
            raise SystemExit('--confidence_planes needs the sample-sharded schedule (--shard_samples): a set-level run gathers one table only')
        NCF = len(CONFIDENCE_COLUMNS) * (3 if a.relax else 2)
    elif a.confidence_planes:
        raise SystemExit('--confidence_planes needs --confidence')
    NA = 0                                                      # --accuracy: the row (+ that of the relaxed structure) + the wild type's row
    if a.accuracy:
        from .accuracy import ACCURACY_COLUMNS, AccuracyScorer
        if not a.accuracy_radius > 0 or not a.accuracy_contact > 0:
            raise SystemExit('--accuracy_radius and --accuracy_contact must be > 0')
        if a.accuracy_rows and plan is not None:
            raise SystemExit('--accuracy_rows needs the sample-sharded schedule (--shard_samples): a set-level run gathers one table only')
        NA = len(ACCURACY_COLUMNS) * (3 if a.relax else 2)
    elif a.accuracy_rows:
        raise SystemExit('--accuracy_rows needs --accuracy')
    NP = 0                                                      # --polar: the row (+ that of the relaxed structure) + the wild type's row
    if a.polar:
        from .polar import POLAR_COLUMNS, PolarScorer
        if not a.polar_hb_max >= 2.0 or not 90.0 <= a.polar_hb_angle < 180.0 or not a.polar_salt >= 0:
            raise SystemExit('--polar_hb_max must be >= 2.0 (the smallest donor-acceptor distance), --polar_hb_angle in [90, 180), --polar_salt >= 0')
        if not 1 <= a.interface_points <= 1024 or a.interface_probe < 0:
            raise SystemExit('--interface_points must be in 1..1024, --interface_probe >= 0')
        if a.polar_rows and plan is not None:
            raise SystemExit('--polar_rows needs the sample-sharded schedule (--shard_samples): a set-level run gathers one table only')
        NP = len(POLAR_COLUMNS) * (3 if a.relax else 2)
    elif a.polar_rows:
        raise SystemExit('--polar_rows needs --polar')
    NE = 0                                                      # --ensemble, set-level rows: the antibody backbone (maxLab, 4, 3), f32 values
    analyzers = {}                                              # --ensemble: job -> EnsembleAnalyzer (the compared rows of the complex)
    if a.ensemble:
        from . import ensemble
        if not 1 <= N <= ensemble.MAX_N or not a.ensemble_cutoff >= 0:
            raise SystemExit(f'--ensemble compares 1..{ensemble.MAX_N} samples of a complex, --ensemble_cutoff must be >= 0')
        NE = 12 * maxLab
    E0 = 4 + maxLab + NS + n_rec * (1 + NS)                     # set-level rows: the backbone columns follow the scores
    WIDTH = E0 + NE + NCF + NA + NP + NR + NI                   # (the confidence, accuracy and polar columns sit between the backbone and the relax report)

    def analyze_ensemble(ji, out_dir, cname, ids, seq, backbone):
        """The ensemble tables of job ji from the gathered tokens (N, Lab) and backbone (N, Lab, 4, 3) in the order of `ids`."""
        import numpy as np
        if ji not in analyzers:                                 # a complex this rank did not sample: its features give the compared rows
            J = load_job(ji)
            raw = {k: v.to(dev) for k, v in J['one'].items()}
            fb = features.build_features(raw, diffuser, generate_area=a.generate_area, opt_step=jobs[ji][3] if a.mode == 'optimize' else None,
                                         noise=features.per_sample_init_noise([0], J['L'], a.seed, dev))
            analyzers[ji] = ensemble.EnsembleAnalyzer(fb, atoms=a.ensemble_atoms, metric=a.ensemble_metric, cutoff=a.ensemble_cutoff)
        an = analyzers[ji]
        x = torch.zeros(seq.shape[0], an.Lab, 14, 3, dtype=torch.float32, device=dev)
        x[:, :, :4] = backbone.to(dev)
        res = an.analyze(x, seq.to(dev).long())
        table = res['table'].cpu().numpy()
        centres = res['centres'].cpu().tolist()[:int(res['n_clusters'])]
        out = [_write_ensemble(out_dir, cname, ensemble.summary(table, an.n_region), list(zip(ids, table.tolist())), centres)]
        if a.ensemble_matrix:
            out.append(os.path.join(out_dir, f'{cname}_ensemble_rmsd.npy'))
            np.save(out[-1], res['planes'].cpu().numpy())
        return out

    ref_written = set()
    for ji, ids in work:
        kind, path, out_dir, opt_step, ref_layout, ref_dir = jobs[ji]
        n = len(ids)
        t_job = time.perf_counter()
        os.makedirs(out_dir, exist_ok=True)
        J = load_job(ji)
        cname, L, Lab = J['cname'], J['L'], J['Lab']
        one = {k: v.to(dev) for k, v in J['one'].items()}
        if kind in ('pdb', 'npz'):
            cb = J['cb']
            meta = {k: list(cb[k]) * n for k in ('str_heavy_seq', 'str_light_seq', 'antigen_origin_str_seq',
                                                 'antigen_origin_atom14_gt_positions', 'antigen_origin_atom14_gt_exists',
                                                 'antigen_origin_chain_ids')}
            # the "reference batch" = the ground-truth antibody with pLDDT 100, once per complex: by rank 0 when the samples of the
            # complex are sharded, by the rank that runs the complex's first block under the set-level schedule
            first_block = bool(ids) and ids[0] == 0
            if ref_layout and ref_dir is not None and (rank == 0 if plan is None else first_block) and (cname, ref_dir) not in ref_written:
                from .io import postprocess_trajectory
                ref_written.add((cname, ref_dir))
                ref_meta = {k: list(cb[k]) for k in meta}
                ref_meta['name'] = [cname]
                files += postprocess_trajectory(ref_meta, [{'seq': one['seq'][:, :Lab], 'atom14_results': one['atom14_gt_positions'][:, :Lab],
                                                            'pLDDT': torch.full((1, Lab), 100.0), 'time': 0.0}], ref_dir)
        else:
            w = J['w']
            nh, nl = w['L_heavy'], w['L_light']
            meta = dict(str_heavy_seq=[index_to_str_seq(J['seq'][:nh])] * n, str_light_seq=[index_to_str_seq(J['seq'][nh:nh + nl])] * n)
        if ref_layout:                                      # inference.py:363-367: <k:04d>/<name>.pdb
            meta['name'] = [cname] * n
            meta['subdir'] = [f'{i:04d}' for i in ids]
        else:
            meta['name'] = sample_names(cname, ids, N)
        if n > 0:
            raw = {k: v.expand(n, *v.shape[1:]).contiguous() for k, v in one.items()}
            batch = features.build_features(raw, diffuser, generate_area=a.generate_area,
                                            opt_step=opt_step if a.mode == 'optimize' else None,
                                            noise=features.per_sample_init_noise(ids, L, a.seed, dev))
            batch['_shared_context'] = True
            diffuser.seed = a.seed
            writer = TrajectoryWriter(meta, out_dir, multi=a.mode == 'trajectory')
            iface = InterfaceScorer(batch, n_points=a.interface_points, probe=a.interface_probe, cutoff=a.interface_cutoff) if a.interface else None
            conf = None
            if a.confidence:
                conf = DistogramScorer(batch, model, cutoff=a.confidence_cutoff, conf=cfg.model.heads.distogram)
                conf.want_planes = a.confidence_planes
            acc = AccuracyScorer(batch, radius=a.accuracy_radius, contact=a.accuracy_contact) if a.accuracy else None
            pol = None
            if a.polar:                                         # (with --interface: one surface call per structure set serves both tables)
                pol = PolarScorer(batch, hb_max=a.polar_hb_max, hb_angle=a.polar_hb_angle, salt=a.polar_salt, n_points=a.interface_points,
                                  probe=a.interface_probe, interface=iface)
                pol.want_rows = a.polar_rows
            if a.ensemble and ji not in analyzers:
                analyzers[ji] = ensemble.EnsembleAnalyzer(batch, atoms=a.ensemble_atoms, metric=a.ensemble_metric, cutoff=a.ensemble_cutoff)
            torch.cuda.synchronize()
            t_feat = time.perf_counter()
            traj = sampler.sample_fn(batch, cfg, diffuser, model, mode=a.mode, num_t=a.num_t,
                                     sample_ids=torch.tensor(ids, device=dev, dtype=torch.int64), on_record=writer.submit, guidance=guide,
                                     **({'scorer': DesignScorer(batch)} if a.score else {}),
                                     **({'relaxer': ViolationRelaxer(batch, flank=a.relax_flank, max_iter=a.relax_iters,
                                                                     k_restraint=a.relax_restraint)} if a.relax else {}),
                                     **({'interface': iface} if a.interface else {}),
                                     **({'confidence': conf} if a.confidence else {}),
                                     **({'accuracy': acc} if a.accuracy else {}),
                                     **({'polar': pol} if a.polar else {}))
            torch.cuda.synchronize()
            t_samp = time.perf_counter()
            new_files = writer.close()
            if a.relax:                                         # <name>_relaxed.pdb beside every design, through the same writer
                from .io import postprocess_trajectory
                last = traj[-1]
                new_files += postprocess_trajectory(dict(meta, suffix='_relaxed'), [{'seq': last['seq'], 'atom14_results': last['atom14_relaxed'],
                                                                                     'pLDDT': last['pLDDT'], 'time': 0.0}], out_dir)
            files += new_files
            t_done = time.perf_counter()
            TIMINGS.append(dict(complex=cname, L=int(L), samples=n, mode=a.mode, opt_step=opt_step, read_and_featurise_s=t_feat - t_job,
                                sampling_s=t_samp - t_feat, writer_tail_s=t_done - t_samp, files=len(new_files),
                                range_fallbacks=len(traj[-1].get('range_fallbacks', [])),
                                range_sticky_ops=list(traj[-1].get('range_sticky_ops', []))))
            local = {'seq': traj[-1]['seq'], 'pLDDT': traj[-1]['pLDDT']}
            if a.score:
                local['scores'] = traj[-1]['scores']
                if n_rec:                                       # (samples, records, 1 + NS): t, then the scores of the record
                    local['traj_scores'] = torch.stack([torch.cat([torch.full((n, 1), r['time'], dtype=torch.float64, device=dev), r['scores']], 1)
                                                        for r in traj], 1)
            if a.relax:
                local['relax'] = torch.cat([traj[-1]['relax']] + ([traj[-1]['scores_relaxed']] if a.score else []), 1)
            wild_pts = pol.new_points(1) if (a.polar and a.interface) else None      # the wild type's point counts serve both tables too
            if a.interface:                                     # the wild type's row rides along in every row: any rank can write the table
                local['interface'] = torch.cat([traj[-1]['interface']] + ([traj[-1]['interface_relaxed']] if a.relax else []) +
                                               [iface.wild(points=wild_pts).expand(n, -1)], 1)
            if a.confidence:                                    # every sample's own wild row rides along: any rank can write the table
                local['confidence'] = torch.cat([traj[-1]['confidence']] + ([traj[-1]['confidence_relaxed']] if a.relax else []) +
                                                [traj[-1]['confidence_wild']], 1)
                if a.confidence_planes:
                    local['confidence_contacts'] = traj[-1]['confidence_planes'][0]
            if a.accuracy:                                      # the wild type's row rides along in every row: any rank can write the table
                local['accuracy'] = torch.cat([traj[-1]['accuracy']] + ([traj[-1]['accuracy_relaxed']] if a.relax else []) +
                                              [acc.wild().expand(n, -1)], 1)
                if a.accuracy_rows:
                    local['accuracy_rows'] = traj[-1]['accuracy_rows']
            if a.polar:                                         # the wild type's row rides along in every row: any rank can write the table
                local['polar'] = torch.cat([traj[-1]['polar']] + ([traj[-1]['polar_relaxed']] if a.relax else []) +
                                           [pol.wild(points=wild_pts).expand(n, -1)], 1)
                if a.polar_rows:
                    local['polar_rows'] = traj[-1]['polar_rows']
            if a.ensemble:                                      # N, CA, C, O of the antibody rows: what the comparison reads
                local['backbone'] = traj[-1]['atom14_results'][:, :, :4].float().contiguous()
        else:                                                   # more ranks than samples: join the gather with zero-row blocks
            local = {'seq': torch.zeros(0, Lab, dtype=torch.int64, device=dev), 'pLDDT': torch.zeros(0, Lab, device=dev)}
            if a.score:
                local['scores'] = torch.zeros(0, NS, dtype=torch.float64, device=dev)
                if n_rec:
                    local['traj_scores'] = torch.zeros(0, n_rec, 1 + NS, dtype=torch.float64, device=dev)
            if a.relax:
                local['relax'] = torch.zeros(0, NR, dtype=torch.float64, device=dev)
            if a.interface:
                local['interface'] = torch.zeros(0, NI, dtype=torch.float64, device=dev)
            if a.confidence:
                local['confidence'] = torch.zeros(0, NCF, dtype=torch.float64, device=dev)
                if a.confidence_planes:
                    local['confidence_contacts'] = torch.zeros(0, L, L, dtype=torch.float32, device=dev)
            if a.accuracy:
                local['accuracy'] = torch.zeros(0, NA, dtype=torch.float64, device=dev)
                if a.accuracy_rows:
                    local['accuracy_rows'] = torch.zeros(0, L, 4, dtype=torch.float64, device=dev)
            if a.polar:
                local['polar'] = torch.zeros(0, NP, dtype=torch.float64, device=dev)
                if a.polar_rows:
                    local['polar_rows'] = torch.zeros(0, L, 4, dtype=torch.int32, device=dev)
            if a.ensemble:
                local['backbone'] = torch.zeros(0, Lab, 4, 3, dtype=torch.float32, device=dev)
        if plan is not None:
            row = torch.zeros(n, WIDTH, dtype=torch.float64)
            row[:, 0], row[:, 1], row[:, 3] = ji, torch.tensor(ids, dtype=torch.float64), Lab
            row[:, 2] = local['pLDDT'].float().mean(1).double().cpu()       # (the float32 mean of the sample-sharded path: same TSV digits)
            row[:, 4:4 + Lab] = local['seq'].double().cpu()
            if a.score:
                row[:, 4 + maxLab:4 + maxLab + NS] = local['scores'].cpu()
                if n_rec:
                    row[:, 4 + maxLab + NS:4 + maxLab + NS + n_rec * (1 + NS)] = local['traj_scores'].reshape(n, -1).cpu()
            if a.ensemble:                                      # f32 values are exact in float64
                row[:, E0:E0 + 12 * Lab] = local['backbone'].reshape(n, -1).double().cpu()
            if a.confidence:
                row[:, E0 + NE:E0 + NE + NCF] = local['confidence'].cpu()
            if a.accuracy:
                row[:, E0 + NE + NCF:E0 + NE + NCF + NA] = local['accuracy'].cpu()
            if a.polar:
                row[:, E0 + NE + NCF + NA:E0 + NE + NCF + NA + NP] = local['polar'].cpu()
            if a.relax:
                row[:, row.shape[1] - NI - NR:row.shape[1] - NI] = local['relax'].cpu()
            if a.interface:
                row[:, row.shape[1] - NI:] = local['interface'].cpu()
            set_rows.append(row)
            continue
        if a.debug_one_gpu and world > 1:                       # gloo moves host tensors
            local = {k: v.cpu() for k, v in local.items()}
        res = sampler.gather_results(local, N, rank, world, group, force=a.force_collective)
        if rank == 0:
            sc = res['scores'].tolist() if a.score else None
            files.append(_write_designs(out_dir, cname, [(i, float(res['pLDDT'][i].float().mean()), res['seq'][i].tolist()) + ((sc[i],) if a.score else ())
                                                         for i in range(N)]))
            if n_rec:
                files.append(_write_trajectory_scores(out_dir, cname, res['traj_scores'].cpu()))
            if a.relax:
                files.append(_write_relax(out_dir, cname, list(enumerate(res['relax'].tolist())), a.score))
            if a.interface:
                it = res['interface'].tolist()
                files.append(_write_interface(out_dir, cname, it[0][NI - len(INTERFACE_COLUMNS):], list(enumerate(it)), a.relax))
            if a.confidence:
                files.append(_write_confidence(out_dir, cname, list(enumerate(res['confidence'].tolist())), a.relax))
                if a.confidence_planes:
                    import numpy as np
                    files.append(os.path.join(out_dir, f'{cname}_confidence_contacts.npy'))
                    np.save(files[-1], res['confidence_contacts'].double().mean(0).float().cpu().numpy())
            if a.accuracy:
                at = res['accuracy'].tolist()
                files.append(_write_accuracy(out_dir, cname, at[0][NA - len(ACCURACY_COLUMNS):], list(enumerate(at)), a.relax))
                if a.accuracy_rows:
                    import numpy as np
                    files.append(os.path.join(out_dir, f'{cname}_accuracy_rows.npy'))
                    np.save(files[-1], res['accuracy_rows'].cpu().numpy())
            if a.polar:
                pt = res['polar'].tolist()
                files.append(_write_polar(out_dir, cname, pt[0][NP - len(POLAR_COLUMNS):], list(enumerate(pt)), a.relax))
                if a.polar_rows:
                    import numpy as np
                    files.append(os.path.join(out_dir, f'{cname}_polar_rows.npy'))
                    np.save(files[-1], res['polar_rows'].cpu().numpy().astype(np.int16))
            if a.ensemble:
                files += analyze_ensemble(ji, out_dir, cname, list(range(N)), res['seq'], res['backbone'])
    if plan is not None:
        # ---- the one collective of the set: every rank's rows of the designs table (counts known from the common plan)
        table = torch.cat(set_rows, 0) if set_rows else torch.zeros(0, WIDTH, dtype=torch.float64)
        if not (a.debug_one_gpu and world > 1):
            table = table.to(dev)
        counts = [sum(len(ids_) for _, ids_ in p) for p in plan]
        full = sampler.gather_rows(table, counts, rank, world, group, force=a.force_collective).cpu()
        if rank == 0:
            for ji in range(len(jobs)):
                rows = full[full[:, 0] == ji]
                rows = rows[torch.argsort(rows[:, 1])]
                assert rows.shape[0] == N, (jobs[ji][1], rows.shape)
                files.append(_write_designs(jobs[ji][2], load_job(ji)['cname'],
                                            [(int(r[1]), float(r[2]), r[4:4 + int(r[3])].long().tolist()) +
                                             ((r[4 + maxLab:4 + maxLab + NS].tolist(),) if a.score else ()) for r in rows]))
                if n_rec:
                    files.append(_write_trajectory_scores(jobs[ji][2], load_job(ji)['cname'],
                                                          rows[:, 4 + maxLab + NS:4 + maxLab + NS + n_rec * (1 + NS)].reshape(N, n_rec, 1 + NS)))
                if a.relax:
                    files.append(_write_relax(jobs[ji][2], load_job(ji)['cname'], [(int(r[1]), r[r.shape[0] - NI - NR:r.shape[0] - NI].tolist()) for r in rows], a.score))
                if a.interface:
                    files.append(_write_interface(jobs[ji][2], load_job(ji)['cname'], rows[0, rows.shape[1] - len(INTERFACE_COLUMNS):].tolist(),
                                                  [(int(r[1]), r[r.shape[0] - NI:].tolist()) for r in rows], a.relax))
                if a.confidence:
                    files.append(_write_confidence(jobs[ji][2], load_job(ji)['cname'], [(int(r[1]), r[E0 + NE:E0 + NE + NCF].tolist()) for r in rows], a.relax))
                if a.accuracy:
                    A0 = E0 + NE + NCF
                    files.append(_write_accuracy(jobs[ji][2], load_job(ji)['cname'], rows[0, A0 + NA - len(ACCURACY_COLUMNS):A0 + NA].tolist(),
                                                 [(int(r[1]), r[A0:A0 + NA].tolist()) for r in rows], a.relax))
                if a.polar:
                    P0 = E0 + NE + NCF + NA
                    files.append(_write_polar(jobs[ji][2], load_job(ji)['cname'], rows[0, P0 + NP - len(POLAR_COLUMNS):P0 + NP].tolist(),
                                              [(int(r[1]), r[P0:P0 + NP].tolist()) for r in rows], a.relax))
                if a.ensemble:
                    lab = int(rows[0, 3])
                    files += analyze_ensemble(ji, jobs[ji][2], load_job(ji)['cname'], [int(r[1]) for r in rows], rows[:, 4:4 + lab].long(),
                                              rows[:, E0:E0 + 12 * lab].float().reshape(N, lab, 4, 3))
    if world > 1 or a.force_collective:
        import torch.distributed as dist
        dist.barrier()
        if a.force_collective and world == 1:
            dist.destroy_process_group()
    print(f'rank {rank}/{world}: {len(files)} files in {a.output_dir}')
    return files


if __name__ == '__main__':
    main()
