"""End-to-end driver in the shape of the reference's design.py / inference.py main (design.py:277-375, inference.py:59-82,
275-392): build the diffuser and the score network, featurise each complex, run the reverse diffusion for `num_samples` samples
and write the PDB files (per step in trajectory mode, asynchronously).

    python -m abx_amd.design --pdb_file 6ct7_H_L_S.pdb --num_samples 100 --mode design --output_dir out/      (raw PDB, 8f-1)
    python -m abx_amd.design --workload L256 --num_samples 4 --mode trajectory --num_t 10 --output_dir out/   (synthetic complex)
    python -m abx_amd.design --pdb_file 6ct7_H_L_S.pdb --mode optimize --optimize_steps 10 --guidance --num_samples 100     (config 4)
    python -m abx_amd.design --pdb_file 6ct7_H_L_S.pdb --mode optimize --optimize_steps 10 --guidance --guidance_contact 1 \
        --guidance_hotspots epitope --num_samples 100                           (+ interface guidance: contacts, hotspots, restraints)
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
The per-design analyses run on the GPU without a host synchronisation in the sampling loop; abx_amd.analyses states each of them once.
--score: per-CDR RMSD / AAR, violation and clash counts as further columns of <complex>_designs.tsv; in trajectory mode also
<complex>_trajectory_scores.tsv.  --relax: rigid-body + chi minimisation of the violation energy of the designed residues;
<name>_relaxed.pdb beside every design, <complex>_relax.tsv, and _relaxed columns in the six tables that follow, each with a `wild`
line for the input complex and one line per sample.  --interface: buried surface, interface residues and contacts,
<complex>_interface.tsv.  --confidence: the distogram head of the last network call against the emitted structure,
<complex>_confidence.tsv (--confidence_planes: also <complex>_confidence_contacts.npy).  --accuracy: lDDT, TM-score / GDT / RMSD and
Fnat against the input structure, <complex>_accuracy.tsv (--accuracy_rows: also <complex>_accuracy_rows.npy).  --polar: hydrogen bonds,
salt bridges and unsatisfied polar atoms across the interface, <complex>_polar.tsv (--polar_rows: also <complex>_polar_rows.npy).
--developability: spatial aggregation propensity, chain charges and sequence liabilities of the free antibody,
<complex>_developability.tsv (--developability_rows: also <complex>_developability_rows.npy).  --shape: the shape complementarity Sc
of the interface (Lawrence & Colman), both directions, the designed residues' share, gaps and dot counts, <complex>_shape.tsv.
--patches: the patches of surface hydrophobicity and of charge around the CDRs of the free antibody (TAP's PSH / PPC / PNC), its charge
symmetry and the charge pairing across the interface, <complex>_patches.tsv (--patches_rows: also <complex>_patches_rows.npy).
--torsions: cis and twisted peptides, residues with phi >= 0, the ABEGO classes of the designed residues and the chi1 / chi1+2 recovery
against the input structure, <complex>_torsions.tsv with the ABEGO string as its last column (--torsions_rows: also
<complex>_torsions_rows.npy).
--secondary: DSSP over the antibody - backbone hydrogen bonds on a virtual H, bridges and the eight states of the designed residues
against the input structure, <complex>_secondary.tsv with the state string as its last column (--secondary_rows: also
<complex>_secondary_rows.npy).
--ensemble: the designs of a complex compared with each other, Daura clusters and their centres, <complex>_ensemble.tsv
(--ensemble_matrix: also <complex>_ensemble_rmsd.npy).  No flag changes a file that another one writes; the _rows / _planes tables need
the sample-sharded schedule (--shard_samples).
--seq_bias / --seq_forbid / --seq_fix: sequence constraints inside the step (abx_amd.constraints): per-residue logit biases, letters
forbidden at every designed residue, a residue held to given letters; with any of them <complex>_sequence.tsv, one line per designed
residue: the letter counts among the designs and `violations` (0).
Weights: a checkpoint with the reference's `model_state_dict`, or seeded random weights (no checkpoint ships with the reference)."""
import argparse
import os
from collections import OrderedDict

import torch

from . import analyses, features, sampler, synthetic
from .analyses import (_write_accuracy, _write_confidence, _write_designs, _write_ensemble, _write_interface, _write_polar,      # noqa: F401
                       _write_relax, _write_trajectory_scores, _write_developability, _write_shape, _write_patches, _write_torsions, _write_secondary)                 # (the table writers, under the names the host tests call)
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
    ap.add_argument('--guidance_contact', type=float, default=0.0, metavar='W', help='interface guidance (abx_contact_grad): weight of the smooth '
                    'count of heavy-atom contacts between the designed residues and the antigen (0: off)')
    ap.add_argument('--guidance_contact_range', type=float, nargs=2, default=[4.0, 8.0], metavar=('D0', 'D1'),
                    help='--guidance_contact: a contact counts fully within D0 and not at all beyond D1 (Angstrom)')
    ap.add_argument('--guidance_hotspots', nargs='+', default=None, metavar='RES', help="interface guidance: antigen residues that a designed "
                    "residue should come near, as <chain letter>:<residue index as featurised>, or 'epitope' = the antigen residues the "
                    "input loop touches")
    ap.add_argument('--guidance_hotspot_weight', type=float, default=1.0, help='--guidance_hotspots: weight of the hotspot term')
    ap.add_argument('--guidance_restraints', default=None, metavar='FILE', help='interface guidance: pair-distance restraints, one '
                    '`res atom res atom lo hi [weight]` per line')
    ap.add_argument('--seq_bias', default=None, metavar='FILE', help='sequence constraints (abx_amd.constraints): per-residue logit biases, one '
                    '`RES|* LETTERS VALUE` per line; RES as <chain letter>:<residue index as featurised>, * = every designed residue, VALUE a '
                    'float or -inf (the letters are forbidden there)')
    ap.add_argument('--seq_forbid', nargs='+', default=None, metavar='LETTERS', help='sequence constraints: letters forbidden at every designed '
                    'residue, e.g. C M')
    ap.add_argument('--seq_fix', nargs='+', default=None, metavar='RES=LETTERS', help='sequence constraints: only these letters at RES, e.g. '
                    'H:100=Y; wins over --seq_forbid, the kept letters keep their --seq_bias value')
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
    ap.add_argument('--developability', action='store_true', help='developability row of every design on the GPU (abx_developability_scores): '
                    'spatial aggregation propensity, net charge of the heavy and the light chain, sequence liabilities of exposed residues '
                    'of the free antibody, and their difference to the input complex; writes <complex>_developability.tsv')
    ap.add_argument('--developability_radius', type=float, default=10.0, help='--developability: radius of the SAP sphere (Angstrom, > 0)')
    ap.add_argument('--developability_exposed', type=float, default=0.075, help='--developability: smallest relative side-chain area of an '
                    'exposed residue, in [0, 1]')
    ap.add_argument('--developability_rows', action='store_true', help='--developability: also write <complex>_developability_rows.npy, '
                    '(N, L, 4) float64 per residue: mean SAP of its atoms, relative side-chain area, liability bit mask, charge')
    ap.add_argument('--shape', action='store_true', help='shape complementarity of every design on the GPU (abx_shape_scores): the Sc statistic '
                    'of Lawrence & Colman on the contact surface of antibody and antigen, both directions, the dots of the designed residues, '
                    'gaps and dot counts, and their difference to the input complex; writes <complex>_shape.tsv.  The dots are the sphere '
                    'points of --interface_points: Sc rises with them (512 for values comparable with the literature)')
    ap.add_argument('--shape_trim', type=float, default=1.5, help='--shape: width of the peripheral band of the buried surface that is dropped '
                    '(Angstrom, >= 0)')
    ap.add_argument('--shape_weight', type=float, default=0.5, help='--shape: weight of the squared distance in exp(-w d^2) (1 / square Angstrom, >= 0)')
    ap.add_argument('--shape_max_dots', type=int, default=8192, help='--shape: capacity of each dot list of a structure; the run ends by this '
                    'name when an interface outgrows it')
    ap.add_argument('--patches', action='store_true', help='surface patches of every design on the GPU (abx_patch_scores): patches of surface '
                    'hydrophobicity and of positive / negative charge over the exposed residues near the CDRs of the free antibody (PSH, PPC, '
                    'PNC of the Therapeutic Antibody Profiler), its Fv charge symmetry, like and opposite charges facing each other across the '
                    'interface, and their difference to the input complex; writes <complex>_patches.tsv')
    ap.add_argument('--patches_cutoff', type=float, default=7.5, help='--patches: closest heavy-atom distance of a patch pair and of a cross '
                    'pair (Angstrom, > 0)')
    ap.add_argument('--patches_vicinity', type=float, default=4.0, help='--patches: closest heavy-atom distance to an exposed CDR residue that '
                    'puts an exposed residue into the CDR vicinity (Angstrom, > 0)')
    ap.add_argument('--patches_salt', type=float, default=3.2, help='--patches: cation-anion distance of a salt bridge within the antibody; a '
                    'salt-bridged residue takes the hydrophobicity of Gly (Angstrom, > 0)')
    ap.add_argument('--patches_exposed', type=float, default=0.075, help='--patches: smallest relative side-chain area of an exposed residue, '
                    'in [0, 1]')
    ap.add_argument('--patches_rows', action='store_true', help='--patches: also write <complex>_patches_rows.npy, (N, L, 4) float64 per '
                    'residue: its share of PSH, of PPC or PNC, of attract minus repel across the interface, and its flags (1 present, 2 exposed, '
                    '4 CDR seed, 8 vicinity, 16 salt-bridged, 32 region)')
    ap.add_argument('--torsions', action='store_true', help='torsion analysis of every design on the GPU (abx_torsion_scores): cis and twisted '
                    'peptides, residues other than Gly with phi >= 0, the ABEGO classes of the designed residues and their agreement with the input '
                    'structure, the distance of phi / psi / omega to it, the chi1 and chi1+2 recovery, and their difference to the input complex; '
                    'writes <complex>_torsions.tsv, whose last column is the ABEGO string of the designed residues')
    ap.add_argument('--torsions_chi_tol', type=float, default=40.0, help='--torsions: largest |delta chi| of a recovered chi angle (degrees, in '
                    '(0, 180])')
    ap.add_argument('--torsions_rows', action='store_true', help='--torsions: also write <complex>_torsions_rows.npy, (N, Lab, 8) float64 per '
                    'antibody residue: phi, psi, omega of the preceding link, chi1..chi4 in degrees (nan: undefined) and its flags (bits 0-2 the '
                    'ABEGO code 1 A, 2 B, 3 G, 4 E, 5 O; 8 cis, 16 twisted, 32 phi >= 0 and not Gly, 64 region, 128 chi1 compared, 256 chi1 ok)')
    ap.add_argument('--secondary', action='store_true', help='secondary structure of every design on the GPU (abx_secondary_scores): DSSP over '
                    'the antibody - backbone hydrogen bonds on a virtual H, in total, touching and inside the designed residues and kept from the input '
                    'structure, their energy, bridge pairs, the eight states of the designed residues and their agreement with the input structure '
                    '(Q8, Q3), and their difference to the input complex; writes <complex>_secondary.tsv, whose last column is the state string of '
                    'the designed residues (H G I helices, E strand, B bridge, T turn, S bend, - coil)')
    ap.add_argument('--secondary_hb_energy', type=float, default=-0.5, help='--secondary: a backbone hydrogen bond has an energy below this '
                    '(kcal/mol, < 0)')
    ap.add_argument('--secondary_rows', action='store_true', help='--secondary: also write <complex>_secondary_rows.npy, (N, Lab, 6) int32 per '
                    'antibody residue: its state (0 absent, 1 H, 2 G, 3 I, 4 E, 5 B, 6 T, 7 S, 8 coil), bonds donated, bonds accepted, its two lowest '
                    'bridge partner rows (-1: none) and its flags (1 region, 2 present, 4 has H, 8 parallel bridge, 16 antiparallel bridge, 32 bend, '
                    '64 / 128 / 256 a 3- / 4- / 5-turn starts here)')
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
    interface_guided = a.guidance_contact != 0.0 or a.guidance_hotspots is not None or a.guidance_restraints is not None

    constrained = a.seq_bias is not None or a.seq_forbid is not None or a.seq_fix is not None

    def job_chains(kind, path):
        """The chain letters of a job in the order of the chain ids: from the file name, `H L A` for a synthetic workload."""
        if kind in ('pdb', 'npz'):
            from .data.antibody import parse_pdb_name
            _, _, heavy, light, antigen = parse_pdb_name(path)
            return [heavy, light] + list(antigen)
        return ['H', 'L', 'A']

    def job_guide(batch, J, kind, path):
        """The guidance of one featurised batch: the violation terms (one object for the run) and, with the --guidance_contact /
        _hotspots / _restraints options, the interface terms of THIS complex (tables built here, before the sampling loop)."""
        if not interface_guided:
            return guide
        from .guidance import InterfaceGuidance, Sum, parse_residues, parse_restraints
        chains = job_chains(kind, path)
        hot = a.guidance_hotspots
        if hot is not None:
            hot = 'epitope' if list(hot) == ['epitope'] else parse_residues(hot, J['one'], chains)
        restraints = parse_restraints(a.guidance_restraints, J['one'], chains) if a.guidance_restraints else None
        ig = InterfaceGuidance(batch, w_contact=a.guidance_contact, d0=a.guidance_contact_range[0], d1=a.guidance_contact_range[1], hotspots=hot,
                               w_hot=a.guidance_hotspot_weight, restraints=restraints, scale_trans=a.guidance_scale[0], scale_rot=a.guidance_scale[1])
        return Sum(guide, ig)

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
    set_rows = []                                               # set-level mode: the rows of this rank (analyses.RowLayout)
    active = analyses.check_options(a, set_level=plan is not None)
    layout = analyses.RowLayout(analyses.fields_of(active, a), max(load_job(ji)['Lab'] for ji in range(len(jobs)))) if plan is not None else None

    def featurise(ji, ids):
        """The featurised batch of the samples `ids` of job ji on the device."""
        J = load_job(ji)
        raw = {k: v.to(dev).expand(len(ids), *v.shape[1:]).contiguous() for k, v in J['one'].items()}
        return features.build_features(raw, diffuser, generate_area=a.generate_area, opt_step=jobs[ji][3] if a.mode == 'optimize' else None,
                                       noise=features.per_sample_init_noise(ids, J['L'], a.seed, dev))

    kept = {}

    def kept_scorer(an, ji, batch=None):
        """The scorer of an analysis that runs after the gather: one per complex, from the first batch this rank sampled of it or, for a
        complex the rank did not sample, from one featurised sample (the scorer reads what all samples share)."""
        if (an.flag, ji) not in kept:
            kept[an.flag, ji] = an.build(batch if batch is not None else featurise(ji, [0]), a, model, cfg, {})
        return kept[an.flag, ji]

    kept_cons = {}

    def job_constraints(ji, batch=None):
        """The sequence constraints of job ji (None without the --seq_* options): one per complex, from the first batch this rank sampled
        of it or, for a complex the rank did not sample, from one featurised sample (the table reads what all samples share)."""
        if not constrained:
            return None
        if ji not in kept_cons:
            from .constraints import SequenceConstraints
            kept_cons[ji] = SequenceConstraints(batch if batch is not None else featurise(ji, [0]), job_chains(jobs[ji][0], jobs[ji][1]),
                                                bias_file=a.seq_bias, forbid=a.seq_forbid or (), fix=a.seq_fix or ())
        return kept_cons[ji]

    def write_sequence_table(ji, out_dir, cname, F):
        """<complex>_sequence.tsv from the gathered designs (rank 0, after write_job; nothing without the --seq_* options)."""
        if not constrained:
            return []
        return [job_constraints(ji).write_report(os.path.join(out_dir, f'{cname}_sequence.tsv'), F['seq'])]

    ref_written = set()
    for ji, ids in work:
        kind, path, out_dir, opt_step, ref_layout, ref_dir = jobs[ji]
        n = len(ids)
        t_job = time.perf_counter()
        os.makedirs(out_dir, exist_ok=True)
        J = load_job(ji)
        cname, L, Lab = J['cname'], J['L'], J['Lab']
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
                one = {k: J['one'][k].to(dev) for k in ('seq', 'atom14_gt_positions')}
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
            batch = featurise(ji, ids)
            batch['_shared_context'] = True
            diffuser.seed = a.seed
            writer = TrajectoryWriter(meta, out_dir, multi=a.mode == 'trajectory')
            scorers = {}                                        # by flag, in the order of the analyses: a later one may build on an earlier one
            for an in active:
                scorers[an.flag] = an.build(batch, a, model, cfg, scorers) if an.kw else kept_scorer(an, ji, batch)
            job_guidance = job_guide(batch, J, kind, path)
            job_cons = job_constraints(ji, batch)
            torch.cuda.synchronize()
            t_feat = time.perf_counter()
            traj = sampler.sample_fn(batch, cfg, diffuser, model, mode=a.mode, num_t=a.num_t,
                                     sample_ids=torch.tensor(ids, device=dev, dtype=torch.int64), on_record=writer.submit, guidance=job_guidance,
                                     **({'constraints': job_cons} if job_cons is not None else {}),
                                     **{an.kw: scorers[an.flag] for an in active if an.kw})
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
            local = analyses.collect(active, a, traj, scorers)
        else:                                                   # more ranks than samples: join the gather with zero-row blocks
            local = analyses.zero_rows(active, a, L, Lab, dev)
        if plan is not None:
            set_rows.append(layout.pack(ji, ids, local))
            continue
        if a.debug_one_gpu and world > 1:                       # gloo moves host tensors
            local = {k: v.cpu() for k, v in local.items()}
        res = sampler.gather_results(local, N, rank, world, group, force=a.force_collective)
        if rank == 0:                                           # (the float32 mean of every sample alone: what a set-level row carries)
            res['mean_pLDDT'] = [float(res['pLDDT'][i].float().mean()) for i in range(N)]
            files += analyses.write_job(active, a, out_dir, cname, list(range(N)), res, lambda an: kept_scorer(an, ji))
            files += write_sequence_table(ji, out_dir, cname, res)
    if plan is not None:
        # ---- the one collective of the set: every rank's rows of the designs table (counts known from the common plan)
        table = torch.cat(set_rows, 0) if set_rows else torch.zeros(0, layout.WIDTH, dtype=torch.float64)
        if not (a.debug_one_gpu and world > 1):
            table = table.to(dev)
        counts = [sum(len(ids_) for _, ids_ in p) for p in plan]
        full = sampler.gather_rows(table, counts, rank, world, group, force=a.force_collective).cpu()
        if rank == 0:
            for ji in range(len(jobs)):
                rows = full[full[:, 0] == ji]
                assert rows.shape[0] == N, (jobs[ji][1], rows.shape)
                ids_, F_ = layout.unpack(rows)
                files += analyses.write_job(active, a, jobs[ji][2], load_job(ji)['cname'], ids_, F_, lambda an: kept_scorer(an, ji))
                files += write_sequence_table(ji, jobs[ji][2], load_job(ji)['cname'], F_)
    if world > 1 or a.force_collective:
        import torch.distributed as dist
        dist.barrier()
        if a.force_collective and world == 1:
            dist.destroy_process_group()
    print(f'rank {rank}/{world}: {len(files)} files in {a.output_dir}')
    return files


if __name__ == '__main__':
    main()
