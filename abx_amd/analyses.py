"""The per-design analyses of the design driver (abx_amd.design), each stated ONCE in ANALYSES beside the writers of its tables, and
RowLayout, the columns of the row table that a set-level run gathers.  design.main walks ANALYSES in its order for the option checks,
the scorers, the keywords of sampler.sample_fn, the gathered fields (filled and zero-row blocks come from the same declarations), the
set-level rows and the files of rank 0: the next analysis is one more entry here and nothing in main."""
import functools
import math
import os
from collections import namedtuple

import numpy as np
import torch

from . import accuracy, confidence, developability, ensemble, interface, metrics, patches, polar, relax, secondary, shape, torsions
from .io import index_to_str_seq

F64 = torch.float64
# One gathered per-sample field (n, *shape).  shape: 'L' / 'Lab' stand for the lengths of the complex / of its antibody; rows: the field
# travels in the rows of a set-level run too (the others exist in sample-sharded runs only: 8 L^2 or 32 L bytes a sample).
Field = namedtuple('Field', 'name dtype shape rows')
# One analysis.  flag: the option that switches it on; kw: the keyword its scorer is passed to sampler.sample_fn under (None: the
# analysis runs after the gather, on the rank that writes, with one scorer per complex); build(batch, a, model, cfg, scorers) -> the
# scorer (scorers: those of the analyses before it, by flag); fields(a) -> [Field]; collect(a, traj, scorers) -> {field: tensor} of a
# sampled batch; write(a, out_dir, cname, ids, F, scorer) -> the files of one complex from the gathered fields F, rows in the order of
# the sample ids; checks: (bad(a), the SystemExit text) pairs; extra: its --<flag>_rows / _planes option, whose field is not one of rows.
Analysis = namedtuple('Analysis', 'flag kw build fields collect write checks extra', defaults=((), None))
HEAD = (Field('seq', torch.int64, ('Lab',), True), Field('pLDDT', torch.float32, ('Lab',), False))


def block_shape(field, L, Lab):
    return tuple({'L': L, 'Lab': Lab}.get(s, s) for s in field.shape)


def _save(out_dir, cname, end, array):
    np.save(os.path.join(out_dir, f'{cname}_{end}.npy'), array)
    return os.path.join(out_dir, f'{cname}_{end}.npy')


# --score: metrics.SCORE_COLUMNS of every record as it is made (metrics.DesignScorer): further columns of <complex>_designs.tsv and, in
# trajectory mode, <complex>_trajectory_scores.tsv with one line per sample and record.
def _score_fields(a):
    NS, n_rec = len(metrics.SCORE_COLUMNS), a.num_t if a.mode == 'trajectory' else 0
    return [Field('scores', F64, (NS,), True)] + ([Field('traj_scores', F64, (n_rec, 1 + NS), True)] if n_rec else [])


def _score_collect(a, traj, scorers):
    s = traj[-1]['scores']
    if a.mode != 'trajectory' or not a.num_t:
        return {'scores': s}                                    # traj_scores (samples, records, 1 + columns): t, then the scores of the record
    return {'scores': s, 'traj_scores': torch.stack([torch.cat([s.new_full((s.shape[0], 1), r['time']), r['scores']], 1) for r in traj], 1)}


def _write_designs(out_dir, cname, rows):
    """<out_dir>/<complex>_designs.tsv: (sample id, mean pLDDT, designed antibody sequence) per sample; with --score a row carries
    a fourth entry, its metrics.SCORE_COLUMNS values, written as further columns."""
    tsv = os.path.join(out_dir, f'{cname}_designs.tsv')
    scored = bool(rows) and len(rows[0]) > 3
    with open(tsv, 'w') as f:
        f.write('sample\tmean_pLDDT\tantibody_sequence' + ('\t' + '\t'.join(metrics.SCORE_COLUMNS) if scored else '') + '\n')
        for i, pl, toks, *sc in rows:
            f.write(f'{i}\t{pl:.3f}\t{index_to_str_seq(toks)}' + ('\t' + '\t'.join(metrics.format_scores(sc[0])) if scored else '') + '\n')
    return tsv


def _write_trajectory_scores(out_dir, cname, table):
    """<out_dir>/<complex>_trajectory_scores.tsv: one line per (sample, record of the trajectory).  table (samples, records, 1 + columns):
    t of the record, then its metrics.SCORE_COLUMNS values."""
    tsv = os.path.join(out_dir, f'{cname}_trajectory_scores.tsv')
    with open(tsv, 'w') as f:
        f.write('sample\tstep\tt\t' + '\t'.join(metrics.SCORE_COLUMNS) + '\n')
        for i, recs in enumerate(table.tolist()):
            for k, r in enumerate(recs):
                f.write(f'{i}\t{k}\t{r[0]:.4f}\t' + '\t'.join(metrics.format_scores(r[1:])) + '\n')
    return tsv


SCORE = Analysis('score', 'scorer', lambda batch, *_: metrics.DesignScorer(batch), _score_fields, _score_collect,
                 lambda a, out_dir, cname, ids, F, scorer: [_write_trajectory_scores(out_dir, cname, F['traj_scores'].cpu())] if 'traj_scores' in F else [])


# --relax: every design is relaxed after the last step (relax.ViolationRelaxer): <name>_relaxed.pdb beside every design (upstream's
# naming, which its eval_metric.py skips), <complex>_relax.tsv with relax.RELAX_COLUMNS and, with --score, the scores of the relaxed
# structure, and in the wild tables below the columns of the relaxed structure, suffixed _relaxed (nan on the wild line).
def _write_relax(out_dir, cname, rows, scored):
    """<out_dir>/<complex>_relax.tsv: (sample id, values) per sample; values = the relax.RELAX_COLUMNS report and, when scored, the
    metrics.SCORE_COLUMNS of the relaxed structure."""
    NR = len(relax.RELAX_COLUMNS)
    tsv = os.path.join(out_dir, f'{cname}_relax.tsv')
    with open(tsv, 'w') as f:
        f.write('sample\t' + '\t'.join(relax.RELAX_COLUMNS + (metrics.SCORE_COLUMNS if scored else ())) + '\n')
        for i, v in rows:
            f.write(f'{i}\t' + '\t'.join(relax.format_report(v[:NR]) + (metrics.format_scores(v[NR:]) if scored else [])) + '\n')
    return tsv


RELAX = Analysis('relax', 'relaxer', lambda batch, a, *_: relax.ViolationRelaxer(batch, flank=a.relax_flank, max_iter=a.relax_iters, k_restraint=a.relax_restraint),
                 lambda a: [Field('relax', F64, (len(relax.RELAX_COLUMNS) + (len(metrics.SCORE_COLUMNS) if a.score else 0),), True)],
                 lambda a, traj, scorers: {'relax': torch.cat([traj[-1]['relax']] + ([traj[-1]['scores_relaxed']] if a.score else []), 1)},
                 lambda a, out_dir, cname, ids, F, scorer: [_write_relax(out_dir, cname, list(zip(ids, F['relax'].tolist())), a.score)])


def _write_with_wild_deltas(kind, out_dir, cname, wild, rows, relaxed, strings=None, text=None):
    """<out_dir>/<complex>_<kind>.tsv of the analysis module abx_amd.<kind> (interface, polar, confidence, developability, shape, patches,
    torsions, secondary): the `wild` line, then (sample id, values) per sample; values = the module's <KIND>_COLUMNS row and, when
    relaxed, the row of the relaxed structure.  After the columns: delta_<column> = row minus wild for the module's DELTA_COLUMNS, then
    the _relaxed columns.  wild None: every sample has a wild row of its own, the last columns of its values, and the `wild` line is
    their mean.  text: the name of a last column of strings; strings = (the wild type's string, [the string of every sample]); None: '-'."""
    mod = {'interface': interface, 'polar': polar, 'confidence': confidence, 'developability': developability, 'shape': shape, 'patches': patches,
           'torsions': torsions, 'secondary': secondary}[kind]
    columns, fmt = getattr(mod, f'{kind.upper()}_COLUMNS'), getattr(mod, f'format_{kind}')
    N = len(columns)
    wilds = [wild if wild is not None else v[len(v) - N:] for _, v in rows]
    if wild is None:
        wild = [sum(w[k] for w in wilds) / max(len(wilds), 1) for k in range(N)]
    wild_s, row_s = strings if strings is not None else ('-', ['-'] * len(rows))
    last = (lambda s: [s]) if text else (lambda s: [])
    tsv = os.path.join(out_dir, f'{cname}_{kind}.tsv')
    with open(tsv, 'w') as f:
        f.write('sample\t' + '\t'.join(list(columns) + ['delta_' + c for c in mod.DELTA_COLUMNS] +
                                       ([c + '_relaxed' for c in columns] if relaxed else []) + last(text)) + '\n')
        f.write('wild\t' + '\t'.join(fmt(wild) + mod.format_delta(wild, wild) + (['nan'] * N if relaxed else []) + last(wild_s)) + '\n')
        for (i, v), w, st in zip(rows, wilds, row_s):
            f.write(f'{i}\t' + '\t'.join(fmt(v[:N]) + mod.format_delta(v[:N], w) + (fmt(v[N:2 * N]) if relaxed else []) + last(st)) + '\n')
    return tsv


# What --<flag>_rows / _planes adds to a wild table.  of_record: last record -> the field; to_array: gathered field -> <complex>_<field>.npy
Extra = namedtuple('Extra', 'option field of_record to_array')
# The text column of a wild table: the class string of the designed residues.  field: the name of a second gathered field (n, 3, Lab)
# int32 - the codes of the design, those of the wild type and the region mask, so that any rank can write the column on both schedules
# (it travels in the rows like `seq`); string(classes, region) -> the text of a line.  The sampler's record carries <flag>_classes, the
# scorer has new_classes(1) and wild(classes=).
Text = namedtuple('Text', 'field string')


def _wild_table(flag, columns, writer, build, wild, checks, extra=None, text=None):
    """An analysis whose <complex>_<flag>.tsv compares every design with a wild row.  Its field is the design's row, with --relax the
    relaxed structure's, then the wild row, so that any rank can write the table: (n, 2 or 3 x columns).  wild(last, scorers) -> the
    wild row(s): (1, columns) of the complex, or (n, columns), one per sample (with a Text: unused, the wild row comes with the wild
    type's classes); writer(out_dir, cname, wild of row 0, rows, relaxed), with a Text one argument more, the strings."""
    def fields(a):
        return [Field(flag, F64, (len(columns) * (3 if a.relax else 2),), True)] + ([Field(text.field, torch.int32, (3, 'Lab'), True)] if text else []) + \
            ([extra.field] if extra and getattr(a, extra.option) else [])

    def collect(a, traj, scorers):
        last, n = traj[-1], traj[-1]['seq'].shape[0]
        if text:
            sc = scorers[flag]
            wild_classes = sc.new_classes(1)
            w = sc.wild(classes=wild_classes)
        else:
            w = wild(last, scorers)
        out = {flag: torch.cat([last[flag]] + ([last[flag + '_relaxed']] if a.relax else []) + [w.expand(n, -1)], 1)}
        if text:
            out[text.field] = torch.stack([last[flag + '_classes'], wild_classes.expand(n, -1), sc.region[None, :sc.Lab].to(torch.int32).expand(n, -1)], 1)
        if extra and getattr(a, extra.option):
            out[extra.field.name] = extra.of_record(last)
        return out

    def write(a, out_dir, cname, ids, F, scorer):
        t, strings = F[flag].tolist(), []
        if text:
            ab = F[text.field].cpu().numpy()
            strings = [(text.string(ab[0, 1], ab[0, 2]), [text.string(r[0], r[2]) for r in ab])]
        files = [writer(out_dir, cname, t[0][-len(columns):], list(zip(ids, t)), a.relax, *strings)]
        if extra and getattr(a, extra.option):
            files.append(_save(out_dir, cname, extra.field.name, extra.to_array(F[extra.field.name])))
        return files
    return Analysis(flag, flag, build, fields, collect, write, checks, extra and extra.option)


def _build(make, rows_option=None):
    """build of an analysis from make(batch, a, the interface scorer of the batch or None) -> the scorer; rows_option: the --<flag>_rows
    option that sets its want_rows."""
    def build(batch, a, model, cfg, scorers):
        sc = make(batch, a, scorers.get('interface'))
        if rows_option:
            sc.want_rows = getattr(a, rows_option)
        return sc
    return build


_write_interface = functools.partial(_write_with_wild_deltas, 'interface')
INTERFACE = _wild_table('interface', interface.INTERFACE_COLUMNS, _write_interface,
                        lambda batch, a, *_: interface.InterfaceScorer(batch, n_points=a.interface_points, probe=a.interface_probe, cutoff=a.interface_cutoff),
                        lambda last, scorers: scorers['interface'].wild(points=_shared_wild_points(scorers)),
                        [(lambda a: not 1 <= a.interface_points <= 1024 or a.interface_probe < 0 or a.interface_cutoff <= 0,
                          '--interface_points must be in 1..1024, --interface_probe >= 0, --interface_cutoff > 0')])


# The analyses on the point counts of the interface analysis (the interface.SurfaceScorer classes: polar, developability, shape,
# patches) are coupled to --interface in three places: with --interface the scorer is built on THAT InterfaceScorer and the surface kernel
# runs once per structure set for all tables (sampler.sample_fn hands the counts over); one buffer of counts serves all wild rows
# (_shared_wild_points); and without --interface each validates the options of the surface, --interface_points and --interface_probe,
# itself (SURFACE_CHECK).
SURFACE_CHECK = (lambda a: not 1 <= a.interface_points <= 1024 or a.interface_probe < 0, '--interface_points must be in 1..1024, --interface_probe >= 0')
SURFACE_FLAGS = []


def _surface_table(flag, columns, writer, make, check, extra=None):
    """_wild_table of an analysis whose scorer make(batch, a, interface) is a SurfaceScorer; check: of its own options."""
    SURFACE_FLAGS.append(flag)
    return _wild_table(flag, columns, writer, _build(make, extra and extra.option),
                       lambda last, scorers: scorers[flag].wild(points=_shared_wild_points(scorers)), [check, SURFACE_CHECK], extra)


def _shared_wild_points(scorers):
    """A surface analysis with --interface: the (1, L, 14, 2) point counts of the wild type that interface.wild() fills and the wild()
    of every SurfaceScorer reads instead of running the surface kernel again, kept with the scorers of the batch; None without
    --interface or without any of them."""
    users = [scorers[k] for k in SURFACE_FLAGS if k in scorers]
    if users and 'interface' in scorers and 'wild_points' not in scorers:
        scorers['wild_points'] = users[0].new_points(1)
    return scorers.get('wild_points')


# --confidence: every sample carries a wild row of its own, the input complex's coordinates under the SAME design's prediction; the
# `wild` line of the table is their mean.
def _confidence_build(batch, a, model, cfg, scorers):
    conf = confidence.DistogramScorer(batch, model, cutoff=a.confidence_cutoff, conf=cfg.model.heads.distogram)
    conf.want_planes = a.confidence_planes
    return conf


def _write_confidence(out_dir, cname, rows, relaxed):
    return _write_with_wild_deltas('confidence', out_dir, cname, None, rows, relaxed)


CONFIDENCE = _wild_table('confidence', confidence.CONFIDENCE_COLUMNS, lambda out_dir, cname, wild, *rest: _write_confidence(out_dir, cname, *rest), _confidence_build,
                         lambda last, scorers: last['confidence_wild'], [(lambda a: not a.confidence_cutoff > 0, '--confidence_cutoff must be > 0')],
                         Extra('confidence_planes', Field('confidence_contacts', torch.float32, ('L', 'L'), False),
                               lambda last: last['confidence_planes'][0], lambda t: t.double().mean(0).float().cpu().numpy()))


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


ACCURACY = _wild_table('accuracy', accuracy.ACCURACY_COLUMNS, _write_accuracy,
                       lambda batch, a, *_: accuracy.AccuracyScorer(batch, radius=a.accuracy_radius, contact=a.accuracy_contact),
                       lambda last, scorers: scorers['accuracy'].wild(),
                       [(lambda a: not a.accuracy_radius > 0 or not a.accuracy_contact > 0, '--accuracy_radius and --accuracy_contact must be > 0')],
                       Extra('accuracy_rows', Field('accuracy_rows', F64, ('L', 4), False), lambda last: last['accuracy_rows'], lambda t: t.cpu().numpy()))


# --polar: hydrogen bonds and salt bridges across the interface; the unsatisfied atoms come from the point counts of the interface analysis.
_write_polar = functools.partial(_write_with_wild_deltas, 'polar')
POLAR = _surface_table('polar', polar.POLAR_COLUMNS, _write_polar,
                       lambda batch, a, it: polar.PolarScorer(batch, hb_max=a.polar_hb_max, hb_angle=a.polar_hb_angle, salt=a.polar_salt,
                                                              n_points=a.interface_points, probe=a.interface_probe, interface=it),
                       (lambda a: not a.polar_hb_max >= 2.0 or not 90.0 <= a.polar_hb_angle < 180.0 or not a.polar_salt >= 0,
                        '--polar_hb_max must be >= 2.0 (the smallest donor-acceptor distance), --polar_hb_angle in [90, 180), --polar_salt >= 0'),
                       Extra('polar_rows', Field('polar_rows', torch.int32, ('L', 4), False), lambda last: last['polar_rows'],
                             lambda t: t.cpu().numpy().astype('int16')))


# --ensemble: the designs of a complex compared with each other (ensemble.EnsembleAnalyzer) by the rank that writes, after the gather: the
# backbone of the antibody travels with the other fields.  <complex>_ensemble.tsv; --ensemble_matrix: <complex>_ensemble_rmsd.npy, the
# (3, N, N) planes rmsd_fit, rmsd_frame, seq_diff.  With --relax the analysis still describes the designs as written.
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


def _ensemble_write(a, out_dir, cname, ids, F, an):
    """The ensemble tables from the gathered tokens (N, Lab) and backbone (N, Lab, 4, 3); an: the EnsembleAnalyzer of the complex."""
    dev = an.region.device
    x = torch.zeros(F['seq'].shape[0], an.Lab, 14, 3, dtype=torch.float32, device=dev)
    x[:, :, :4] = F['backbone'].to(dev)
    res = an.analyze(x, F['seq'].to(dev).long())
    table = res['table'].cpu().numpy()
    centres = res['centres'].cpu().tolist()[:int(res['n_clusters'])]
    files = [_write_ensemble(out_dir, cname, ensemble.summary(table, an.n_region), list(zip(ids, table.tolist())), centres)]
    return files + ([_save(out_dir, cname, 'ensemble_rmsd', res['planes'].cpu().numpy())] if a.ensemble_matrix else [])


ENSEMBLE = Analysis('ensemble', None, lambda batch, a, *_: ensemble.EnsembleAnalyzer(batch, atoms=a.ensemble_atoms, metric=a.ensemble_metric, cutoff=a.ensemble_cutoff),
                    lambda a: [Field('backbone', torch.float32, ('Lab', 4, 3), True)],      # N, CA, C, O of the antibody rows: what the comparison reads
                    lambda a, traj, scorers: {'backbone': traj[-1]['atom14_results'][:, :, :4].float().contiguous()}, _ensemble_write,
                    [(lambda a: not 1 <= a.num_samples <= ensemble.MAX_N or not a.ensemble_cutoff >= 0,
                      f'--ensemble compares 1..{ensemble.MAX_N} samples of a complex, --ensemble_cutoff must be >= 0')])

# --developability: aggregation propensity, chain charges and sequence liabilities of the free antibody; its exposure comes from the point
# counts of the interface analysis.
_write_developability = functools.partial(_write_with_wild_deltas, 'developability')
DEVELOPABILITY = _surface_table('developability', developability.DEVELOPABILITY_COLUMNS, _write_developability,
                                lambda batch, a, it: developability.DevelopabilityScorer(batch, radius=a.developability_radius, exposed=a.developability_exposed,
                                                                                         n_points=a.interface_points, probe=a.interface_probe, interface=it),
                                (lambda a: not a.developability_radius > 0 or not 0.0 <= a.developability_exposed <= 1.0,
                                 '--developability_radius must be > 0, --developability_exposed in [0, 1]'),
                                Extra('developability_rows', Field('developability_rows', F64, ('L', 4), False), lambda last: last['developability_rows'],
                                      lambda t: t.cpu().numpy()))


# --shape: the shape complementarity Sc of the interface; its dots are the sphere points of the interface analysis.  A row of -1 says
# that a dot list outgrew --shape_max_dots: no table is written with such a row.
def _write_shape(out_dir, cname, wild, rows, relaxed):
    """_write_with_wild_deltas('shape', ...); a row of -1 (its dot count is negative) ends the run by the name of the option to raise."""
    N = len(shape.SHAPE_COLUMNS)
    written = [wild] + [v[:N] for _, v in rows] + ([v[N:2 * N] for _, v in rows] if relaxed else [])
    if any(r[6] < 0 for r in written):
        raise SystemExit(f'--shape: a dot list of {cname} outgrew --shape_max_dots (a row of -1): raise --shape_max_dots')
    return _write_with_wild_deltas('shape', out_dir, cname, wild, rows, relaxed)


SHAPE = _surface_table('shape', shape.SHAPE_COLUMNS, _write_shape,
                       lambda batch, a, it: shape.ShapeScorer(batch, trim=a.shape_trim, weight=a.shape_weight, n_points=a.interface_points,
                                                              probe=a.interface_probe, max_dots=a.shape_max_dots, interface=it),
                       (lambda a: not a.shape_trim >= 0 or not a.shape_weight >= 0 or not a.shape_max_dots >= 1,
                        '--shape_trim must be >= 0, --shape_weight >= 0, --shape_max_dots >= 1'))


# --patches: the patches of surface hydrophobicity and of charge around the CDRs, the charge symmetry of the Fv and the charge pairing
# across the interface; its exposure comes from the point counts of the interface analysis.
_write_patches = functools.partial(_write_with_wild_deltas, 'patches')
PATCHES = _surface_table('patches', patches.PATCHES_COLUMNS, _write_patches,
                         lambda batch, a, it: patches.PatchScorer(batch, cutoff=a.patches_cutoff, vicinity=a.patches_vicinity, salt=a.patches_salt,
                                                                  exposed=a.patches_exposed, n_points=a.interface_points, probe=a.interface_probe, interface=it),
                         (lambda a: not a.patches_cutoff > 0 or not a.patches_vicinity > 0 or not a.patches_salt > 0 or not 0.0 <= a.patches_exposed <= 1.0,
                          '--patches_cutoff, --patches_vicinity and --patches_salt must be > 0, --patches_exposed in [0, 1]'),
                         Extra('patches_rows', Field('patches_rows', F64, ('L', 4), False), lambda last: last['patches_rows'], lambda t: t.cpu().numpy()))


# --torsions: cis and twisted peptides, phi >= 0, the ABEGO classes and the chi recovery of the designs; the text column is `abego`.
_write_torsions = functools.partial(_write_with_wild_deltas, 'torsions', text='abego')
TORSIONS = _wild_table('torsions', torsions.TORSIONS_COLUMNS, _write_torsions,
                       _build(lambda batch, a, it: torsions.TorsionScorer(batch, chi_tol=a.torsions_chi_tol), 'torsions_rows'), None,
                       [(lambda a: not 0.0 < a.torsions_chi_tol <= 180.0, '--torsions_chi_tol must be in (0, 180] degrees')],
                       Extra('torsions_rows', Field('torsions_rows', F64, ('Lab', 8), False), lambda last: last['torsions_rows'], lambda t: t.cpu().numpy()),
                       Text('torsions_abego', torsions.abego_string))

# --secondary: DSSP's backbone hydrogen bonds, bridges and states of the antibody against the crystal structure; the text column is
# `dssp`, the state string of the designed residues.
_write_secondary = functools.partial(_write_with_wild_deltas, 'secondary', text='dssp')
SECONDARY = _wild_table('secondary', secondary.SECONDARY_COLUMNS, _write_secondary,
                        _build(lambda batch, a, it: secondary.SecondaryScorer(batch, hb_energy=a.secondary_hb_energy), 'secondary_rows'), None,
                        [(lambda a: not (math.isfinite(a.secondary_hb_energy) and a.secondary_hb_energy < 0.0),
                          '--secondary_hb_energy must be a finite energy below 0 kcal/mol')],
                        Extra('secondary_rows', Field('secondary_rows', torch.int32, ('Lab', 6), False), lambda last: last['secondary_rows'],
                              lambda t: t.cpu().numpy()),
                        Text('secondary_ss', secondary.ss_string))

# Every analysis, in the order they are walked: it fixes the order of the gathered fields and of the collectives.  The next analysis is
# appended here.
ANALYSES = (SCORE, RELAX, INTERFACE, CONFIDENCE, ACCURACY, POLAR, ENSEMBLE, DEVELOPABILITY, SHAPE, PATCHES, TORSIONS, SECONDARY)


def check_options(a, set_level):
    """The analyses that the parsed options `a` switch on, in order, after their option checks.  set_level: the run gathers rows."""
    active = []
    for an in ANALYSES:
        if getattr(a, an.flag):
            for bad, text in an.checks:
                if bad(a):
                    raise SystemExit(text)
            if an.extra and getattr(a, an.extra) and set_level:
                raise SystemExit(f'--{an.extra} needs the sample-sharded schedule (--shard_samples): a set-level run gathers one table only')
            active.append(an)
        elif an.extra and getattr(a, an.extra):
            raise SystemExit(f'--{an.extra} needs --{an.flag}')
    return active


def fields_of(active, a):
    return list(HEAD) + [f for an in active for f in an.fields(a)]


def collect(active, a, traj, scorers):
    """The fields of a sampled batch, keyed and ordered as declared (one gather per field, in this order on every rank)."""
    got = {'seq': traj[-1]['seq'], 'pLDDT': traj[-1]['pLDDT']}
    for an in active:
        got.update(an.collect(a, traj, scorers))
    assert list(got) == [f.name for f in fields_of(active, a)], list(got)
    return got


def zero_rows(active, a, L, Lab, device):
    """The block of a rank without samples of a complex: it still joins the gather."""
    return {f.name: torch.zeros(0, *block_shape(f, L, Lab), dtype=f.dtype, device=device) for f in fields_of(active, a)}


class RowLayout:
    """Columns of the (n, WIDTH) float64 row table of a set-level run: job, sample id, mean pLDDT, Lab, then one span per field that
    travels in rows, wide enough for the longest antibody of the set (maxLab) and filled up to the job's own Lab.  Every value is exact
    in float64: tokens, float32 coordinates, and the float32 mean of pLDDT that the sample-sharded path prints too."""
    def __init__(self, fields, maxLab):
        self.fields, self.spans, c = [f for f in fields if f.rows], {}, 4
        for f in self.fields:
            self.spans[f.name] = (c, c + math.prod(block_shape(f, 0, maxLab)))
            c = self.spans[f.name][1]
        self.WIDTH = c

    def pack(self, ji, ids, local):
        """The rows of the samples `ids` of job ji from their fields (on any device) -> (n, WIDTH) on the host."""
        n, Lab = local['seq'].shape
        rows = torch.zeros(n, self.WIDTH, dtype=F64)
        rows[:, 0], rows[:, 1], rows[:, 3] = ji, torch.tensor(ids, dtype=F64), Lab
        rows[:, 2] = local['pLDDT'].float().mean(1).double().cpu()
        for f in self.fields:
            v = local[f.name].reshape(n, -1).double().cpu()
            rows[:, self.spans[f.name][0]:self.spans[f.name][0] + v.shape[1]] = v
        return rows

    def unpack(self, rows):
        """The rows of ONE job in any order -> (sample ids, {field: (n, ...)}) in the order of the sample ids, 'mean_pLDDT' for 'pLDDT'."""
        rows = rows[torch.argsort(rows[:, 1])]
        n, Lab = rows.shape[0], int(rows[0, 3])
        F = {'mean_pLDDT': rows[:, 2]}
        for f in self.fields:
            shape, c = block_shape(f, 0, Lab), self.spans[f.name][0]
            F[f.name] = rows[:, c:c + math.prod(shape)].to(f.dtype).reshape(n, *shape)
        return [int(i) for i in rows[:, 1]], F


def write_job(active, a, out_dir, cname, ids, F, kept_scorer):
    """The tables of one complex from the form both schedules end in: the sample ids and the gathered fields F = {name: (n, ...)} in their
    order, 'mean_pLDDT' (n) among them.  kept_scorer(an): the per-complex scorer of an analysis that runs after the gather."""
    sc = F['scores'].tolist() if 'scores' in F else None
    files = [_write_designs(out_dir, cname, [(i, float(pl), toks) + ((sc[k],) if sc else ()) for k, (i, pl, toks) in
                                             enumerate(zip(ids, F['mean_pLDDT'], F['seq'].tolist()))])]
    for an in active:
        files += an.write(a, out_dir, cname, ids, F, kept_scorer(an) if an.kw is None else None)
    return files
