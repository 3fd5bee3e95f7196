"""ctypes binding of libabx_hip.so (C ABI declared in include/abx_hip.h).

The product path has NO fallback: if the library is missing or a call fails, an exception is raised.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# ABX_HIP_LIB: an alternative build of the same C ABI (kernel experiments under tools/probes/); the default is the in-tree library
LIB_PATH = os.environ.get('ABX_HIP_LIB') or os.path.join(_HERE, 'csrc', 'libabx_hip.so')

c_f = C.c_void_p          # device pointers travel as integers
LL = C.c_longlong
I = C.c_int
F = C.c_float


class AbxGemm(C.Structure):
    _fields_ = [
        ('A', c_f), ('sAb', LL), ('sAm', LL), ('sAk', LL),
        ('B', c_f), ('sBb', LL), ('sBk', LL), ('sBn', LL),
        ('C', c_f), ('sCb', LL), ('sCm', LL),
        ('M', I), ('N', I), ('K', I), ('batch', I),
        ('c_transposed', I),
        ('ln_stats', c_f), ('sSb', LL),
        ('ln_csum', c_f),
        ('ln_eps', F),
        ('a_relu', I),
        ('bias', c_f),
        ('alpha', F),
        ('act', I),
        ('rowscale', c_f), ('sRSb', LL),
        ('gate', c_f), ('sGb', LL), ('sGm', LL), ('gate_sigmoid', I),
        ('resid', c_f), ('sRb', LL), ('sRm', LL),
        ('B_split', C.c_void_p), ('sB3p', LL), ('sB3n', LL), ('sB3k', LL), ('sB3b', LL),
        ('A_split', C.c_void_p), ('sA3p', LL), ('sA3m', LL), ('sA3k', LL), ('sA3b', LL),
        ('batch_inner', I), ('sA3i', LL), ('sB3i', LL),
        ('c_split_tile', I),
        ('c_split_nA', I),
        ('C_split', C.c_void_p), ('sCp', LL), ('sCk', LL), ('c_split_L', I),
        ('glu', I),
        ('a_pair_transpose', I),
        ('pair_L', I), ('pair_Lp', I), ('a_pair', I), ('c_pair', I),
        ('A2', c_f), ('sA2b', LL), ('sA2m', LL), ('K2', I),
        ('B2_split', C.c_void_p), ('sB23p', LL), ('sB23n', LL), ('sB23k', LL),
        ('ln2_csum', c_f), ('bias2', c_f),
        ('mlp', I), ('N2', I),
        ('out_ln_w', c_f), ('out_ln_b', c_f), ('out_ln_eps', F),
        ('exact', I),
        ('b_f16', I), ('b_exp', I), ('b2_exp', I),
        ('tune', I),
        ('c_planes_from', I), ('c_planes_group', I),
        ('range_flag', c_f), ('range_tag', I),
        ('clock_probe', c_f),
        ('a_vec_ok', I), ('b_vec_ok', I), ('fast_ok', I),
        ('c_vec_ok', I), ('g_vec_ok', I), ('r_vec_ok', I), ('rs_vec_ok', I),
    ]


class AbxIpaTail(C.Structure):
    _fields_ = [
        ('feat', c_f), ('s_feat', LL),
        ('s', c_f), ('s_s', LL),
        ('M', I), ('K1', I), ('C', I),
        ('W_final', C.c_void_p), ('e_final', I), ('b_final', c_f),
        ('ln1_w', c_f), ('ln1_b', c_f),
        ('W_t0', C.c_void_p), ('e_t0', I), ('b_t0', c_f),
        ('W_t2', C.c_void_p), ('e_t2', I), ('b_t2', c_f),
        ('W_t4', C.c_void_p), ('e_t4', I), ('b_t4', c_f),
        ('ln2_w', c_f), ('ln2_b', c_f),
        ('ln_eps', F),
        ('W_aff', c_f), ('b_aff', c_f),
        ('fixed', c_f), ('init_q', c_f), ('init_t', c_f),
        ('cur_q', c_f), ('cur_t', c_f), ('cur_R', c_f), ('delta_q', c_f), ('pscale', F),
        ('range_flag', c_f), ('range_tag', I),
        ('partial', c_f), ('n_partial', I), ('s_partial', LL),
    ]


class AbxHeadsTail(C.Structure):
    _fields_ = [
        ('s', c_f), ('s_s', LL), ('s0', c_f), ('s_s0', LL), ('M', I),
        ('W_act', C.c_void_p), ('e_act', I), ('b_act', c_f),
        ('W_init', C.c_void_p), ('e_init', I), ('b_init', c_f),
        ('W_r0', C.c_void_p), ('e_r0', I), ('b_r0', c_f),
        ('W_r1', C.c_void_p), ('e_r1', I), ('b_r1', c_f),
        ('W_r2', C.c_void_p), ('e_r2', I), ('b_r2', c_f),
        ('W_r3', C.c_void_p), ('e_r3', I), ('b_r3', c_f),
        ('W_proj', C.c_void_p), ('e_proj', I), ('b_proj', c_f),
        ('un', c_f),
        ('lns_w', c_f), ('lns_b', c_f),
        ('W_s1', C.c_void_p), ('e_s1', I), ('b_s1', c_f),
        ('W_s3', C.c_void_p), ('e_s3', I), ('b_s3', c_f),
        ('W_s5', C.c_void_p), ('e_s5', I), ('b_s5', c_f),
        ('logits', c_f),
        ('lnp_w', c_f), ('lnp_b', c_f),
        ('W_p1', C.c_void_p), ('e_p1', I), ('b_p1', c_f),
        ('W_p3', C.c_void_p), ('e_p3', I), ('b_p3', c_f),
        ('W_p5', C.c_void_p), ('e_p5', I), ('b_p5', c_f),
        ('pl', c_f),
        ('ln_eps', F),
        ('range_flag', c_f), ('range_tag', I),
    ]


class AbxTriAttn(C.Structure):
    _fields_ = [
        ('q', c_f), ('k', c_f), ('v', c_f), ('gate', c_f),
        ('sb', LL), ('ss', LL), ('sl', LL),
        ('bias', c_f), ('bias_sb', LL), ('bias_sh', LL), ('bias_sq', LL), ('bias_sk', LL),
        ('keymask', c_f), ('km_sb', LL),
        ('out', c_f), ('ob', LL), ('os', LL), ('ol', LL),
        ('B', I), ('S', I), ('L', I), ('H', I), ('D', I),
        ('scale', F),
        ('exact', I),
        ('clock_probe', c_f),
        ('range_flag', c_f), ('range_tag', I),
        ('tune', I),
        ('bias_log2', I),
        ('kv_planes', I),
        ('q_parts', I), ('row_groups', I),
    ]


class AbxLinearPack(C.Structure):
    _fields_ = [('Wt', c_f), ('csum', c_f), ('bias', c_f), ('planes', C.c_void_p), ('b_exp', I), ('K', I), ('N', I)]


class AbxLinearSrc(C.Structure):
    _fields_ = [('W', c_f), ('b', c_f), ('rows', I), ('glu', I)]


class AbxTriMulPack(C.Structure):
    _fields_ = [('glu', AbxLinearPack), ('out', AbxLinearPack), ('gate', AbxLinearPack)]


class AbxTriRowPack(C.Structure):
    _fields_ = [('planes', C.c_void_p), ('csum', c_f), ('bias', c_f), ('b_exp', I), ('H', I)]


class AbxTriAttnPack(C.Structure):
    _fields_ = [('qkv', AbxLinearPack), ('gate', AbxLinearPack), ('pair', AbxLinearPack), ('out', AbxLinearPack), ('row', AbxTriRowPack)]


class AbxScoreArgs(C.Structure):
    _fields_ = [
        ('init_q', c_f), ('init_t', c_f), ('delta_q', c_f), ('cur_t', c_f), ('fixed_mask', c_f),
        ('t', c_f), ('t_is_f32', I),
        ('score_norms', c_f), ('num_sigma', I), ('num_omega', I), ('discrete_sigma', c_f), ('discrete_omega', c_f),
        ('exp_max_sigma', F), ('exp_min_sigma', F),
        ('min_b', F), ('bdiff', F),
        ('coord_scale', F),
        ('position_scale', F),
        ('rot_score', c_f), ('trans_score', c_f), ('rigids', c_f),
        ('B', I), ('L', I),
    ]


class AbxReverseArgs(C.Structure):
    _fields_ = [
        ('rigid_in', c_f), ('rigid_is_f64', I),
        ('seq_in', c_f),
        ('rot_score', c_f), ('trans_score', c_f), ('ts_is_f32', I), ('logits', c_f),
        ('diffuse_mask', c_f), ('t', c_f), ('dt', F),
        ('z_rot', c_f), ('z_trans', c_f), ('jumps', c_f),
        ('u_jumps', c_f),
        ('dt_dev', c_f),
        ('seed', C.c_ulonglong), ('sample_ids', c_f), ('step', I),
        ('step_dev', c_f),
        ('exp_max_sigma', F), ('exp_min_sigma', F), ('min_b', F), ('bdiff', F), ('coord_scale', F), ('rate_const', F),
        ('noise_scale', F), ('center', I),
        ('rigid_out', c_f), ('seq_out', c_f), ('rates_out', c_f), ('jumps_out', c_f),
        ('B', I), ('L', I),
        ('seq_bias', c_f),
    ]


class AbxGuidanceArgs(C.Structure):
    _fields_ = [
        ('atom14', c_f), ('atom_mask', c_f), ('aatype', c_f), ('chain_id', c_f),
        ('residx', c_f),
        ('radius', c_f), ('frame_trans', c_f),
        ('overlap_tolerance', F), ('between_chain_factor', F), ('bond_tolerance_factor', F), ('w_clash', F), ('w_bond', F), ('w_angle', F),
        ('energy', c_f), ('grad_atom', c_f), ('grad_trans', c_f), ('grad_rot', c_f),
        ('B', I), ('L', I),
    ]


class AbxContactArgs(C.Structure):
    _fields_ = [
        ('atom14', c_f), ('atom_mask', c_f),
        ('moved', c_f),
        ('target', c_f),
        ('frame_trans', c_f),
        ('hotspots', c_f), ('hotspots_host', c_f),
        ('restr_idx', c_f), ('restr_idx_host', c_f),
        ('restr_par', c_f), ('restr_par_host', c_f),
        ('w_contact', F), ('d0', F), ('d1', F), ('w_hot', F), ('d_hot', F), ('beta', F),
        ('energy', c_f), ('grad_atom', c_f), ('grad_trans', c_f), ('grad_rot', c_f),
        ('B', I), ('L', I), ('H', I), ('R', I),
    ]


# The leading fields of the five per-design analyses' descriptors (include/abx_hip.h): the structure that csrc/structure_dev.h reads
_STRUCTURE_FIELDS = [
    ('pred_atom14', c_f), ('pred_sb', LL), ('Lpred', I),
    ('pred_seq', c_f), ('pred_seq_sb', LL),
    ('pred_mask', c_f), ('res_mask', c_f),
    ('gt_atom14', c_f), ('gt_exists', c_f), ('gt_seq', c_f),
]

SCORE_COLS = 19           # ABX_SCORE_COLS


class AbxDesignScoreArgs(C.Structure):
    _fields_ = _STRUCTURE_FIELDS + [
        ('cdr_def', c_f), ('chain_id', c_f), ('residx', c_f),
        ('complex_batched', I),
        ('radius', c_f),
        ('overlap_tolerance', F), ('bond_tolerance_factor', F),
        ('out', c_f), ('out_stride', LL),
        ('B', I), ('L', I), ('Lab', I),
    ]


RELAX_COLS = 11           # ABX_RELAX_COLS


class AbxRelaxArgs(C.Structure):
    _fields_ = _STRUCTURE_FIELDS + [
        ('chain_id', c_f), ('residx', c_f), ('movable', c_f),
        ('radius', c_f), ('chi_axis', c_f), ('rigid_group', c_f),
        ('overlap_tolerance', F), ('between_chain_factor', F), ('bond_tolerance_factor', F), ('w_clash', F), ('w_bond', F), ('w_angle', F),
        ('k_restraint', F), ('eta0', F), ('rho', F), ('grow', F), ('shrink', F),
        ('max_iter', I),
        ('out_atom14', c_f), ('out_sb', LL),
        ('report', c_f), ('report_stride', LL),
        ('gen_grad', c_f),
        ('B', I), ('L', I), ('Lab', I), ('M', I),
    ]


IFACE_COLS = 12           # ABX_IFACE_COLS


class AbxInterfaceArgs(C.Structure):
    _fields_ = _STRUCTURE_FIELDS + [
        ('region', c_f),
        ('radius', c_f),
        ('sphere', c_f), ('P', I),
        ('probe', C.c_double), ('cutoff', C.c_double),
        ('out', c_f), ('out_stride', LL),
        ('points', c_f),
        ('B', I), ('L', I), ('Lab', I),
    ]


ENS_COLS = 10             # ABX_ENS_COLS
ENS_MAX_POINTS = 512      # ABX_ENS_MAX_POINTS
ENS_MAX_N = 1024          # ABX_ENS_MAX_N


class AbxEnsemblePairsArgs(C.Structure):
    _fields_ = [
        ('pred_atom14', c_f), ('pred_sb', LL), ('Lpred', I),
        ('pred_seq', c_f), ('pred_seq_sb', LL),
        ('region', c_f),
        ('atoms', I), ('M', I),
        ('planes', c_f), ('plane_stride', LL),
        ('N', I),
    ]


class AbxEnsembleClusterArgs(C.Structure):
    _fields_ = [
        ('planes', c_f), ('plane_stride', LL),
        ('metric', I),
        ('cutoff', C.c_double),
        ('out', c_f), ('out_stride', LL),
        ('centres', c_f), ('n_clusters', c_f),
        ('N', I),
    ]


DISTO_CHANNELS, DISTO_BINS, DISTO_COLS, DISTO_ROWSUMS = 192, 64, 10, 10     # ABX_DISTO_*
DISTO_ANTIBODY, DISTO_ANTIGEN, DISTO_DESIGNED = 1, 2, 4


class AbxDistogramArgs(C.Structure):
    _fields_ = [
        ('z', c_f),
        ('W', c_f), ('bias', c_f),
        ('breaks', c_f), ('sq_breaks', c_f), ('num_breaks', I),
        ('pb', c_f),
        ('classes', c_f), ('valid', c_f),
        ('cutoff', F),
        ('table', c_f), ('table_stride', LL),
        ('rows', c_f),
        ('p_contact', c_f), ('exp_dist', c_f),
        ('rowsums', c_f),
        ('B', I), ('L', I),
    ]


ACC_COLS = 21             # ABX_ACC_COLS


class AbxAccuracyArgs(C.Structure):
    _fields_ = _STRUCTURE_FIELDS + [
        ('region', c_f),
        ('radius', c_f),
        ('plddt', c_f), ('plddt_sb', LL),
        ('lddt_radius', C.c_double), ('contact', C.c_double),
        ('out', c_f), ('out_stride', LL),
        ('rows', c_f), ('counts', c_f), ('contacts', c_f),
        ('B', I), ('L', I), ('Lab', I),
    ]


POLAR_COLS = 14           # ABX_POLAR_COLS
POLAR_DONOR, POLAR_ACCEPTOR, POLAR_CATION, POLAR_ANION, POLAR_ELEMENT = 1, 2, 4, 8, 16     # ABX_POLAR_*


class AbxPolarArgs(C.Structure):
    _fields_ = _STRUCTURE_FIELDS + [
        ('region', c_f),
        ('radius', c_f),
        ('table', c_f),
        ('points', c_f), ('P', I), ('probe', C.c_double),
        ('hb_min', C.c_double), ('hb_max', C.c_double),
        ('hb_angle', C.c_double), ('hb_cos2', C.c_double),
        ('salt', C.c_double),
        ('out', c_f), ('out_stride', LL),
        ('bonds', c_f), ('rows', c_f),
        ('B', I), ('L', I), ('Lab', I),
    ]


DEV_COLS = 21             # ABX_DEV_COLS


class AbxDevelopabilityArgs(C.Structure):
    _fields_ = _STRUCTURE_FIELDS + [
        ('region', c_f),
        ('radius', c_f),
        ('chain_id', c_f), ('residx', c_f),
        ('cdr_def', c_f),
        ('q', c_f), ('q_max', LL),
        ('a', c_f), ('ref', c_f),
        ('points', c_f), ('P', I),
        ('radius2', C.c_double),
        ('exposed', C.c_double),
        ('out', c_f), ('out_stride', LL),
        ('rows', c_f),
        ('j_chunk', I),
        ('B', I), ('L', I), ('Lab', I),
    ]


SHAPE_COLS = 11           # ABX_SHAPE_COLS


class AbxShapeArgs(C.Structure):
    _fields_ = _STRUCTURE_FIELDS + [
        ('region', c_f),
        ('radius', c_f),
        ('sphere', c_f), ('P', I),
        ('points', c_f),
        ('probe', C.c_double), ('trim', C.c_double), ('weight', C.c_double),
        ('out', c_f), ('out_stride', LL),
        ('max_dots', I), ('j_chunk', I),
        ('B', I), ('L', I), ('Lab', I),
    ]


PATCH_COLS = 18           # ABX_PATCH_COLS


class AbxPatchArgs(C.Structure):
    _fields_ = _STRUCTURE_FIELDS + [
        ('region', c_f),
        ('radius', c_f),
        ('points', c_f),
        ('chain_id', c_f),
        ('cdr_def', c_f),
        ('h', c_f), ('h_max', C.c_double),
        ('q10', c_f), ('q_max', I),
        ('table', c_f),
        ('a', c_f), ('ref', c_f),
        ('cutoff2', C.c_double), ('vicinity2', C.c_double), ('salt2', C.c_double),
        ('exposed', C.c_double),
        ('out', c_f), ('out_stride', LL),
        ('rows', c_f),
        ('gly', I),
        ('B', I), ('L', I), ('Lab', I),
    ]


TORSION_COLS = 25         # ABX_TORSION_COLS
TORSION_MAX_LAB = 800     # ABX_TORSION_MAX_LAB
_PAIR = C.c_double * 2    # a (cos, sin) pair


class AbxTorsionArgs(C.Structure):
    _fields_ = _STRUCTURE_FIELDS + [
        ('region', c_f),
        ('radius', c_f),
        ('chain_id', c_f), ('residx', c_f),
        ('chi_atoms', c_f), ('chi_pi', c_f),
        ('cis', _PAIR), ('trans', _PAIR), ('o', _PAIR), ('a_mid', _PAIR), ('a_half', _PAIR), ('g_half', _PAIR), ('chi_tol', _PAIR),
        ('out', c_f), ('out_stride', LL),
        ('rows', c_f), ('classes', c_f),
        ('gly', I), ('pro', I),
        ('B', I), ('L', I), ('Lab', I),
    ]


SECONDARY_COLS = 22       # ABX_SECONDARY_COLS
SECONDARY_MAX_LAB = 800   # ABX_SECONDARY_MAX_LAB


class AbxSecondaryArgs(C.Structure):
    _fields_ = _STRUCTURE_FIELDS + [
        ('region', c_f),
        ('radius', c_f),
        ('chain_id', c_f), ('residx', c_f),
        ('hb_energy', C.c_double), ('bend', _PAIR),
        ('out', c_f), ('out_stride', LL),
        ('rows', c_f), ('classes', c_f),
        ('pro', I),
        ('B', I), ('L', I), ('Lab', I),
    ]


_S = c_f   # hipStream_t

_PROTOS = {
    'abx_version': (I, []),
    'abx_last_error_string': (C.c_char_p, []),
    'abx_init': (I, [I]),
    'abx_gemm': (I, [C.POINTER(AbxGemm), _S]),
    'abx_gemm_side': (I, [C.POINTER(AbxGemm), C.POINTER(AbxGemm), _S]),
    'abx_gemm_check_modes': (I, [C.POINTER(AbxGemm)]),
    'abx_gemm_planes_ok': (I, [LL]),
    'abx_split_weights_f16': (I, [c_f, LL, LL, I, I, I, C.c_void_p, _S]),
    'abx_ipa_tail': (I, [C.POINTER(AbxIpaTail), _S]),
    'abx_heads_tail': (I, [C.POINTER(AbxHeadsTail), _S]),
    'abx_gemm3_occupancy': (I, [I]),
    'abx_gemm_plan': (I, [C.POINTER(AbxGemm), C.POINTER(AbxGemm), C.c_char_p, I]),
    'abx_row_stats': (I, [c_f, LL, LL, LL, I, I, I, F, c_f, _S]),
    'abx_layernorm': (I, [c_f, LL, LL, I, c_f, c_f, F, c_f, LL, c_f, LL, _S]),
    'abx_tri_attn_fwd': (I, [C.POINTER(AbxTriAttn), _S]),
    'abx_tri_rowpack_bytes': (LL, []),
    'abx_tri_rowpack': (I, [C.POINTER(AbxLinearPack), c_f, C.POINTER(AbxTriRowPack), _S]),
    'abx_tri_attn_rowfused_ok': (I, [I]),
    'abx_tri_row_touch': (I, [I]),
    'abx_tri_attn_plan': (I, [C.POINTER(AbxTriAttn), I, C.c_char_p, I]),
    'abx_tri_attn_rowfused_fwd': (I, [C.POINTER(AbxTriAttn), c_f, LL, LL, LL, C.POINTER(AbxTriRowPack), I, _S]),
    'abx_seq_attn_fwd': (I, [c_f, c_f, c_f, c_f, c_f, I, I, I, I, F, _S]),
    'abx_seq_attn_plan': (I, [I, C.c_char_p, I, C.POINTER(C.c_int)]),
    'abx_ipa_pack': (I, [c_f, c_f, c_f, c_f, c_f, c_f, I, I, F, _S]),
    'abx_ipa_attn': (I, [c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_f, I, I, _S]),
    'abx_debug_poison_lds': (I, [C.c_uint, _S]),
    'abx_ipa_weights': (I, [c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_f, I, I, _S]),
    'abx_ipa_pair': (I, [c_f, c_f, c_f, I, I, _S]),
    'abx_ipa_attn_workspace_bytes': (C.c_longlong, [I, I]),
    'abx_ipa_qpack_bytes': (C.c_longlong, [I, I]),
    'abx_timestep_embedding': (I, [c_f, c_f, I, I, c_f, _S]),
    'abx_assemble_seq': (I, [c_f, LL, c_f, c_f, I, c_f, c_f, c_f, c_f, c_f, I, I, I, I, _S]),
    'abx_assemble_pair': (I, [c_f, LL, c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_f, I, I, I, I, _S]),
    'abx_opm_features': (I, [c_f, c_f, LL, c_f, I, I, I, _S]),
    'abx_opm_out_fwd': (I, [c_f, LL, c_f, c_f, c_f, I, I, c_f, I, _S]),
    'abx_assemble_pair_bias': (I, [c_f, LL, c_f, c_f, c_f, c_f, c_f, c_f, c_f, C.c_void_p, I, c_f, c_f, F, c_f, I, I, c_f, I, _S]),
    'abx_pair_mask': (I, [c_f, c_f, I, I, I, _S]),
    'abx_transpose_last2': (I, [c_f, c_f, I, I, I, I, _S]),
    'abx_pair_embed_features': (I, [c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_f, I, I, _S]),
    'abx_relpos_block': (I, [c_f, c_f, c_f, I, I, I, I, I, _S]),
    'abx_gather_rows': (I, [c_f, c_f, c_f, c_f, LL, LL, I, _S]),
    'abx_frames_init': (I, [c_f, I, c_f, c_f, c_f, c_f, c_f, c_f, I, F, _S]),
    'abx_rigid_update': (I, [c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_f, I, F, _S]),
    'abx_scores': (I, [C.POINTER(AbxScoreArgs), _S]),
    'abx_torsion_finalize': (I, [c_f, c_f, c_f, c_f, I, _S]),
    'abx_seq_head_atoms': (I, [c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_f, I, _S]),
    'abx_seq_head_atoms_biased': (I, [c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_f, I, c_f, I, _S]),
    'abx_prev_pos': (I, [c_f, c_f, I, c_f, I, I, _S]),
    'abx_plddt': (I, [c_f, c_f, I, I, _S]),
    'abx_igso3_tables': (I, [c_f, c_f, I, I, I, c_f, c_f, c_f, _S]),
    'abx_reverse_step': (I, [C.POINTER(AbxReverseArgs), _S]),
    'abx_clash_grad_workspace_bytes': (LL, [I, I]),
    'abx_clash_grad': (I, [C.POINTER(AbxGuidanceArgs), c_f, _S]),
    'abx_contact_grad_workspace_bytes': (LL, [I, I, I]),
    'abx_contact_grad': (I, [C.POINTER(AbxContactArgs), c_f, _S]),
    'abx_design_scores_workspace_bytes': (LL, [I, I]),
    'abx_design_scores': (I, [C.POINTER(AbxDesignScoreArgs), c_f, _S]),
    'abx_relax_workspace_bytes': (LL, [I, I, I]),
    'abx_relax_lds_bytes': (LL, [I, I]),
    'abx_relax': (I, [C.POINTER(AbxRelaxArgs), c_f, _S]),
    'abx_interface_scores_workspace_bytes': (LL, [I, I, I]),
    'abx_interface_scores': (I, [C.POINTER(AbxInterfaceArgs), c_f, _S]),
    'abx_ensemble_pairs_workspace_bytes': (LL, [I, I]),
    'abx_ensemble_pairs': (I, [C.POINTER(AbxEnsemblePairsArgs), c_f, _S]),
    'abx_ensemble_cluster': (I, [C.POINTER(AbxEnsembleClusterArgs), _S]),
    'abx_distogram_scores': (I, [C.POINTER(AbxDistogramArgs), _S]),
    'abx_distogram_logits': (I, [C.POINTER(AbxDistogramArgs), c_f, _S]),
    'abx_accuracy_scores_workspace_bytes': (LL, [I, I]),
    'abx_accuracy_scores': (I, [C.POINTER(AbxAccuracyArgs), c_f, _S]),
    'abx_polar_scores_workspace_bytes': (LL, [I, I]),
    'abx_polar_scores_lds_bytes': (LL, [I]),
    'abx_polar_scores': (I, [C.POINTER(AbxPolarArgs), c_f, _S]),
    'abx_developability_scores_workspace_bytes': (LL, [I, I]),
    'abx_developability_scores': (I, [C.POINTER(AbxDevelopabilityArgs), c_f, _S]),
    'abx_shape_scores_workspace_bytes': (LL, [I, I, I, I]),
    'abx_shape_scores': (I, [C.POINTER(AbxShapeArgs), c_f, _S]),
    'abx_patch_scores_workspace_bytes': (LL, [I, I, I]),
    'abx_patch_scores': (I, [C.POINTER(AbxPatchArgs), c_f, _S]),
    'abx_torsion_scores_workspace_bytes': (LL, [I, I]),
    'abx_torsion_scores': (I, [C.POINTER(AbxTorsionArgs), c_f, _S]),
    'abx_secondary_scores_workspace_bytes': (LL, [I, I]),
    'abx_secondary_scores': (I, [C.POINTER(AbxSecondaryArgs), c_f, _S]),
    'abx_pack_linear_bytes': (LL, [I, I]),
    'abx_pack_linear': (I, [C.POINTER(AbxLinearSrc), I, I, c_f, c_f, I, c_f, C.POINTER(AbxLinearPack), _S]),
    'abx_transition_workspace_bytes': (LL, [LL, I, I]),
    'abx_transition_fwd': (I, [C.POINTER(AbxLinearPack), C.POINTER(AbxLinearPack), c_f, LL, I, c_f, c_f, I, _S]),
    'abx_tri_mul_workspace_bytes': (LL, [I, I]),
    'abx_tri_mul_workspace_init': (I, [c_f, I, I, _S]),
    'abx_tri_mul_fwd': (I, [C.POINTER(AbxTriMulPack), c_f, c_f, c_f, I, I, I, c_f, c_f, I, _S]),
    'abx_tri_attn_block_workspace_bytes': (LL, [I, I]),
    'abx_tri_attn_block_fwd': (I, [C.POINTER(AbxTriAttnPack), c_f, c_f, I, I, I, I, c_f, c_f, I, _S]),
}

EXPORTED = tuple(_PROTOS)
_lib = None


class AbxHipError(RuntimeError):
    pass


def library_path():
    """Path of the shared object that load() binds (ABX_HIP_LIB or the in-tree build)."""
    return LIB_PATH


def load():
    """Load the library (raises if it has not been built: run `python -c 'import __graft_entry__ as g; g.build()'`)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise AbxHipError(f'{LIB_PATH} not found: build it with `make -C abx_amd/csrc` (no CPU fallback exists)')
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in _PROTOS.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    if lib.abx_version() != 1:
        raise AbxHipError('libabx_hip ABI version mismatch')
    _lib = lib
    return lib


def check(rc, what):
    if rc != 0:
        msg = load().abx_last_error_string()
        raise AbxHipError(f'{what} failed (rc={rc}): {msg.decode() if msg else ""}')
