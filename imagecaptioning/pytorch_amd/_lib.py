"""ctypes binding of libcapmi.so (the C ABI declared in include/capmi.h).

The product path has NO CPU fallback: if the shared object is missing or does not export a symbol
this module raises at import time (build it with ``python -m imagecaptioning.pytorch_amd.build``).
``import torch`` comes first on purpose -- torch ships its own ``libamdhip64.so.7``; loading it first
makes libcapmi resolve the same HIP runtime, so torch streams and device pointers are valid inside
our launches.
"""
import ctypes as C
import os

import torch  # noqa: F401  (must precede the CDLL: shared HIP runtime)

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('CAPMI_LIB') or os.path.join(HERE, 'libcapmi.so')   # CAPMI_LIB: experiment builds only
MAX_SEG = 4
MAX_BCOL = 3
EINVAL = -1

c_f = C.c_void_p      # device pointers travel as integers (tensor.data_ptr())


class GemmSeg(C.Structure):
    _fields_ = [('A', c_f), ('B', c_f), ('lda', C.c_int), ('ldb', C.c_int), ('K', C.c_int), ('a_row_div', C.c_int)]


class GemmDesc(C.Structure):
    _fields_ = [('seg', GemmSeg * MAX_SEG), ('nseg', C.c_int), ('a_layout', C.c_int), ('b_layout', C.c_int),
                ('M', C.c_int), ('N', C.c_int), ('C', c_f), ('ldc', C.c_int), ('bias', c_f), ('bias2', c_f),
                ('row_bias', c_f), ('row_bias_div', C.c_int), ('mul_mask', c_f), ('relu', C.c_int),
                ('accumulate', C.c_int), ('partial', c_f), ('partial_capacity', C.c_int64), ('splits', C.c_int),
                ('defer_reduce', C.c_int), ('splits_used', C.c_int), ('a_planes', c_f * MAX_SEG), ('addend', c_f),
                ('allow_wide_deferred', C.c_int), ('n_bcol', C.c_int), ('bcol_B', c_f * MAX_BCOL), ('bcol_ldb', C.c_int * MAX_BCOL),
                ('bcol_n', C.c_int * MAX_BCOL)]


class NextEmbed(C.Structure):
    """capmi_next_embed (include/capmi.h): the next step's token embedding written by the select launch"""
    _fields_ = [('E', c_f), ('mask', c_f), ('x', c_f), ('it_save', c_f), ('Edim', C.c_int), ('relu', C.c_int), ('x_planes', c_f),
                ('alive', c_f)]


class CtxStep(C.Structure):
    """capmi_ctx_step (include/capmi.h): the att2ctx stage of an AoA decode step, every decoder_type"""
    _fields_ = [(k, c_f) for k in ('slabs', 'bias', 'bias2', 'pre', 'c_prev', 'c', 'out', 'resid', 'mask_a', 'out_a', 'planes_a',
                                   'mask_b', 'out_b', 'planes_b')] + \
        [('stride', C.c_int64), ('kind', C.c_int), ('splits', C.c_int), ('M', C.c_int), ('R', C.c_int)]


CTX_GLU, CTX_RELU, CTX_LSTM = 0, 1, 2        # capmi.h CAPMI_CTX_*


class UpDownWeights(C.Structure):
    _fields_ = [(k, c_f) for k in (
        'embed', 'att_w_ih', 'att_w_hh', 'att_b_ih', 'att_b_hh', 'lang_w_ih', 'lang_w_hh', 'lang_b_ih', 'lang_b_hh',
        'h2att_w', 'h2att_b', 'alpha_w', 'alpha_b', 'logit_w', 'logit_b')]


class UpDownRollout(C.Structure):
    _fields_ = ([(k, C.c_int) for k in ('B', 'n', 'N', 'K', 'A', 'R', 'E', 'V1', 'B_feat')] + [('row_img', c_f)] +
                [(k, C.c_int) for k in ('T', 'L')] +
                [(k, c_f) for k in ('fc', 'att', 'p_att', 'att_mask', 'drop_xt', 'drop_out')] +
                [('mode', C.c_int), ('row_mode', c_f), ('temperature', C.c_float), ('gumbel', c_f),
                 ('seed', C.c_uint64), ('forced', c_f), ('forced_ld', C.c_int), ('teacher', C.c_int)] +
                [(k, c_f) for k in ('h_att', 'c_att', 'h_lang', 'c_lang', 'xt', 'it_all', 'gates_att', 'gates_lang',
                                    'att_h', 'alpha', 'ctx', 'h_drop', 'seq', 'seq_logp', 'sel_logp', 'live',
                                    'fc_gates', 'logits', 'it', 'unfinished', 'partial')] +
                [('partial_capacity', C.c_int64), ('top_k', C.c_int), ('top_p', C.c_float), ('ss_mode', c_f),
                 ('planes', c_f), ('planes_bytes', C.c_int64), ('early_exit', C.c_int), ('early_exit_from', C.c_int),
                 ('alive_host', c_f), ('steps_run', C.c_int), ('pre_partial', c_f), ('pre_capacity', C.c_int64), ('raw_logits', C.c_int)])


class SampleFilter(C.Structure):
    _fields_ = [('top_k', C.c_int), ('top_p', C.c_float)]


LP_HIST_MAX, LP_NGRAM_MAX, LP_BAD_MAX, LP_BAD_LEN = 64, 8, 16, 4      # capmi.h CAPMI_LP_*


class LogitsProc(C.Structure):
    _fields_ = [('no_repeat_ngram_size', C.c_int), ('repetition_penalty', C.c_float), ('min_length', C.c_int), ('n_bad', C.c_int),
                ('bad_len', C.c_int * LP_BAD_MAX), ('bad_words', C.c_int * (LP_BAD_MAX * LP_BAD_LEN))]


class UpDownGrads(C.Structure):
    _fields_ = [(k, c_f) for k in (
        'embed', 'att_w_ih', 'att_w_hh', 'att_b_ih', 'att_b_hh', 'lang_w_ih', 'lang_w_hh', 'lang_b_ih', 'lang_b_hh',
        'h2att_w', 'h2att_b', 'alpha_w', 'alpha_b', 'logit_w', 'logit_b', 'd_fc', 'd_att', 'd_p_att')]


class SparseLogpGrad(C.Structure):
    _fields_ = [('g_sel', c_f), ('g_sum', c_f), ('tok', c_f), ('tok_ld', C.c_int), ('raw', C.c_int), ('scale', c_f)]


class MaskDesc(C.Structure):
    _fields_ = [('mask', c_f), ('count', C.c_int64), ('offset', C.c_uint64), ('row_len', C.c_int), ('rows', C.c_int),
                ('keep_from', C.c_int)]


class ReduceItem(C.Structure):
    _fields_ = [('partial', c_f), ('C', c_f), ('bias', c_f), ('splits', C.c_int32), ('M', C.c_int32), ('N', C.c_int32),
                ('ldc', C.c_int32), ('accumulate', C.c_int32), ('reserved', C.c_int32)]


class GroupGemm(C.Structure):
    _fields_ = [('A', c_f), ('B', c_f), ('C', c_f), ('lda', C.c_int32), ('ldb', C.c_int32), ('ldc', C.c_int32), ('K', C.c_int32),
                ('M', C.c_int32), ('N', C.c_int32), ('accumulate', C.c_int32), ('splits_used', C.c_int32), ('colsum', c_f)]


class ColsumItem(C.Structure):
    _fields_ = [('in', c_f), ('out', c_f), ('out2', c_f), ('rows', C.c_int32), ('cols', C.c_int32), ('ld', C.c_int32),
                ('accumulate', C.c_int32)]


class UpDownBwdScratch(C.Structure):
    _fields_ = ([(k, c_f) for k in ('dlogits', 'd_hdrop', 'dg_att', 'dg_lang', 'd_x2', 'd_e_all', 'd_att_h_all',
                                    'dh_att_attn', 'd_x1', 'dc_att', 'dc_lang', 'd_xt_all', 'sum_dg_att', 'w_lang_cat',
                                    'w_att_cat', 'partial')] +
                [('partial_capacity', C.c_int64), ('sparse', C.POINTER(SparseLogpGrad)), ('n_grad_rows', C.c_int), ('pack', c_f),
                 ('pack_capacity', C.c_int64), ('planes', c_f), ('planes_bytes', C.c_int64)])


class UpDownBeam(C.Structure):
    _fields_ = ([(k, C.c_int) for k in ('B', 'bd', 'K', 'A', 'R', 'E', 'V1', 'L')] +
                [(k, c_f) for k in ('fc', 'att', 'p_att', 'att_mask')] + [('temperature', C.c_float), ('unk_col', C.c_int)] +
                [(k, c_f) for k in ('state', 'xt', 'gates', 'att_h', 'alpha', 'ctx', 'fc_gates', 'logits', 'it', 'sums',
                                    'logp_rows', 'parent', 'token', 'score', 'ended', 'partial')] +
                [('partial_capacity', C.c_int64)])


class UpDownBeamTrain(C.Structure):
    """capmi_updown_beam_train: the search struct + the per-step keep masks by search row"""
    _fields_ = [('b', UpDownBeam), ('drop_xt', c_f), ('drop_out', c_f), ('h_drop', c_f)]


class NewFCWeights(C.Structure):
    _fields_ = [(k, c_f) for k in ('embed', 'i2h_w', 'i2h_b', 'h2h_w', 'h2h_b', 'logit_w', 'logit_b')]


class NewFCRollout(C.Structure):
    _fields_ = ([(k, C.c_int) for k in ('B', 'n', 'N', 'R', 'E', 'V1', 'T', 'L')] + [('fc_emb', c_f), ('drop_out', c_f)] +
                [('mode', C.c_int), ('temperature', C.c_float), ('gumbel', c_f), ('seed', C.c_uint64), ('forced', c_f),
                 ('forced_ld', C.c_int), ('teacher', C.c_int)] +
                [(k, c_f) for k in ('h', 'c', 'x', 'it_all', 'saved', 'h_drop', 'seq', 'seq_logp', 'sel_logp', 'live',
                                    'logits', 'it', 'unfinished', 'partial')] + [('partial_capacity', C.c_int64), ('ss_mode', c_f)])


class NewFCGrads(C.Structure):
    _fields_ = [(k, c_f) for k in ('embed', 'i2h_w', 'i2h_b', 'h2h_w', 'h2h_b', 'logit_w', 'logit_b', 'd_fc_emb')]


class StepState(C.Structure):
    """capmi_step_state (include/capmi.h): the per-iteration record a captured training step reads from DEVICE memory"""
    _fields_ = [('epoch', C.c_uint64), ('adam_step', C.c_int32), ('lr', C.c_float), ('bc1', C.c_float), ('bc2_sqrt', C.c_float),
                ('reserved', C.c_float * 2)]


class OptimHp(C.Structure):
    """capmi_optim_hp (include/capmi.h): rule and hyper-parameters of capmi_optim_step / capmi_optim_step_dyn"""
    _fields_ = [('rule', C.c_int32), ('alpha', C.c_float), ('beta', C.c_float), ('eps', C.c_float), ('weight_decay', C.c_float),
                ('clip', C.c_float), ('grad_scale', C.c_float)]


OPTIM_RMSPROP, OPTIM_ADAGRAD, OPTIM_SGDM, OPTIM_SGDMOM, OPTIM_ADAMW = 1, 2, 3, 4, 5        # capmi.h CAPMI_OPTIM_*


class NewFCBwdScratch(C.Structure):
    _fields_ = ([(k, c_f) for k in ('dlogits', 'd_hdrop', 'd_sums', 'dh_prev', 'dc', 'd_x_all', 'd_ximg', 'partial')] +
                [('partial_capacity', C.c_int64), ('sparse', C.POINTER(SparseLogpGrad))])


class Att2in2Weights(C.Structure):
    _fields_ = [(k, c_f) for k in ('embed', 'i2h_w', 'i2h_b', 'h2h_w', 'h2h_b', 'a2c_w', 'a2c_b', 'h2att_w', 'h2att_b', 'alpha_w',
                                   'alpha_b', 'logit_w', 'logit_b')]


class Att2in2Rollout(C.Structure):
    _fields_ = ([(k, C.c_int) for k in ('B', 'n', 'N', 'K', 'A', 'R', 'E', 'V1', 'T', 'L')] +
                [(k, c_f) for k in ('att', 'p_att', 'att_mask', 'drop_xt', 'drop_out')] +
                [('mode', C.c_int), ('temperature', C.c_float), ('gumbel', c_f), ('seed', C.c_uint64), ('forced', c_f),
                 ('forced_ld', C.c_int), ('teacher', C.c_int), ('ss_mode', c_f)] +
                [(k, c_f) for k in ('h', 'c', 'x', 'it_all', 'xin', 'att_h', 'alpha', 'ctx', 'saved', 'h_drop', 'seq', 'seq_logp',
                                    'sel_logp', 'live', 'it', 'unfinished', 'partial')] + [('partial_capacity', C.c_int64)])


class Att2in2Grads(C.Structure):
    _fields_ = [(k, c_f) for k in ('embed', 'i2h_w', 'i2h_b', 'h2h_w', 'h2h_b', 'a2c_w', 'a2c_b', 'h2att_w', 'h2att_b', 'alpha_w',
                                   'alpha_b', 'logit_w', 'logit_b', 'd_att', 'd_p_att')]


class Att2in2BwdScratch(C.Structure):
    _fields_ = ([(k, c_f) for k in ('dlogits', 'd_hdrop', 'd_sums', 'd_ctx', 'd_att_h', 'd_e', 'dc', 'd_x', 'partial')] +
                [('partial_capacity', C.c_int64), ('sparse', C.POINTER(SparseLogpGrad))])


class Att2in2Step(C.Structure):
    _fields_ = ([(k, C.c_int) for k in ('B', 'K', 'A', 'R', 'E', 'V1')] +
                [(k, c_f) for k in ('att', 'p_att', 'att_mask', 'it', 'xt', 'att_h', 'alpha', 'ctx', 'saved', 'logits', 'partial')] +
                [('partial_capacity', C.c_int64)])


class TileDrop(C.Structure):
    """capmi_tile_drop (include/capmi.h): dropout of the sentinel attention's tanh tile, injected or drawn in the kernels"""
    _fields_ = [('mask', c_f), ('p', C.c_float), ('seed', C.c_uint64), ('row0', C.c_int64)]


class AdaAttWeights(C.Structure):
    _fields_ = [(k, c_f) for k in ('embed', 'xw', 'hw', 'fr_w', 'fr_b', 'ho_w', 'ho_b', 'fre_w', 'fre_b', 'hoe_w', 'hoe_b', 'alpha_w',
                                   'alpha_b', 'att2h_w', 'att2h_b', 'logit_w', 'logit_b')]


class AdaAttRollout(C.Structure):
    _fields_ = ([(k, C.c_int) for k in ('B', 'n', 'N', 'K', 'A', 'R', 'E', 'V1', 'T', 'L', 'maxout')] +
                [(k, c_f) for k in ('fc_gates', 'att', 'p_att', 'att_mask', 'drop_xt', 'drop_h', 'drop_fake', 'drop_fr', 'drop_ho',
                                    'drop_out', 'drop_tile')] +
                [('tile_p', C.c_float), ('tile_seed', C.c_uint64), ('mode', C.c_int), ('temperature', C.c_float), ('gumbel', c_f),
                 ('seed', C.c_uint64), ('forced', c_f), ('forced_ld', C.c_int), ('teacher', C.c_int), ('ss_mode', c_f)] +
                [(k, c_f) for k in ('h', 'c', 'x', 'it_all', 'xin', 'saved', 'h_drop', 'fake_drop', 'fr', 'ho_t', 'ho', 'fr_e', 'ho_e',
                                    'pi', 'ctx', 'out_t', 'out_drop', 'seq', 'seq_logp', 'sel_logp', 'live', 'it', 'unfinished',
                                    'partial')] + [('partial_capacity', C.c_int64)])


class AdaAttGrads(C.Structure):
    _fields_ = [(k, c_f) for k in ('embed', 'w2h_w', 'r_w2h_w', 'h2h_w', 'r_h2h_w', 'gate_b', 'd_fc_gates', 'fr_w', 'fr_b', 'ho_w',
                                   'ho_b', 'fre_w', 'fre_b', 'hoe_w', 'hoe_b', 'alpha_w', 'alpha_b', 'att2h_w', 'att2h_b', 'logit_w',
                                   'logit_b', 'd_att', 'd_p_att')]


class AdaAttBwdScratch(C.Structure):
    _fields_ = ([(k, c_f) for k in ('dlogits', 'd_out', 'd_ctx', 'd_e', 'd_hoe', 'd_fre', 'd_fr', 'd_ho', 'd_hdrop', 'd_fakedrop',
                                    'd_sums', 'dc', 'd_x', 'partial')] +
                [('partial_capacity', C.c_int64), ('sparse', C.POINTER(SparseLogpGrad))])


class AdaAttStep(C.Structure):
    _fields_ = ([(k, C.c_int) for k in ('B', 'K', 'A', 'R', 'E', 'V1', 'maxout')] +
                [(k, c_f) for k in ('fc_gates', 'att', 'p_att', 'att_mask', 'it', 'xt', 'saved', 'h_drop', 'fake_drop', 'fr', 'ho_t',
                                    'ho', 'fr_e', 'ho_e', 'pi', 'ctx', 'out_t', 'out_drop', 'logits', 'partial')] +
                [('partial_capacity', C.c_int64)])


ENSEMBLE_MAX = 8       # capmi.h CAPMI_ENSEMBLE_MAX


class Ensemble(C.Structure):
    """capmi_ensemble (include/capmi.h): M member rows -> their mixture log-probability"""
    _fields_ = ([(k, C.c_int) for k in ('M', 'rows', 'V1', 'ld_in', 'ld_out')] + [('in', c_f * ENSEMBLE_MAX),
                ('w', C.c_float * ENSEMBLE_MAX), ('out', c_f)])


DISC_MAX = 8           # capmi.h CAPMI_DISC_MAX
DISC_SUPPRESS, DISC_LISTENER = 0, 1


class Disc(C.Structure):
    """capmi_disc (include/capmi.h): the slot rows of B * cur hypotheses -> their pragmatic rows"""
    _fields_ = ([(k, C.c_int) for k in ('B', 'D1', 'cur', 'V1', 'ld_in', 'ld_out', 'mode')] + [('lambda', C.c_float)] +
                [(k, c_f) for k in ('in', 'present', 'out')])


class Ppo(C.Structure):
    """capmi_ppo (include/capmi.h): the PPO structure loss of one rollout, forward and backward"""
    _fields_ = ([(k, C.c_int) for k in ('N', 'L', 'V1', 'n', 'ld_new', 'ld_old', 'ld_grad', 'per_row')] +
                [('eps', C.c_float), ('kl_coef', C.c_float)] +
                [(k, c_f) for k in ('lp_new', 'lp_old', 'seq', 'scores', 'row_stats', 'msum', 'out', 'loss_rows', 'g_out', 'grad')])


class XeLoss(C.Structure):
    """capmi_xe_loss (include/capmi.h): LanguageModelCriterion / LabelSmoothing of one teacher-forced pass, forward and backward"""
    _fields_ = ([(k, C.c_int) for k in ('N', 'T', 'V1', 'tok_ld', 'mask_ld', 'per_row')] + [('smoothing', C.c_double)] +
                [(k, c_f) for k in ('logp', 'tok', 'mask', 'pos', 'msum', 'loss', 'g_out', 'g_sel', 'g_sum')])


class Distill(C.Structure):
    """capmi_distill (include/capmi.h): hard-label NLL + soft-target KL of one teacher-forced pass, forward and backward"""
    _fields_ = ([(k, C.c_int) for k in ('N', 'T', 'V1', 'ld_s', 'ld_t', 'ld_grad', 't_rows', 'tok_ld', 'mask_ld', 'per_row')] +
                [('lambda', C.c_float), ('tau', C.c_float)] +
                [(k, c_f) for k in ('lp_s', 'lp_t', 'tok', 'mask', 'row_stats', 'msum', 'out', 'loss_rows', 'g_out', 'grad')])


LANGEVAL_LMAX = 64     # capmi.h CAPMI_LANGEVAL_LMAX
CIDERD_COOKED_BYTES = 4392     # capmi.h CAPMI_CIDERD_COOKED_BYTES
SELF_CIDER_NMAX = 32   # capmi.h CAPMI_SELF_CIDER_NMAX
MBR_CIDERD, MBR_BLEU4 = 0, 1   # capmi.h CAPMI_MBR_*
LANGEVAL_E_TABLE_FULL, LANGEVAL_E_TOKEN, LANGEVAL_E_IMAGE = 1, 2, 4      # capmi.h CAPMI_LANGEVAL_E_*
DF_E_OFFSETS = 8       # capmi.h CAPMI_DF_E_OFFSETS


class LangEval(C.Structure):
    """capmi_langeval (include/capmi.h): the references of a split, their document-frequency table and the per-image results"""
    _fields_ = ([(k, C.c_int) for k in ('n_img', 'total_refs', 'ref_w')] +
                [(k, c_f) for k in ('refs', 'ref_off', 'table_keys', 'table_counts')] + [('table_cap', C.c_uint32)] +
                [(k, c_f) for k in ('ref_norm', 'cider', 'rouge', 'bleu_stats', 'lens', 'lcs', 'seen', 'err')])


DIVEVAL_NMAX, DIVEVAL_NOUT, DIVEVAL_VOCAB_WORDS = 32, 22, 2048      # capmi.h CAPMI_DIVEVAL_*


class DivEval(C.Structure):
    """capmi_diveval (include/capmi.h): n sampled captions per image on the tables of a capmi_langeval, per-image diversity results"""
    _fields_ = ([('lang', LangEval), ('n', C.c_int), ('oracle', C.c_int)] +
                [(k, c_f) for k in ('norm', 'slot_distinct', 'distinct', 'tokens', 'mbleu_stats', 'sent_bleu2', 'K', 'eig',
                                    'self_cider', 'oracle_scores', 'seen', 'err', 'vocab_bits')])


SENTSET_NCOUNT, SENTSET_NOUT = 5, 9      # capmi.h CAPMI_SENTSET_*


class SentSet(C.Structure):
    """capmi_sentset (include/capmi.h): the training and the generated sentences as sets in HBM, the counters of sentstats.py"""
    _fields_ = ([(k, C.c_int) for k in ('n_train', 'train_w', 'train_elem', 'unk_id')] + [('train_rows', c_f), ('train_table', c_f),
                ('train_cap', C.c_uint32), ('gen_capacity', C.c_int), ('gen_rows', c_f), ('gen_table', c_f), ('gen_cap', C.c_uint32),
                ('V1', C.c_int), ('vocab_bits', c_f), ('bad', c_f), ('n_bad', C.c_int), ('counts', c_f), ('sums', c_f), ('err', c_f),
                ('hash_mask', C.c_uint64)])


_I, _F, _P, _U64, _I64 = C.c_int, C.c_float, C.c_void_p, C.c_uint64, C.c_int64
DECODE_NO_REPEAT, DECODE_NO_BAD_ENDING, DECODE_BLOCK_TRIGRAMS = 1, 2, 4      # capmi.h CAPMI_DECODE_*
ROWS_L2NORM_DMAX = 8192       # capmi.h CAPMI_ROWS_L2NORM_DMAX
ROWS_F32, ROWS_BF16, ROWS_FP16 = 0, 1, 2      # capmi.h CAPMI_ROWS_*: the element format of the resident store's rows
TRUNCATE_MINP, TRUNCATE_EPS, TRUNCATE_ETA, TRUNCATE_TYP, TRUNCATE_STREAM = 0, 1, 2, 3, 256      # capmi.h CAPMI_TRUNCATE_*
CONTRASTIVE_KMAX = 32      # capmi.h CAPMI_CONTRASTIVE_KMAX
SELECT_RAW = 256       # capmi.h CAPMI_SELECT_RAW: OR into the select `mode` -- the stored rows are the logits, not the log-probabilities

# name -> argtypes (restype is always int unless noted).  Must list EVERY symbol of include/capmi.h:
# tests/test_abi.py cross-checks this table against the header and the built library.
SIGNATURES = {
    'capmi_version': [],
    'capmi_arch': [],
    'capmi_gemm_f32': [C.POINTER(GemmDesc), _P],
    'capmi_gemm_plan': [C.POINTER(GemmDesc), C.POINTER(C.c_char_p), C.POINTER(_I), C.POINTER(C.c_char_p)],
    'capmi_planes_bytes': [_I],
    'capmi_planes_from_f32': [_P, _I, _I, _I, _P, _P],
    'capmi_updown_planes_bytes': [_I, _I],
    'capmi_updown_bwd_planes_bytes': [_I],
    'capmi_attention_fwd': [_P] * 8 + [_I] * 5 + [_P, _I, _P],
    'capmi_attention_fwd_partial': [_P, _I, _I64, _P, _P] + [_P] * 7 + [_I] * 5 + [_P, _I, _P],
    'capmi_attention_fwd_partial_pl': [_P, _I, _I64, _P, _P] + [_P] * 7 + [_I] * 5 + [_P, _I, _P, _P],
    'capmi_attention_bwd': [_P, _I] + [_P] * 8 + [_I] * 5 + [_P, _I, _P],
    'capmi_attention_bwd_partial': [_P, _I, _I64, _I, _P] + [_P] * 7 + [_I] * 5 + [_P, _I, _P],
    'capmi_attention_bwd_batched': [_P, _I] + [_P] * 9 + [_I] * 7 + [_P],
    'capmi_attention_bwd_batched_ws': [_P, _I] + [_P] * 9 + [_I] * 7 + [_P, _P],
    'capmi_lstm_cell_fwd': [_P, _I, _P, _P, _P, _I, _P] + [_P] * 6 + [_I, _I, _P],
    'capmi_lstm_cell_fwd_pl': [_P, _I, _P, _P, _P, _I, _P] + [_P] * 6 + [_I, _I, _P, _P, _P],
    'capmi_lstm_cell_fwd_pl2': [_P, _I, _P, _I, _P, _P, _P, _I, _P] + [_P] * 6 + [_I, _I, _P, _P, _P],
    'capmi_lstm_cell_bwd': [_P, _I, _P, _P, _I, _P, _I] + [_P] * 6 + [_I, _I, _P],
    'capmi_lstm_cell_bwd_partial_pl': [_P, _I, _P, _P, _I, _I, _I64, _P, _I, _I, _I64] + [_P] * 6 + [_I, _I, _P, _P],
    'capmi_embed_fwd_pl': [_P, _I, _P, _P, _P, _P, _I, _I, _I, _P, _P],
    'capmi_lstm_cell_bwd_partial': [_P, _I, _P, _P, _I, _I, _I64, _P, _I, _I, _I64] + [_P] * 6 + [_I, _I, _P],
    'capmi_embed_fwd': [_P, _I, _P, _P, _P, _P, _I, _I, _I, _P],
    'capmi_embed_bwd': [_P] * 5 + [_I, _I, _I, _P],
    'capmi_logsoftmax_select': [_P, _I, _I, _I, _I, _I, _P, _F, _P, _U64, _P, _I, _I, _P, _I, _P, _P, _P, _P, _P, _P],
    'capmi_logsoftmax_select_partial': [_P, _I, _I64, _P, _I, _I, _I, _I, _I, _P, _F, _P, _U64, _P, _I, _I, _P, _I, _P, _P, _P,
                                        _P, _P, _P, _P, _P],
    'capmi_logsoftmax_select_partial_gemm': [_P, _I, _I64, _P, _I, _I, _I, _I, _I, _P, _F, _P, _U64, _P, _I, _I, _P, _I, _P, _P, _P,
                                        _P, _P, _P, _P, _P, _P],
    'capmi_logsoftmax_bwd': [_P, _P, _P, _P, _I, _I, _I, _I, _P],
    'capmi_logsoftmax_bwd_sparse': [C.POINTER(SparseLogpGrad), _P, _P, _P, _P, _I, _I, _I, _I, _P],
    'capmi_splitk_reduce': [_P, _I, _P, _I, _I, _I, _P, _P, _P, _I, _P, _I, _I, _P],
    'capmi_dropout_mask': [_P, _I64, _F, _U64, _U64, _P],
    'capmi_dropout_masks': [C.POINTER(MaskDesc), _I, _F, _U64, _P],
    'capmi_rollout_init': [_P, _P, _P, _P, _I64, _P, _P, _I, _P],
    'capmi_reward_criterion': [_P, _I, _P, _I, _P, _I, _I, _I, _I, _I, _I, _P, _P, _P],
    'capmi_colsum': [_P, _I, _I, _I, _P, _I, _P],
    'capmi_colsum_batch': [_P, _I, _P],
    'capmi_colsum_batch_args': [C.POINTER(ColsumItem), _I, _P],
    'capmi_splitk_reduce_batch': [_P, _I, _P],
    'capmi_group_rowsum': [_P, _I, _I64, _I, _I, _I, _P, _P],
    'capmi_relu_mask_bwd': [_P, _P, _P, _P, _I64, _P],
    'capmi_relu_scale_bwd': [_P, _P, _F, _P, _I64, _P],
    'capmi_adam_step': [_P, _P, _P, _P, _I64, _F, _F, _F, _F, _F, _F, _F, _I, _P],
    'capmi_upload_async': [_P, _P, _I64, _P],
    'capmi_step_advance': [_P, _F, _F, _P],
    'capmi_step_set_lr': [_P, _F, _P],
    'capmi_rng_bind_epoch': [_P, _P],
    'capmi_adam_step_dyn': [_P, _P, _P, _P, _I64, _P, _F, _F, _F, _F, _F, _F, _P],
    'capmi_optim_step': [C.POINTER(OptimHp), _P, _P, _P, _P, _I64, _F, _I, _P],
    'capmi_optim_step_dyn': [C.POINTER(OptimHp), _P, _P, _P, _P, _I64, _P, _P],
    'capmi_ema_step': [_P, _P, _I64, _F, _I, _I, _P],
    'capmi_ema_step_dyn': [_P, _P, _I64, _P, _F, _I, _P],
    'capmi_ciderd_score': [_P, _I, _I, _P, _P, _P, _I, _I, _P, _P, C.c_uint32, C.c_double, _P, _P],
    'capmi_ciderd_cook_refs': [_P, _P, _I, _I, _I, _P, _P, C.c_uint32, C.c_double, _P, _P],
    'capmi_ciderd_score_cooked': [_P, _I, _I, _P, _P, _P, _I, _P, _P, C.c_uint32, C.c_double, _P, _P],
    'capmi_scst_advantage': [_P, _I, _I, _P, _P],
    'capmi_scst_advantage_mean': [_P, _I, _I, _P, _P, _P],
    'capmi_reward_bleu4': [_P, _I, _I, _P, _P, _P, _I, _I, _I, _P, C.c_double, C.c_double, _P, _P, _P],
    'capmi_self_cider_reward': [_P, _I, _I, _I, _P, _P, C.c_uint32, C.c_double, _P, _P, _P, _P, _P, _P],
    'capmi_nsc_advantage': [_P, _P, C.c_double, _I, _I, _P, _P, _P],
    'capmi_mbr_utility': [_P, _I, _I, _I, _I, _P, _P, C.c_uint32, C.c_double, _P, _P, _P],
    'capmi_mbr_select': [_P, _P, _P, _I, _I, _I, _P, _P, _P],
    'capmi_prof_enable': [_I],
    'capmi_prof_reset': [],
    'capmi_prof_read': [_I, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_double), C.POINTER(C.c_double)],
    'capmi_beam_select': [_P, _P, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P],
    'capmi_beam_reorder': [_P, _P, _P, _I, _I, _I, _I, _I, _P],
    'capmi_beam_logsoftmax': [_P, _P, _I, _I, _F, _I, _P],
    'capmi_updown_beam_search': [C.POINTER(UpDownWeights), C.POINTER(UpDownBeam), _P],
    'capmi_updown_decode_step': [C.POINTER(UpDownWeights), C.POINTER(UpDownBeam), _I, _I, _P, _P, _I, _P],
    'capmi_updown_beam_search_train': [C.POINTER(UpDownWeights), C.POINTER(UpDownBeamTrain), _P],
    'capmi_beam_finalize': [_P, _P, _P, _P, _P, _I, _I, _I, _I, _P, _P, _P, _P, _P],
    'capmi_lineage_gather': [_P, _I, _I, _I, _P, _P, _I, _P, _P, _I, _P],
    'capmi_decode_constrain': [_P, _I, _I, _P, _I, _I, _P, _I, _P, _I, _I, _I, _P],
    'capmi_beam_diversity': [_P, _P, _I, _I, _I, _P, _I, _I, _F, _P],
    'capmi_column_penalty': [_P, _I, _I, _P, _I, _I, _F, _P],
    'capmi_logits_process': [_P, _I, _I, _I, _I, _I, C.POINTER(LogitsProc), _P, _I, _P, _P, _I, _I, _P, _I, _P],
    'capmi_select_logp': [_P, _I, _I, _I, _I, _I, _F, _P, _U64, _P, _I, _P, _P, _P, _P, _I, _P, _P],
    'capmi_truncate_rows': [_P, _I, _P, _I, _I, _I, _I, _F, _F, _P, _P, _P, _I64, _P, _P],
    'capmi_contrastive_topk': [_P, _I, _I, _I, _I, _P, _P, _P, _P, _I64, _P],
    'capmi_contrastive_select': [_P, _P, _P, _I, _P, _P, _I, _I, _I, _I, _I, _I, _I, _F, _P, _P, _P, _P, _I, _P, _P, _P],
    'capmi_layernorm_fwd': [_P] * 6 + [_I, _I, _F, _P],
    'capmi_layernorm_bwd': [_P] * 6 + [_I, _P, _I, _I, _F, _P],
    'capmi_layernorm_bwd_parts_rows': [_I],
    'capmi_layernorm_bwd_parts': [_P, _P, _P, _P, _P, _P, _I, _P, _P, _I, _I, _F, _P],
    'capmi_mha_fwd': [_P, _P, _P, _I, _I, _P, _I, _I, _I, _I, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P],
    'capmi_mha_bwd': [_P, _P, _P, _P, _I, _I, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P],
    'capmi_mha_fwd_s': [_P, _I, _P, _P, _I, _I, _P, _I, _I, _I, _I, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P],
    'capmi_mha_bwd_s': [_P, _P, _I, _P, _P, _I, _I, _P, _P, _P, _I, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P],
    'capmi_glu_fwd': [_P, _P, _P, _P, _I, _I, _P],
    'capmi_glu_fwd_fused': [_P, _I, _I64, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _P],
    'capmi_glu_bwd': [_P, _P, _P, _P, _I, _I, _P],
    'capmi_ctx_fwd_fused': [_P, _P],
    'capmi_relu_bwd_add': [_P, _P, _I, _I64, _P, _P, _P, _I, _I, _P],
    'capmi_glu_bwd_add': [_P, _P, _P, _I, _I64, _P, _P, _P, _I, _I, _P],
    'capmi_layernorm_bwd_slabs': [_P, _I, _I64, _P, _P, _P, _P, _P, _P, _I, _I64, _I, _P, _P, _I, _I, _F, _P],
    'capmi_mha_fwd_qslabs': [_P, _I, _I, _I64, _P, _P, _P, _P, _I, _I, _P, _I, _I, _I, _I, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P],
    'capmi_mha_bwd_slabs': [_P, _I, _I64, _I, _P, _I, _P, _P, _I, _I, _P, _P, _P, _I, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P],
    'capmi_gemm_group_tn': [_P, _I, _P, _I64, _P],
    'capmi_mha_plan': [_I] * 7 + [_P] * 4,
    'capmi_split_halves': [_P, _I, _I64, _P, _P, _P, _P, _I, _I, _P],
    'capmi_meanpool_fwd': [_P, _P, _P, _I, _I, _I, _P],
    'capmi_meanpool_bwd': [_P, _P, _P, _I, _I, _I, _I, _P],
    'capmi_embed_pe_fwd': [_P, _I, _P, _P, _P, _P, _I, _I, _I, _I, _P],
    'capmi_embed_pe_bwd': [_P, _I, _P, _P, _P, _I, _I, _I, _P],
    'capmi_log_softmax_rows': [_P, _P, _I, _I, _P],
    'capmi_caption_stats': [_P, _P, _I, _I, _I, _P, _P, _P, _P],
    'capmi_maxout_cell_fwd': [_P, _I] + [_P] * 8 + [_I, _I, _P],
    'capmi_maxout_cell_bwd': [_P] * 9 + [_I, _I, _P],
    'capmi_newfc_rollout_fwd': [C.POINTER(NewFCWeights), C.POINTER(NewFCRollout), _P],
    'capmi_newfc_rollout_bwd': [C.POINTER(NewFCWeights), C.POINTER(NewFCRollout), _P, C.POINTER(NewFCBwdScratch),
                                C.POINTER(NewFCGrads), _P],
    'capmi_att2in2_cell_fwd': [_P, _I, _P, _I] + [_P] * 10 + [_I, _I, _P],
    'capmi_att2in2_cell_bwd': [_P, _P, _P, _I, _I64] + [_P] * 6 + [_I, _I, _P],
    'capmi_att2in2_rollout_fwd': [C.POINTER(Att2in2Weights), C.POINTER(Att2in2Rollout), _P],
    'capmi_att2in2_rollout_bwd': [C.POINTER(Att2in2Weights), C.POINTER(Att2in2Rollout), _P, C.POINTER(Att2in2BwdScratch),
                                  C.POINTER(Att2in2Grads), _P],
    'capmi_att2in2_decode_step': [C.POINTER(Att2in2Weights), C.POINTER(Att2in2Step), _I, _I, _P, _P, _P, _P, _P],
    'capmi_sentinel_attention_fwd': [_P, _I, _I64, _P, _P, _I, _I64, _P] + [_P] * 9 + [C.POINTER(TileDrop), _P, _P] + [_I] * 5 + [_P],
    'capmi_sentinel_attention_bwd': [_P] * 8 + [C.POINTER(TileDrop)] + [_P] * 4 + [_I] * 6 + [_P],
    'capmi_sentinel_attention_bwd_batched': [_P] * 7 + [C.POINTER(TileDrop)] + [_P] * 4 + [_I] * 6 + [_P, _P],
    'capmi_adaatt_cell_fwd': [_P, _I, _P, _P, _I] + [_P] * 8 + [_I, _I, _I, _P],
    'capmi_adaatt_cell_bwd': [_P, _P, _P, _P, _P, _I, _I64] + [_P] * 6 + [_I, _I, _I, _P],
    'capmi_adaatt_rollout_fwd': [C.POINTER(AdaAttWeights), C.POINTER(AdaAttRollout), _P],
    'capmi_adaatt_rollout_bwd': [C.POINTER(AdaAttWeights), C.POINTER(AdaAttRollout), _P, C.POINTER(AdaAttBwdScratch),
                                 C.POINTER(AdaAttGrads), _P],
    'capmi_adaatt_decode_step': [C.POINTER(AdaAttWeights), C.POINTER(AdaAttStep), _I, _I, _P, _P, _P, _P, _P],
    'capmi_ensemble_logprobs': [C.POINTER(Ensemble), _P],
    'capmi_disc_combine': [C.POINTER(Disc), _P],
    'capmi_ppo_loss_fwd': [C.POINTER(Ppo), _P],
    'capmi_ppo_loss_bwd': [C.POINTER(Ppo), _P],
    'capmi_xe_loss_fwd': [C.POINTER(XeLoss), _P],
    'capmi_xe_loss_bwd': [C.POINTER(XeLoss), _P],
    'capmi_distill_loss_fwd': [C.POINTER(Distill), _P],
    'capmi_distill_loss_bwd': [C.POINTER(Distill), _P],
    'capmi_langeval_build': [C.POINTER(LangEval), _P],
    'capmi_langeval_add': [C.POINTER(LangEval), _P, _I, _I, _P, _P],
    'capmi_langeval_reduce': [C.POINTER(LangEval), _P, _P, _P],
    'capmi_diveval_add': [C.POINTER(DivEval), _P, _I, _I, _P, _P],
    'capmi_diveval_reduce': [C.POINTER(DivEval), _P, _P, _P],
    'capmi_sentset_build': [C.POINTER(SentSet), _P],
    'capmi_sentset_add': [C.POINTER(SentSet), _P, _I, _I, _I, _P],
    'capmi_sentset_add_first': [C.POINTER(SentSet), _P, _I, _I, _P, _P, _P],
    'capmi_sentset_reduce': [C.POINTER(SentSet), _P, _P],
    'capmi_df_count': [_P, _I, _I64, _P, _P, _I64, _P, _P, _I, _P, _P, C.c_uint32, _P, _P, _P],
    'capmi_df_finalize': [_P, _P, C.c_uint32, _P, _P, C.c_uint32, _P, _P],
    'capmi_updown_rollout_fwd': [C.POINTER(UpDownWeights), C.POINTER(UpDownRollout), _P],
    'capmi_updown_rollout_bwd': [C.POINTER(UpDownWeights), C.POINTER(UpDownRollout), _P, C.POINTER(UpDownBwdScratch),
                                 C.POINTER(UpDownGrads), _P],
    'capmi_updown_rollout_bwd_phases': [C.POINTER(UpDownWeights), C.POINTER(UpDownRollout), _P, C.POINTER(UpDownBwdScratch),
                                 C.POINTER(UpDownGrads), _I, _P],
    'capmi_region_rows_build': [_P, _P, _P, _P, _I, _I, _P, _I64, _I, _I, _I, _P],
    'capmi_rows_l2norm': [_P, _I64, _I, _P],
    'capmi_rows_narrow': [_P, _P, _I64, _I, _P],
    'capmi_resident_gather': [_P, _I, _I, _P, _P, _I, _I, _P, _P, _P],
    'capmi_bn_row_blocks': [_I],
    'capmi_bn_stats': [_P, _P, _I, _I, _P, _P],
    'capmi_bn_finalize': [_P, _P, _P, _I, _I, _I, _F, _F, _P, _P, _P, _P, _P, _P, _P, _P],
    'capmi_bn_apply': [_P] * 7 + [_I, _I, _P],
    'capmi_bn_bwd_partial': [_P] * 5 + [_I, _I, _P, _P],
    'capmi_bn_colsum_parts': [_P, _I, _I, _P, _P, _P],
    'capmi_bn_bwd_dx': [_P] * 9 + [_I, _P, _I, _I, _P],
    'capmi_bn_linear_bwd': [_P] * 7 + [_I, _I, _P, _P],
    'capmi_att_trace_rollout': [_P, _P, _P, _I, _I, _I, _I, _I, _P, _P],
    'capmi_att_trace_beam': [_P, _P, _P, _I, _I, _I, _I, _I, _P, _P],
    'capmi_att_ground': [_P, _I, _I, _I, _P, _I, _I, _I, _I, _P, _P, _P, _P, _P],
    'capmi_sbs_scratch_bytes': [_I, _I, _I, _I],
    'capmi_sbs_select': [_P, _P, _P, _P, _P, _U64, C.c_uint32, _I, _I, _I, _I, _I, _I, _P, _I64, _P, _P, _P, _P, _P, _P],
    'capmi_sbs_backtrack': [_P, _P, _P, _I, _I, _I, _P, _P, _P, _P],
    'capmi_cbs_scratch_bytes': [_I, _I, _I, _I],
    'capmi_cbs_select': [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P, _I64, _P, _P, _P, _P, _P, _P, _P],
    'capmi_cbs_finalize': [_P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P],
    'capmi_score_step': [_P, _I64, _I, _I, _P, _P, _P, _P, _P, _F, _I, _P],
    'capmi_retrieval_rank': [_P, _I64, _I, _I, _P, _P, _P, _P],
}


class CapmiError(RuntimeError):
    pass


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            'libcapmi.so not found at %s -- the HIP backend is mandatory (no CPU fallback). '
            'Build it: python -m imagecaptioning.pytorch_amd.build' % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    for name, argtypes in SIGNATURES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as e:  # pragma: no cover
            raise ImportError('libcapmi.so does not export %s (stale build?)' % name) from e
        fn.argtypes = argtypes
        fn.restype = (C.c_char_p if name == 'capmi_arch' else
                      C.c_int64 if name in ('capmi_planes_bytes', 'capmi_updown_planes_bytes',
                                                   'capmi_updown_bwd_planes_bytes', 'capmi_sbs_scratch_bytes',
                                                   'capmi_cbs_scratch_bytes')
                      else C.c_int)
    return lib


lib = _load()


def check(rc, what):
    if rc != 0:
        raise CapmiError('%s failed: %s' % (what, 'invalid argument' if rc == EINVAL else 'hipError %d' % rc))


def ptr(t):
    """device pointer of a tensor (None -> NULL)."""
    return None if t is None else t.data_ptr()


_raw_stream = getattr(torch._C, '_cuda_getCurrentRawStream', None)
_cur_device = getattr(torch._C, '_cuda_getDevice', None)


def stream_ptr():
    """the current HIP stream of the current device as the integer the C ABI takes.  (r4: torch.cuda.current_stream() builds a
    Stream object through three Python layers -- 4 us per launch, 3 ms of an AoA step's 744 launches; the two C entry points
    below are what it ends up calling)"""
    if _raw_stream is not None and _cur_device is not None:
        return _raw_stream(_cur_device())
    return torch.cuda.current_stream().cuda_stream
