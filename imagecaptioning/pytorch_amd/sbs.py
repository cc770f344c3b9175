"""Stochastic beam search: ``opt['sample_method'] = 'sbs'`` with ``opt['sample_n'] = k`` decodes k DISTINCT captions per image, drawn
without replacement from the model (Kool, van Hoof and Welling 2019, "Stochastic Beams and Where to Find Them").  The search is
beam.stochastic_beam_search_steps on the kernels of csrc/sbs.hip; this module holds the option checks and the importance weights.

After such a call ``model.last_sbs = {'phi', 'g', 'log_w'}``, each [B, k] on the device, rows in the order of the returned captions
(descending g):

    phi     log p(y_i): the caption's joint log-probability (at opt['temperature'], under the decoding constraints)
    g       its perturbed log-probability G_phi_i; the k captions are the k largest over all sequences
    log_w   the normalised importance weights of the paper's estimator (eqs. 15, 19), for sum_i w_i f(y_i) ~ E_p[f]:
                kappa = g[:, k - 1]                                   the k-th largest perturbed value, the threshold
                q_i   = 1 - exp(-exp(phi_i - kappa))                  P(G_phi_i > kappa)
                w_i   = exp(phi_i) / q_i            for i < k - 1
                log_w = log w_i - log sum_j w_j;    the k-th caption is spent on the threshold: log_w = -inf
              k = 1: the one caption is an exact sample, log_w = 0.  k = 2 leaves one weighted caption, log_w = (0, -inf).
"""
import torch

K_MAX = 16            # BD_MAX of csrc/search_common.h


def wanted(opt):
    return bool(opt) and opt.get('sample_method', 'greedy') == 'sbs'


def log_weights(phi, g):
    """phi, g [B, k] (g descending) -> log_w [B, k] float64, see the module docstring"""
    phi, g = phi.double(), g.double()
    k = phi.shape[1]
    if k == 1:
        return torch.zeros_like(phi)
    kappa = g[:, k - 1:k]
    # log q = log(1 - exp(-e)), e = exp(phi - kappa) > 0: log(-expm1(-e)), stable for small and large e
    log_q = torch.log(-torch.expm1(-torch.exp(phi[:, :k - 1] - kappa)))
    log_w = phi[:, :k - 1] - log_q
    log_w = log_w - torch.logsumexp(log_w, 1, keepdim=True)
    return torch.cat([log_w, log_w.new_full((phi.shape[0], 1), float('-inf'))], 1)


def check_options(model, opt):
    """the refusals of a sample call with sample_method 'sbs', before any device work -> k"""
    if getattr(model, '_sbs_refusal', None) is not None:
        raise NotImplementedError("sample_method 'sbs' is not implemented for %s: %s" % (type(model).__name__, model._sbs_refusal))
    if model.training:
        raise NotImplementedError("sample_method 'sbs' is a test-time option: call model.eval() first")
    if opt.get('block_trigrams', 0):
        raise NotImplementedError("sample_method 'sbs' does not support block_trigrams: the blocking reads a hypothesis's whole "
                                  'history, which a beam keeps as parent pointers until the search has ended')
    if int(opt.get('group_size', 1)) > 1:
        raise NotImplementedError("sample_method 'sbs' does not support group_size > 1: the captions of one search are already "
                                  'distinct, and penalising groups against each other would end the sampling without replacement')
    if not opt.get('output_logsoftmax', 1):
        raise NotImplementedError("output_logsoftmax=0 is implemented for the sampled / greedy rollout; sample_method 'sbs' "
                                  'returns log-probabilities')
    k = int(opt.get('sample_n', 1))
    if not 1 <= k <= K_MAX:
        raise ValueError("sample_method 'sbs' draws the sample_n captions of an image in one search: 1 <= sample_n <= %d, got %d"
                         % (K_MAX, k))
    if not float(opt.get('temperature', 1.0)) > 0:
        raise ValueError("sample_method 'sbs' needs temperature > 0, got %r" % (opt.get('temperature'),))
    return k
