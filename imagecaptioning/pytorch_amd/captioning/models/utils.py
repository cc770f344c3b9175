"""captioning/models/utils.py of the reference (3-24): B -> B*n row expansion helpers.

The HIP kernels never need the expanded copies (they index ``row // n``); these exist for API
parity with callers that expand tensors themselves (beam search, ensembles)."""
import torch


from imagecaptioning.pytorch_amd.ops import clip_len      # noqa: F401  (clip_att's K, cached on the mask)


def repeat_tensors(n, x):
    """[B, ...] -> [B*n, ...], rows of one image adjacent (reference: models/utils.py:3-14)."""
    if torch.is_tensor(x):
        return x.repeat_interleave(n, dim=0)
    if isinstance(x, (list, tuple)):
        return [repeat_tensors(n, v) for v in x]
    return x


def split_tensors(n, x):
    """inverse grouping (reference: models/utils.py:17-24)."""
    if torch.is_tensor(x):
        assert x.shape[0] % n == 0
        return x.reshape(x.shape[0] // n, n, *x.shape[1:]).unbind(1)
    if isinstance(x, (list, tuple)):
        return [split_tensors(n, v) for v in x]
    if x is None:
        return [None] * n
    return x


# the truncation samplers beyond top-k / nucleus: spelling -> (rule, range of its parameter, upper bound included?)
TRUNCATION_RULES = {'minp': ('minp', '0 < a <= 1', True), 'eps': ('eps', '0 < e < 1', False), 'eta': ('eta', '0 < e < 1', False),
                    'typ': ('typ', '0 < tau < 1', False)}


def parse_truncation(sample_method):
    """'minp<a>' / 'eps<e>' / 'eta<e>' / 'typ<tau>' -> (rule, parameter): min-p, epsilon, eta and locally typical sampling
    (capmi_truncate_rows, include/capmi.h).  None for every other name; ValueError for a parameter outside the rule's range."""
    if not isinstance(sample_method, str):
        return None
    for prefix, (kind, rng, closed) in TRUNCATION_RULES.items():
        if sample_method.startswith(prefix):
            try:
                num = float(sample_method[len(prefix):])
            except ValueError:
                return None
            if not (0 < num < 1 or (closed and num == 1)):
                raise ValueError('sample_method %r: the parameter of %s must satisfy %s' % (sample_method, kind, rng))
            return kind, num
    return None


def parse_sample_method(sample_method, temperature):
    """CaptionModel.sample_next_word (CaptionModel.py:370-407) -> (kernel mode, temperature, top_k, top_p).
    'gumbel': arg-max of (logp + Gumbel) / T is a categorical draw from softmax(logp) -- the temperature cancels in the
    arg-max -- i.e. the 'sample' kernel at temperature 1.  'top<k>' keeps the k most probable tokens, 'top<p>' (0<p<1)
    the nucleus of softmax(logp / T).  The truncation rules of parse_truncation are plain sampling here: the rule itself runs
    in front of the token choice (decode.sample_steps)."""
    if parse_truncation(sample_method) is not None:
        return 'sample', temperature, 0, 0.0
    if sample_method == 'greedy':
        return 'greedy', temperature, 0, 0.0
    if sample_method == 'sample':
        return 'sample', temperature, 0, 0.0
    if sample_method == 'gumbel':
        return 'sample', 1.0, 0, 0.0
    if sample_method.startswith('top'):
        num = float(sample_method[3:])
        return ('sample', temperature, 0, num) if 0 < num < 1 else ('sample', temperature, int(num), 0.0)
    raise NotImplementedError('sample_method %r' % sample_method)
