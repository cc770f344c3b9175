#!/usr/bin/env python3
"""Generate ``tests/golden/ensemble_tiny.npz``: the REAL reference's AttEnsemble (captioning/models/AttEnsemble.py, the model of
tools/eval_ensemble.py) over the tiny members of the single-family fixtures, run on CPU.  Run only where the reference checkout
exists (never on the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_ensemble.py

The members are make_golden.family_model(<name>) -- the weights of <name>_tiny.npz, nothing new is stored -- and the inputs are
updown_tiny.npz's (fc, att, ragged att_masks, labels, masks).  The reference's AttEnsemble constructor predates three attributes its
inherited AttModel code reads (bos_idx / eos_idx / pad_idx, unk_idx, vocab); they are set on the instance here, the reference is
neither edited nor copied.  Recorded per member set (key prefix = set tag):

    tf_logp, tf_member<i>, tf_loss    teacher-forced ensemble output, each member's own log-probs, LanguageModelCriterion loss
    greedy_seq, greedy_logp           greedy decode
    b3 / b3n / b3tl                   beam 3 (sample_n 1), beam 3 with sample_n 3, beam 3 at temperature 1.3 + length_penalty wu_0.5:
                                      seq, logp and every done_beams entry's seq, p, unaug_p (make_golden._dump_beams layout)
and for the first set only: greedy with decoding_constraint + remove_bad_endings ('dc'), diverse beam search (beam 4, group 2,
'dbs'), with bad_endings_ix set by hand as in make_golden.main_opts.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF, _dump_beams, family_model      # noqa: E402

SETS = (
    # tag, members, weights
    ('ua', ('updown', 'att2in2'), (0.3, 0.7)),
    ('uta', ('updown', 'transformer', 'aoa'), (1.0, 2.0, 1.0)),
    ('nu', ('newfc', 'updown'), (1.0, 1.0)),
)


def _compat(models_pkg):
    """What make_golden.main_opts does so that the unmodified reference runs its decode options on torch >= 2: uint8 masks from
    numpy mean boolean masks inside AttModel (the torch 1.x meaning), and CaptionModel.repeat_tensor -- called by add_diversity
    but no longer defined -- is bound to models/utils.py:repeat_tensors."""
    ref_attmodel = sys.modules['captioning.models.AttModel']

    class _TorchCompat:
        def __getattr__(self, k):
            return getattr(torch, k)

        @staticmethod
        def from_numpy(a):
            x = torch.from_numpy(a)
            return x.bool() if x.dtype == torch.uint8 else x
    ref_attmodel.torch = _TorchCompat()
    ref_utils = sys.modules['captioning.models.utils']
    sys.modules['captioning.models.CaptionModel'].CaptionModel.repeat_tensor = lambda self, n, x: ref_utils.repeat_tensors(n, x)


def main():
    sys.path.insert(0, REF)
    sys.dont_write_bytecode = True
    import captioning.models as models            # noqa: E402  (the reference)
    from captioning.models.AttEnsemble import AttEnsemble
    from captioning.modules import losses
    _compat(models)
    u = np.load(os.path.join(HERE, 'updown_tiny.npz'))
    fc, att, am = (torch.from_numpy(u[k]) for k in ('fc', 'att', 'att_masks'))
    labels, masks = torch.from_numpy(u['labels']), torch.from_numpy(u['masks'])
    crit = losses.LanguageModelCriterion()
    out = {}
    for si, (tag, names, weights) in enumerate(SETS):
        members = [family_model(models, n) for n in names]
        model = AttEnsemble(members, weights=list(weights))
        model.bos_idx = model.eos_idx = model.pad_idx = 0
        model.unk_idx = None
        model.vocab = members[0].vocab
        model.eval()
        out[tag + '_weights'] = np.array(weights, dtype=np.float32)
        with torch.no_grad():
            logp = model(fc, att, labels[..., :-1], am)
            out[tag + '_tf_logp'] = logp.numpy()
            out[tag + '_tf_loss'] = crit(logp, labels[..., 1:], masks[..., 1:]).numpy()
            for i, m in enumerate(members):
                out['%s_tf_member%d' % (tag, i)] = m(fc, att, labels[..., :-1], am).numpy()
            seq, slp = model(fc, att, am, opt={'sample_method': 'greedy', 'beam_size': 1}, mode='sample')
            out[tag + '_greedy_seq'], out[tag + '_greedy_logp'] = seq.numpy(), slp.numpy()
            for btag, kw in (('b3', {}), ('b3n', {'sample_n': 3}), ('b3tl', {'temperature': 1.3, 'length_penalty': 'wu_0.5'})):
                o = {'sample_method': 'beam_search', 'beam_size': 3, 'sample_n': 1}
                o.update(kw)
                seq, slp = model(fc, att, am, opt=o, mode='sample')
                _dump_beams(model, out, '%s_%s' % (tag, btag), seq, slp)
            if si == 0:
                # bad endings by hand (the tiny vocabulary has no English words): the last word of every plain greedy caption that
                # ended, else the most frequent word of the greedy decode, so that remove_bad_endings has something to act on
                g = out[tag + '_greedy_seq']
                bad = sorted({int(r[r > 0][-1]) for r in g if 0 < (r > 0).sum() < len(r)})
                if not bad:
                    vals, cnt = np.unique(g[g > 0], return_counts=True)
                    bad = [int(vals[np.argmax(cnt)])]
                model.bad_endings_ix = bad
                out[tag + '_bad_endings_ix'] = np.array(bad, dtype=np.int64)
                seq, slp = model(fc, att, am, opt={'sample_method': 'greedy', 'beam_size': 1, 'decoding_constraint': 1,
                                                   'remove_bad_endings': 1}, mode='sample')
                out[tag + '_dc_seq'], out[tag + '_dc_logp'] = seq.numpy(), slp.numpy()
                seq, slp = model(fc, att, am, opt={'sample_method': 'beam_search', 'beam_size': 4, 'group_size': 2,
                                                   'diversity_lambda': 0.5, 'sample_n': 1}, mode='sample')
                _dump_beams(model, out, tag + '_dbs', seq, slp)
        print(tag, 'greedy', out[tag + '_greedy_seq'].tolist(), 'b3', out[tag + '_b3_seq'].tolist())
    path = os.path.join(HERE, 'ensemble_tiny.npz')
    np.savez_compressed(path, **out)
    print('ensemble_tiny.npz:', len(out), 'arrays,', os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
