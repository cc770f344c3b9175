#!/usr/bin/env python3
"""Which arm a sample call takes, what it returns and how many seeds it draws, recorded from the PARENT of the commit that moved
the five per-family `_sample` ladders into CaptionModel._sample (tests/test_sample_dispatch_gpu.py recomputes and compares).

    python tests/golden/make_sample_dispatch.py --tree PARENT_CHECKOUT [--out tests/golden/sample_dispatch.json]

--tree DIR: the checkout whose package (DIR/imagecaptioning/...) is recorded; CAPMI_LIB may point it at this tree's libcapmi, no
native source differs.  A tree that already has CaptionModel._sample is refused: the fixture is the old ladders' behaviour.

Per family (updown, newfc, att2in2, adaatt, transformer, aoa = configs/aoa.yml's switches, aoa with mean_feats 0) one model at the
smallest sizes at which the ladders can go wrong: B = 2 images (row order is image-major), K = 3 regions of which image 0 keeps two
and image 1 one (the clip to the longest mask row cuts to 2, and the rows are ragged below it), rnn / d_model 32, encoding and
att_hid 16 (adaatt: 32 throughout, its attention views its operands across the three widths), feature sizes 16, 2 heads, 1 + 1
Transformer layers of d_ff 32, V1 = 12, L = 5 (trigram blocking acts from step 3).  The vocabulary holds three of the reference's
bad endings so that remove_bad_endings acts.  Weights: tests/shapes.seeded_state.  Before each case torch.manual_seed(7),
_rng_calls = 0 and no cached decode graph.  Beam cases pass sample_n = 1, as every caller of the beam search does (the default of
10 trips AttModel._sample_beam's own assertion).

Recorded per case: the exception's class and message, or the tokens, sha256 of the bytes of seq and of the log-probabilities and
_rng_calls afterwards; and in both cases the ordered names of the leaves that ran (SPIED, wrapped not replaced).  The generator
runs every case twice: a case whose two runs differ keeps tokens and leaves only ('stable': false).
"""
import argparse
import contextlib
import functools
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
FAMILIES = ('updown', 'newfc', 'att2in2', 'adaatt', 'transformer', 'aoa', 'aoa_fc')
B, K, F, V1, L = 2, 3, 16, 12, 5
VOCAB = {str(i): w for i, w in enumerate(('a', 'the', 'of', 'w4', 'w5', 'w6', 'w7', 'w8', 'w9', 'w10', 'UNK'), start=1)}

# (name, opt, train mode with gradients enabled, CPU tensors)
CASES = [(name, opt, False, False) for name, opt in (
    ('greedy', {}),
    ('greedy_nograph', {'_graph': False}),
    ('sample', {'sample_method': 'sample', 'sample_n': 2}),
    ('gumbel', {'sample_method': 'gumbel', 'sample_n': 2}),
    ('top3', {'sample_method': 'top3', 'sample_n': 2}),
    ('top0.8', {'sample_method': 'top0.8', 'sample_n': 2}),
    ('typ0.9', {'sample_method': 'typ0.9', 'sample_n': 2}),
    ('beam2', {'beam_size': 2, 'sample_n': 1}),
    ('beam4_group2', {'beam_size': 4, 'group_size': 2, 'sample_n': 1}),
    ('beam2_decoding_constraint', {'beam_size': 2, 'sample_n': 1, 'decoding_constraint': 1}),
    ('sbs', {'sample_method': 'sbs', 'sample_n': 2}),
    ('constraints', {'constraints': [[[4]], []]}),
    ('constraints_beam2', {'constraints': [[[4]], []], 'beam_size': 2}),
    ('decoding_constraint', {'decoding_constraint': 1}),
    ('block_trigrams', {'block_trigrams': 1}),
    ('remove_bad_endings', {'remove_bad_endings': 1}),
    ('diverse_group2', {'group_size': 2, 'sample_method': 'sample'}),
    ('raw_greedy', {'output_logsoftmax': 0}),
    ('raw_sample', {'output_logsoftmax': 0, 'sample_method': 'sample', 'sample_n': 2}),
    ('raw_top3', {'output_logsoftmax': 0, 'sample_method': 'top3', 'sample_n': 2}),
    ('raw_beam2', {'output_logsoftmax': 0, 'beam_size': 2, 'sample_n': 1}),
    ('raw_decoding_constraint', {'output_logsoftmax': 0, 'decoding_constraint': 1}),
    ('attention_greedy', {'return_attention': 1}),
    ('attention_beam2', {'return_attention': 1, 'beam_size': 2, 'sample_n': 1}))]
CASES += [('cpu', {}, False, True),
          ('train_sample', {'sample_method': 'sample', 'sample_n': 2}, True, False),
          ('train_greedy', {}, True, False),
          ('train_beam2', {'beam_size': 2, 'sample_n': 1}, True, False)]

SPIED = (('beam', None, 'beam_search_steps'), ('beam', None, 'stochastic_beam_search_steps'),
         ('beam', None, 'constrained_beam_search_steps'), ('beam', None, '_native_search'), ('beam', None, 'updown_beam_train'),
         ('beam', None, 'newfc_beam_train'), ('decode', None, 'sample_steps'), ('decode', None, 'diverse_sample_steps'),
         ('engine_common', 'RolloutBase', 'run'), ('transformer_engine', None, 'sample'), ('aoa_engine', 'AoAGraph', 'rollout'),
         ('graphs', 'GraphedDecode', '__call__'))


@contextlib.contextmanager
def spies(log):
    """wrap every SPIED function so that a call appends its name to `log`, then runs the function itself"""
    import importlib
    saved = []
    for mod, cls, name in SPIED:
        owner = importlib.import_module('imagecaptioning.pytorch_amd.' + mod)
        owner = owner if cls is None else getattr(owner, cls)
        orig = getattr(owner, name)

        def wrapped(*a, _orig=orig, _label='%s.%s' % (cls or mod, name), **k):
            log.append(_label)
            return _orig(*a, **k)
        saved.append((owner, name, orig))
        setattr(owner, name, functools.wraps(orig)(wrapped))
    try:
        yield
    finally:
        for owner, name, orig in saved:
            setattr(owner, name, orig)


def build(family, dev):
    """(model on `dev`, (fc_feats, att_feats, att_masks) on the CPU)"""
    import torch
    from imagecaptioning.pytorch_amd import synthetic
    from imagecaptioning.pytorch_amd.captioning import models
    if os.path.dirname(HERE) not in sys.path:
        sys.path.insert(0, os.path.dirname(HERE))
    import shapes
    wide = 32 if family == 'adaatt' else 16
    over = dict(caption_model='aoa' if family == 'aoa_fc' else family, vocab_size=V1 - 1, vocab=dict(VOCAB), seq_length=L, max_length=L,
                rnn_size=32, input_encoding_size=wide, att_hid_size=wide, fc_feat_size=F, att_feat_size=F)
    if family == 'transformer':
        over.update(d_model=32, d_ff=32, N_enc=1, N_dec=1, num_att_heads=2, dropout=0.1)
    if family.startswith('aoa'):
        over.update(num_heads=2, multi_head_scale=1, use_multi_head=2, refine=1, refine_aoa=1, use_ff=0, decoder_type='AoA',
                    mean_feats=int(family == 'aoa'), ctx_drop=1, dropout_aoa=0.3)
    model = models.setup(synthetic.updown_opt(**over))
    model.load_state_dict(shapes.seeded_state({k: v.shape for k, v in model.state_dict().items()}, 11))
    fc, att = shapes.feats(B, K, F, seed=3)
    masks = torch.tensor([[1.0, 1.0, 0.0], [1.0, 0.0, 0.0]])
    return model.to(dev), (fc, att, masks)


def run_case(model, inputs, case, dev):
    import torch
    name, opt, train, cpu = case
    fc, att, masks = inputs if cpu else [t.to(dev) for t in inputs]
    torch.manual_seed(7)
    model._rng_calls = 0
    model.__dict__.pop('_graphs', None)
    model.train(train)
    rec, leaves = {}, []
    try:
        with spies(leaves), torch.set_grad_enabled(train):
            seq, logp = model(fc, att, masks, opt=dict(opt), mode='sample')
        seq, logp = seq.detach().cpu().contiguous(), logp.detach().cpu().contiguous()
        rec.update(tokens=seq.tolist(), seq_sha256=hashlib.sha256(seq.numpy().tobytes()).hexdigest(),
                   logp_sha256=hashlib.sha256(logp.numpy().tobytes()).hexdigest(), rng_calls=int(model._rng_calls))
    except Exception as e:      # noqa: BLE001  (a refusal is the recorded behaviour)
        if 'hipError' in str(e) or 'HIP error' in str(e):       # a device error is no refusal: nothing more runs on the device
            raise
        rec.update(error=type(e).__name__, message=str(e))
    finally:
        model.eval()
    rec['leaves'] = leaves
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--tree', required=True)
    ap.add_argument('--out', default=os.path.join(HERE, 'sample_dispatch.json'))
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    import torch
    from imagecaptioning.pytorch_amd.captioning.models.CaptionModel import CaptionModel
    if '_sample' in vars(CaptionModel):
        raise SystemExit('%s already has CaptionModel._sample: record the fixture from its parent' % args.tree)
    dev = torch.device('cuda')
    out = {}
    for family in FAMILIES:
        model, inputs = build(family, dev)
        for case in CASES:
            first, second = run_case(model, inputs, case, dev), run_case(model, inputs, case, dev)
            if first != second:
                first = {k: v for k, v in first.items() if k in ('tokens', 'error', 'message', 'leaves')}
                first['stable'] = False
                print('unstable: %s/%s' % (family, case[0]))
            out['%s/%s' % (family, case[0])] = first
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write('\n')
    print('%d cases, %d without digests' % (len(out), sum(1 for r in out.values() if r.get('stable') is False)))


if __name__ == '__main__':
    main()
