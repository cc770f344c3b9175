"""Test-time ensembles on the MI355X: capmi_ensemble_logprobs against fp64, degenerate ensembles against their member, AttEnsemble
against the reference's recorded ensembles (tests/golden/make_ensemble.py), the UpDown config size, tools/eval_ensemble.py."""
import argparse
import ctypes as C
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from test_model_api_gpu import tiny_opt, DEV

pytestmark = pytest.mark.gpu

FAMILIES = ('updown', 'newfc', 'att2in2', 'transformer', 'aoa')
Z = os.path.join(GOLDEN, 'ensemble_tiny.npz')
MEMBERS = {'ua': ('updown', 'att2in2'), 'uta': ('updown', 'transformer', 'aoa'), 'nu': ('newfc', 'updown')}   # make_ensemble.SETS


def mixture64(xs, w):
    w = torch.tensor(w, dtype=torch.float64, device=xs[0].device)
    w = w / w.sum()
    return sum(wi * torch.softmax(x.double(), -1) for wi, x in zip(w, xs)).log()


# ---------------------------------------------------------------------------------------------------------------- the kernel
@pytest.mark.parametrize('M', (1, 2, 3, 8))
@pytest.mark.parametrize('V1', (1, 3, 31, 9487, 9488))
def test_kernel_against_fp64(M, V1):
    from imagecaptioning.pytorch_amd import ops
    from imagecaptioning.pytorch_amd._lib import lib, ptr, stream_ptr
    g = torch.Generator(device=DEV).manual_seed(M * 100003 + V1)
    for rows in (1, 37, 1000):
        w = [0.5 + i for i in range(M)]
        if M > 1:
            w[1] = 0.0                                                     # a member with weight 0 is not read
        base = [4 * torch.randn(rows, V1, generator=g, device=DEV) for _ in range(M)]
        for kind in ('logits', 'logprobs', 'offset'):
            if kind == 'logits':
                xs = base
            elif kind == 'logprobs':
                xs = [torch.log_softmax(x, -1) for x in base]
            else:                                                          # +-1e4: the normalisation must not lose digits
                xs = [x + (1e4 if i % 2 else -1e4) for i, x in enumerate(base)]
            ref = mixture64(xs, w)             # (of the fp32 inputs as given: x + 1e4 itself keeps only ~1e-3 of x)
            live = ref > -60
            out = ops.ensemble_logprobs(xs, w)
            torch.cuda.synchronize()
            assert torch.isfinite(out).all(), (rows, kind)
            err = float((out.double() - ref)[live].abs().max())
            assert err <= 2e-5, (rows, kind, err)
        if M == 1:
            ls = torch.empty_like(base[0])
            assert lib.capmi_log_softmax_rows(ptr(base[0]), ptr(ls), rows, V1, stream_ptr()) == 0
            assert float((ops.ensemble_logprobs(base, None) - ls).abs().max()) <= 2e-5


def test_kernel_edge_cases_and_layouts():
    from imagecaptioning.pytorch_amd import ops, _lib
    from imagecaptioning.pytorch_amd._lib import lib, CapmiError
    V1 = 103
    a, b = torch.randn(5, V1, device=DEV), torch.randn(5, V1, device=DEV)
    a[0, 7] = b[0, 7] = float('-inf')                                       # -inf in every member: -inf
    a[1, 9] = float('-inf')                                                 # -inf in one member only: finite
    b[2, 11] = float('nan')                                                 # NaN propagates (the row's normaliser too)
    out = ops.ensemble_logprobs([a, b], [1, 1])
    ref = mixture64([a, b], [1, 1])
    assert out[0, 7] == float('-inf') and torch.isfinite(out[0, :7]).all() and torch.isfinite(out[1]).all()
    assert torch.isnan(out[2]).all()
    assert float((out[[0, 1, 3, 4]].double() - ref[[0, 1, 3, 4]]).nan_to_num(0, 0, 0).abs().max()) < 2e-5
    # a weight-0 member may hold anything
    junk = torch.full_like(a, float('nan'))
    assert float((ops.ensemble_logprobs([a, junk], [1, 0])[3:] - torch.log_softmax(a, -1)[3:]).abs().max()) < 2e-5
    # strided rows, members at different alignments (scalar path) and a misaligned output
    big = torch.randn(3, 40, V1 + 7, device=DEV)
    xs = [big[0, :, 1:V1 + 1], big[1, :, 2:V1 + 2], big[2, :, 0:V1]]
    obig = torch.zeros(40, V1 + 5, device=DEV)
    out = ops.ensemble_logprobs(xs, [1, 2, 3], out=obig[:, 3:V1 + 3])
    assert float((out.double() - mixture64(xs, [1, 2, 3])).abs().max()) < 2e-5
    assert (obig[:, :3] == 0).all() and (obig[:, V1 + 3:] == 0).all()
    xs = [big[0, :, 1:V1 + 1], big[1, :, 1:V1 + 1]]                          # same alignment, rows not 16-byte aligned
    assert float((ops.ensemble_logprobs(xs, None).double() - mixture64(xs, [1, 1])).abs().max()) < 2e-5
    # the C entry point's own checks
    e = _lib.Ensemble()
    e.M, e.rows, e.V1, e.ld_in, e.ld_out = 2, 5, V1, V1, V1
    getattr(e, 'in')[0], getattr(e, 'in')[1] = a.data_ptr(), b.data_ptr()
    e.w[0], e.w[1] = 0.5, 0.5
    o = torch.empty_like(a)
    e.out = o.data_ptr()
    st = torch.cuda.current_stream().cuda_stream
    assert lib.capmi_ensemble_logprobs(C.byref(e), st) == 0
    for field, val in (('M', 0), ('M', 9), ('V1', 0), ('ld_in', V1 - 1), ('ld_out', V1 - 1)):
        bad = _lib.Ensemble.from_buffer_copy(e)
        setattr(bad, field, val)
        assert lib.capmi_ensemble_logprobs(C.byref(bad), st) == _lib.EINVAL, field
    bad = _lib.Ensemble.from_buffer_copy(e)
    bad.w[0] = -1.0
    assert lib.capmi_ensemble_logprobs(C.byref(bad), st) == _lib.EINVAL
    bad = _lib.Ensemble.from_buffer_copy(e)
    bad.w[0] = bad.w[1] = 0.0
    assert lib.capmi_ensemble_logprobs(C.byref(bad), st) == _lib.EINVAL
    bad = _lib.Ensemble.from_buffer_copy(e)
    bad.out = a.data_ptr()                                                   # aliases an input
    assert lib.capmi_ensemble_logprobs(C.byref(bad), st) == _lib.EINVAL
    zero = _lib.Ensemble.from_buffer_copy(e)
    zero.rows = 0
    assert lib.capmi_ensemble_logprobs(C.byref(zero), st) == 0
    assert ops.ensemble_logprobs([a[:0], b[:0]]).shape == (0, V1)
    with pytest.raises(CapmiError):
        ops.ensemble_logprobs([a, b], [1, 1], out=a)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------- models
def family_model(name):
    """the tiny model of tests/golden/<name>_tiny.npz (make_golden.family_model on this backend)"""
    from imagecaptioning.pytorch_amd.captioning import models
    z = np.load(os.path.join(GOLDEN, name + '_tiny.npz'))
    if name == 'transformer':
        opt = tiny_opt(caption_model='transformer', N_enc=2, N_dec=2, d_model=16, d_ff=32, num_att_heads=2, dropout=0.0)
    elif name == 'aoa':
        opt = tiny_opt(caption_model='aoa', refine=1, refine_aoa=1, use_ff=0, decoder_type='AoA', use_multi_head=2, num_heads=2,
                       multi_head_scale=1, mean_feats=1, ctx_drop=1, dropout_aoa=0.3, num_layers=2)
    else:
        opt = tiny_opt(caption_model=name)
    model = models.setup(opt)
    model.load_state_dict({k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith('P.')})
    return model.to(DEV).eval()


def inputs():
    u = np.load(os.path.join(GOLDEN, 'updown_tiny.npz'))
    fc, att, am, labels, masks = (torch.from_numpy(u[k]).to(DEV) for k in ('fc', 'att', 'att_masks', 'labels', 'masks'))
    return fc, att, am, labels, masks


def ensemble(names, weights=None):
    from imagecaptioning.pytorch_amd.captioning.models import AttEnsemble
    return AttEnsemble([family_model(n) for n in names], weights=weights).to(DEV).eval()


@pytest.mark.parametrize('name', FAMILIES)
def test_one_member_ensemble_is_its_member(name):
    fc, att, am, _, _ = inputs()
    model = family_model(name)
    ens = ensemble([name])
    with torch.no_grad():
        for o in ({'sample_method': 'greedy', 'beam_size': 1}, {'sample_method': 'beam_search', 'beam_size': 3, 'sample_n': 1}):
            seq, slp = model(fc, att, am, opt=dict(o), mode='sample')
            eseq, eslp = ens(fc, att, am, opt=dict(o), mode='sample')
            assert torch.equal(seq, eseq), (name, o)
            assert float((slp - eslp).abs().max()) <= 2e-5, (name, o)


def test_same_model_three_times_is_that_model():
    fc, att, am, labels, _ = inputs()
    model = family_model('updown')
    from imagecaptioning.pytorch_amd.captioning.models import AttEnsemble
    ens = AttEnsemble([model, model, model], weights=[1, 2, 3]).eval()
    with torch.no_grad():
        for o in ({'sample_method': 'greedy'}, {'sample_method': 'beam_search', 'beam_size': 3, 'sample_n': 1}):
            seq, slp = model(fc, att, am, opt=dict(o), mode='sample')
            eseq, eslp = ens(fc, att, am, opt=dict(o), mode='sample')
            assert torch.equal(seq, eseq)
            assert float((slp - eslp).abs().max()) <= 2e-5
        own = model(fc, att, labels[..., :-1], am)
        mix = ens(fc, att, labels[..., :-1], am)
    assert float((own - mix).abs().max()) <= 2e-5


# ---------------------------------------------------------------------------------------------------------------- the reference
def _close(got, want, what):
    np.testing.assert_allclose(got, want, rtol=1e-5, atol=1e-5, err_msg=what)


def _check_beams(model, z, tag, seq, slp):
    assert np.array_equal(seq.cpu().numpy(), z[tag + '_seq']), tag
    _close(slp.cpu().numpy(), z[tag + '_logp'], tag)
    for k, beams in enumerate(model.done_beams):
        assert len(beams) == int(z['%s_n%d' % (tag, k)]), (tag, k)
        for j, bm in enumerate(beams):
            assert np.array_equal(bm['seq'].cpu().numpy(), z['%s_%d_%d_seq' % (tag, k, j)]), (tag, k, j)
            _close(bm['p'], z['%s_%d_%d_p' % (tag, k, j)], (tag, k, j))
            _close(bm['unaug_p'], z['%s_%d_%d_unaug' % (tag, k, j)], (tag, k, j))


@pytest.mark.parametrize('tag', sorted(MEMBERS))
def test_reference_ensemble_fixture(tag):
    from imagecaptioning.pytorch_amd.captioning.modules import losses
    z = np.load(Z)
    fc, att, am, labels, masks = inputs()
    model = ensemble(MEMBERS[tag], weights=z[tag + '_weights'].tolist())
    with torch.no_grad():
        logp = model(fc, att, labels[..., :-1], am)
        loss = losses.LanguageModelCriterion()(logp, labels[..., 1:], masks[..., 1:])
        want = z[tag + '_tf_logp']
        got = logp.cpu().numpy()
        N, T = got.shape[:2]
        zero = (want == 0).all(-1)
        assert (got[zero] == 0).all()
        live = ~zero
        if 'transformer' in MEMBERS[tag]:
            # the reference steps the Transformer with a causal mask only, its own forward also masks input pads: positions after
            # the end of a caption (loss mask 0) differ, see test_ensemble_host
            inp = labels[..., :-1].reshape(N, -1).cpu()
            live &= torch.stack([(inp[:, 1:t + 1] != 0).all(1) for t in range(T)], 1).numpy()
        _close(got[live], want[live], 'tf_logp')
        assert abs(float(loss) - float(z[tag + '_tf_loss'])) <= 1e-5
        seq, slp = model(fc, att, am, opt={'sample_method': 'greedy', 'beam_size': 1}, mode='sample')
        assert np.array_equal(seq.cpu().numpy(), z[tag + '_greedy_seq'])
        _close(slp.cpu().numpy(), z[tag + '_greedy_logp'], 'greedy')
        for btag, kw in (('b3', {}), ('b3n', {'sample_n': 3}), ('b3tl', {'temperature': 1.3, 'length_penalty': 'wu_0.5'})):
            o = {'sample_method': 'beam_search', 'beam_size': 3, 'sample_n': 1}
            o.update(kw)
            seq, slp = model(fc, att, am, opt=o, mode='sample')
            _check_beams(model, z, '%s_%s' % (tag, btag), seq, slp)
        if tag + '_bad_endings_ix' in z.files:
            model.bad_endings_ix = z[tag + '_bad_endings_ix'].tolist()
            seq, slp = model(fc, att, am, opt={'sample_method': 'greedy', 'beam_size': 1, 'decoding_constraint': 1,
                                               'remove_bad_endings': 1}, mode='sample')
            assert np.array_equal(seq.cpu().numpy(), z[tag + '_dc_seq'])
            got, want = slp.cpu().numpy(), z[tag + '_dc_logp']
            assert np.array_equal(np.isneginf(got), np.isneginf(want))
            _close(got, want, 'dc')
            seq, slp = model(fc, att, am, opt={'sample_method': 'beam_search', 'beam_size': 4, 'group_size': 2,
                                               'diversity_lambda': 0.5, 'sample_n': 1}, mode='sample')
            _check_beams(model, z, tag + '_dbs', seq, slp)


def test_get_logprobs_state_steps_the_mixture():
    """AttEnsemble.py:45-53 driven from outside (UpDown + Att2in2, the families with get_logprobs_state): one step from BOS is the
    mixture of the members' own first steps; a member without the API is named."""
    from imagecaptioning.pytorch_amd.captioning.models import AttEnsemble
    fc, att, am, _, _ = inputs()
    a, b = family_model('updown'), family_model('att2in2')
    ens = AttEnsemble([a, b], weights=[0.3, 0.7]).eval()
    with torch.no_grad():
        feats = ens._prepare_feature(fc, att, am)
        state = ens.init_hidden(fc.shape[0])
        it = torch.zeros(fc.shape[0], dtype=torch.long, device=DEV)
        lp, st = ens.get_logprobs_state(it, *feats, state)
        la, _ = a.get_logprobs_state(it, *[f[0] for f in feats], a.init_hidden(fc.shape[0]))
        lb, _ = b.get_logprobs_state(it, *[f[1] for f in feats], b.init_hidden(fc.shape[0]))
        assert float((lp.double() - mixture64([la, lb], [0.3, 0.7])).abs().max()) < 2e-5
        assert len(st) == 4
        lp2, _ = ens.get_logprobs_state(lp.argmax(1), *feats, st)
        assert torch.isfinite(lp2).all()
    with pytest.raises(NotImplementedError, match='TransformerModel'):
        with torch.no_grad():
            AttEnsemble([a, family_model('transformer')]).eval().get_logprobs_state(it, *feats, state)


# ---------------------------------------------------------------------------------------------------------------- config size
def test_updown_config_size_ensemble():
    from imagecaptioning.pytorch_amd.captioning import models
    from imagecaptioning.pytorch_amd.captioning.models import AttEnsemble
    from imagecaptioning.pytorch_amd.captioning.utils import opts
    torch.manual_seed(7)
    opt = opts.parse_opt(['--caption_model', 'updown'])
    opt.vocab = {str(i): 'w%d' % i for i in range(1, opt.vocab_size + 1)}
    a, b = models.setup(opt).to(DEV), models.setup(opt).to(DEV)
    b.load_state_dict(a.state_dict())
    with torch.no_grad():
        for p in b.parameters():
            p.add_(0.02 * torch.randn_like(p))
    B, K, n, T = 10, 36, 5, 17
    fc = torch.randn(B, opt.fc_feat_size, device=DEV).clamp_min(0)
    att = torch.randn(B, K, opt.att_feat_size, device=DEV).clamp_min(0)
    seq = torch.randint(1, opt.vocab_size + 1, (B, n, T), device=DEV)
    seq[..., 0] = 0
    seq[..., 12:] = 0
    ens = AttEnsemble([a, b], weights=[0.4, 0.6]).eval()
    assert ens.vocab_size + 1 == 9488
    with torch.no_grad():
        own = [m.eval()._forward(fc, att, seq, None) for m in (a, b)]
        mix = ens(fc, att, seq, None)
        ref = mixture64(own, [0.4, 0.6])
        ref[:, 12:] = 0
        live = ref > -60
        assert float((mix.double() - ref)[live].abs().max()) <= 2e-5
        assert (mix[:, 12:] == 0).all()
        s, lp = ens(fc, att, None, opt={'sample_method': 'beam_search', 'beam_size': 5, 'sample_n': 1}, mode='sample')
    assert s.shape == (B, opt.max_length) and torch.isfinite(lp).all()


# ---------------------------------------------------------------------------------------------------------------- the CLI
def test_eval_ensemble_cli(tmp_path):
    from imagecaptioning.pytorch_amd.captioning import models
    from imagecaptioning.pytorch_amd.captioning.models import AttEnsemble
    from imagecaptioning.pytorch_amd.captioning.modules import losses
    from imagecaptioning.pytorch_amd.captioning.utils import misc, opts
    from imagecaptioning.pytorch_amd.captioning.data.synthetic_loader import SyntheticLoader
    from imagecaptioning.pytorch_amd.tools import eval_ensemble as EE
    tiny = ['--rnn_size', '16', '--input_encoding_size', '16', '--att_hid_size', '12', '--fc_feat_size', '20', '--att_feat_size',
            '20', '--vocab_size', '30', '--seq_length', '8', '--max_length', '8', '--synthetic_regions', '6', '--batch_size', '4',
            '--seq_per_img', '2', '--synthetic_images', '8', '--drop_prob_lm', '0.0']
    torch.manual_seed(3)
    built = []
    for id_, cm, suffix in (('a', 'updown', ''), ('b', 'att2in2', 'best')):
        opt = opts.parse_opt(tiny + ['--caption_model', cm, '--id', id_, '--checkpoint_path', str(tmp_path / ('log_' + id_))])
        loader = SyntheticLoader(opt)
        opt.vocab = loader.get_vocab()
        m = models.setup(opt)
        with torch.no_grad():
            for p in m.parameters():
                p.add_(0.3 * torch.randn_like(p))
        misc.save_checkpoint(opt, m, {'opt': opt, 'vocab': opt.vocab}, append=suffix)
        built.append(m.to(DEV).eval())
    loss, preds = EE.main(['--ids', 'a', 'b-best', '--weights', '0.5', '0.5', '--log_root', str(tmp_path), '--num_images', '4',
                           '--beam_size', '2', '--split', 'val'])
    assert len(preds) == 4 and len({p['image_id'] for p in preds}) == 4
    # the loss is the criterion over the teacher-forced ensemble on the same batch
    opt = opts.parse_opt(tiny + ['--caption_model', 'updown'])
    data = SyntheticLoader(opt).get_batch('val')
    fc, att, labels, masks = (data[k].to(DEV) for k in ('fc_feats', 'att_feats', 'labels', 'masks'))
    am = None if data.get('att_masks') is None else data['att_masks'].to(DEV)
    ens = AttEnsemble(built, weights=[0.5, 0.5]).eval()
    with torch.no_grad():
        want = losses.LanguageModelCriterion()(ens(fc, att, labels[..., :-1], am), labels[..., 1:], masks[..., 1:])
    assert abs(loss - float(want)) < 1e-6, (loss, float(want))
