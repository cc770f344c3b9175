"""Per-word region attention (opt['return_attention'], att_trace.py, tools/eval.py --dump_attention) without a GPU: the option, the
refusals, the C ABI of the three new entries, and the float64 helper against the reference fixture."""
import argparse
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, GOLDEN
import att_trace_ref64 as R64

Z = os.path.join(GOLDEN, 'att_trace_tiny.npz')
FAMILIES = ('updown', 'att2in2', 'adaatt', 'adaattmo')
CASES = (('n1', True, 1), ('n2', True, 2), ('nomask', False, 1))
ENTRIES = {'capmi_att_trace_rollout': 10, 'capmi_att_trace_beam': 10, 'capmi_att_ground': 14}


def tiny_opt(name, **kw):
    V = 12
    o = argparse.Namespace(caption_model=name, vocab_size=V, input_encoding_size=16, rnn_size=16, num_layers=1, drop_prob_lm=0.0,
                           seq_length=6, max_length=6, fc_feat_size=20, att_feat_size=20, att_hid_size=16, use_bn=0, logit_layers=1,
                           vocab={str(i): 'w%d' % i for i in range(1, V + 1)}, N_enc=1, N_dec=1, d_model=16, d_ff=32, num_att_heads=2,
                           dropout=0.0, refine=1, refine_aoa=1, use_ff=0, decoder_type='AoA', use_multi_head=2, num_heads=2,
                           multi_head_scale=1, mean_feats=1, ctx_drop=0, dropout_aoa=0.0, out_res=0)
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def test_option_default_and_parsing():
    from imagecaptioning.pytorch_amd.captioning.utils import opts
    from imagecaptioning.pytorch_amd import att_trace
    assert opts.DEFAULTS['dump_attention'] == 0
    assert opts.parse_opt([]).dump_attention == 0 and opts.parse_opt(['--dump_attention', '1']).dump_attention == 1
    assert not att_trace.wanted({}) and not att_trace.wanted(None) and not att_trace.wanted({'return_attention': 0})
    assert att_trace.wanted({'return_attention': 1})


def test_models_start_without_a_trace():
    from imagecaptioning.pytorch_amd.captioning import models
    for name in FAMILIES + ('newfc',):
        m = models.setup(tiny_opt(name))
        assert m.last_attention is None and m._trace_req is None
        assert (m._trace_refusal is None) == (name != 'newfc')
        assert m._trace_col0 == (1 if name.startswith('adaatt') else 0)


@pytest.mark.parametrize('name', ('newfc', 'transformer', 'aoa', 'ensemble'))
def test_families_without_region_attention_refuse(name):
    from imagecaptioning.pytorch_amd.captioning import models
    if name == 'ensemble':
        model = models.AttEnsemble([models.setup(tiny_opt('updown')), models.setup(tiny_opt('att2in2'))])
    else:
        model = models.setup(tiny_opt(name))
    model.eval()
    fc, att = torch.zeros(2, 20), torch.zeros(2, 4, 20)
    with pytest.raises(NotImplementedError, match=type(model).__name__):
        model(fc, att, None, opt={'return_attention': 1}, mode='sample')
    assert model.last_attention is None
    # the option off: the refusal is not in the way (the call goes on to the device check of a CPU tensor, as before)
    from imagecaptioning.pytorch_amd._lib import CapmiError
    with pytest.raises((CapmiError, RuntimeError)) as e:
        with torch.no_grad():
            model(fc, att, None, opt={'return_attention': 0}, mode='sample')
    assert not isinstance(e.value, NotImplementedError)


def test_new_entries_in_header_match_the_binding():
    """parsed like tests/test_abi.py: declared in capmi.h, bound with the same argument count, appended behind the older entries"""
    from imagecaptioning.pytorch_amd import _lib
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'capmi.h')).read(), flags=re.S)
    decl = [(m.group(1), m.group(2).strip()) for m in
            re.finditer(r'\b(?:int|int64_t|const char \*)\s*(capmi_\w+)\s*\(([^;{]*?)\)\s*;', src, flags=re.S)]
    names = [n for n, _ in decl]
    for name, nargs in ENTRIES.items():
        assert name in names, name
        args = dict(decl)[name]
        assert len(args.split(',')) == nargs == len(_lib.SIGNATURES[name]), name
        assert args.rstrip().endswith('void *stream')
        assert hasattr(_lib.lib, name)
    # appended behind what was the last entry, in this order; nothing older is reordered (tests/test_abi.py holds the rest)
    for order in (names, list(_lib.SIGNATURES)):
        at = [order.index(n) for n in ('capmi_bn_linear_bwd',) + tuple(ENTRIES)]
        assert at == sorted(at), at


@pytest.mark.parametrize('name', FAMILIES)
def test_float64_helper_reproduces_the_fixture(name):
    z = np.load(Z)
    sentinel = name.startswith('adaatt')
    masks = z[name + '.att_masks']
    Kfull = masks.shape[1]
    K = int(masks.sum(1).max())
    assert K == 5 and Kfull == 6 and masks.sum(1).tolist() == [5, 3, 4]
    for case, masked, n in CASES:
        scores, seq, want = (z['%s.%s.%s' % (name, case, k)] for k in ('scores', 'seq', 'trace'))
        rows = masks[:, :K].repeat(n, 0) if masked else None
        w = R64.weights(scores, None if rows is None else rows[None], sentinel)
        got = R64.trace(w, seq, Kfull + int(sentinel))
        assert got.shape == want.shape == (3 * n, 6, Kfull + int(sentinel))
        assert float(np.abs(got - want).max()) <= 1e-12
        kept = R64.shifted_mask(seq)
        assert np.allclose(want.sum(-1)[kept], 1.0, atol=1e-12) and not want[~kept].any()
        if masked:
            assert not want[:, :, K + int(sentinel):].any()
            for r in range(3 * n):          # the padded regions of every image carry no weight
                assert not want[r, :, int(masks[r // n].sum()) + int(sentinel):].any()
    lens = (z[name + '.n1.seq'] > 0).sum(1)
    assert (lens == 1).any() and (lens == 6).any()          # one caption ends at step 1, one never ends


def test_ground_helper_ties_and_zero_steps():
    att = np.zeros((1, 3, 4))
    att[0, 0] = [0.25, 0.375, 0.375, 0.0]            # a tie: the lowest index
    att[0, 1] = [0.0, 0.0, 0.0, 1.0]
    g = R64.ground(att, boxes=np.arange(16, dtype=np.float64).reshape(1, 4, 4))
    assert g['top'].tolist() == [[1, 3, -1]]
    assert g['top_w'].tolist() == [[0.375, 1.0, 0.0]] and g['entropy'][0, 1] == 0 and g['entropy'][0, 2] == 0
    assert np.allclose(g['box'][0, 1], [12, 13, 14, 15]) and not g['box'][0, 2].any()


# ---------------------------------------------------------------------------------------------------------------------------
# tools/eval.py --dump_attention: the packing of one batch into one block, the npz keys, the boxes of a batch
# ---------------------------------------------------------------------------------------------------------------------------
def _fake_last(N, L, Kw, col0, boxes=None, n=1, seed=0):
    """a last_attention dict as att_trace.publish leaves it, from the float64 helper (CPU tensors)"""
    g = torch.Generator().manual_seed(seed)
    att = torch.rand(N, L, Kw, generator=g)
    att[:, :, Kw - 2:] = 0                                   # columns behind the clipped K
    att = att / att.sum(-1, keepdim=True)
    att[n, 2:] = 0                                           # image 1's first caption ended after two steps
    ref = R64.ground(att.double().numpy(), None if boxes is None else boxes.numpy(), n, col0)
    last = dict(att=att, top=torch.from_numpy(ref['top']), top_w=torch.from_numpy(ref['top_w']).float(),
                entropy=torch.from_numpy(ref['entropy']).float())
    if boxes is not None:
        last['box'] = torch.from_numpy(ref['box']).float()
    return last


@pytest.mark.parametrize('col0', (0, 1))
def test_attention_dump_packs_and_writes_every_array(col0, tmp_path):
    from imagecaptioning.pytorch_amd.tools import eval as E
    B, n, L, Kfull = 3, 2, 5, 6
    Kw = Kfull + col0
    boxes = torch.arange(B * Kfull * 4, dtype=torch.float32).view(B, Kfull, 4)
    last = _fake_last(B * n, L, Kw, col0, boxes, n)
    masks = torch.zeros(B, Kfull)
    for b, k in enumerate((4, 2, 3)):
        masks[b, :k] = 1
    infos = [{'id': 'img%d' % b, 'ix': b} for b in range(B)]
    dump = E.AttentionDump()
    dump.add_batch(last, infos, 2, masks, boxes, col0)                       # the third image is past num_images
    opt = argparse.Namespace(eval_results_dir=str(tmp_path), id='run7')
    path = dump.write(opt, 'val')
    assert path == os.path.join(str(tmp_path), 'run7_val_att.npz')
    z = np.load(path)
    assert sorted({k.split('/')[0] for k in z.files}) == ['img0', 'img1']
    for b, regions in ((0, 4), (1, 2)):
        r = b * n                                                            # the first row of the image
        key = 'img%d/' % b
        assert sorted(k[len(key):] for k in z.files if k.startswith(key)) == ['att', 'box', 'entropy', 'regions', 'top', 'top_box', 'top_w']
        assert int(z[key + 'regions']) == regions and z[key + 'regions'].dtype == np.int32
        assert np.array_equal(z[key + 'att'], last['att'][r, :, :regions + col0].numpy())
        assert np.array_equal(z[key + 'top'], last['top'][r].numpy()) and z[key + 'top'].dtype == np.int32
        assert np.array_equal(z[key + 'top_w'], last['top_w'][r].numpy())
        assert np.array_equal(z[key + 'entropy'], last['entropy'][r].numpy())
        assert np.array_equal(z[key + 'box'], last['box'][r].numpy())
        want = np.zeros((L, 4), dtype=np.float32)
        for t in range(L):
            k = int(last['top'][r, t]) - col0
            if k >= 0:                                                       # not a zeroed step, not the sentinel
                want[t] = boxes[b, k].numpy()
        assert np.array_equal(z[key + 'top_box'], want)
    assert (z['img1/top'][2:] == -1).all() and not z['img1/top_box'][2:].any()      # image 1's caption ended: zeroed steps
    # no boxes, no masks: every region counts, no box keys
    dump = E.AttentionDump()
    last = _fake_last(B, L, Kw, col0)
    dump.add_batch(last, infos, 3, None, None, col0)
    z = np.load(dump.write(opt, 'test'))
    assert sorted(k for k in z.files if k.startswith('img2/')) == ['img2/' + k for k in ('att', 'entropy', 'regions', 'top', 'top_w')]
    assert int(z['img2/regions']) == Kfull and z['img2/att'].shape == (L, Kw)
    assert np.array_equal(z['img2/top'], last['top'][2].numpy())


def test_batch_boxes_follow_the_loaders_row_order(tmp_path):
    from imagecaptioning.pytorch_amd.tools import eval as E
    from imagecaptioning.pytorch_amd.captioning.data import feature_loader as fl
    box_dir = tmp_path / 'box'
    box_dir.mkdir()
    rs = np.random.RandomState(3)
    raw = {}
    for img, k in (('7', 3), ('9', 5)):
        x1, y1 = rs.rand(k) * 50, rs.rand(k) * 40
        raw[img] = np.stack([x1, y1, x1 + 1 + rs.rand(k) * 40, y1 + 1 + rs.rand(k) * 30], 1).astype(np.float32)
        np.save(str(box_dir / (img + '.npy')), raw[img])
    data = {'infos': [{'id': '7', 'ix': 0}, {'id': '9', 'ix': 1}]}

    class Loader:
        info = {'images': [{'id': '7', 'height': 80, 'width': 100}, {'id': '9', 'height': 60, 'width': 90}]}
    opt = argparse.Namespace(input_json='x.json', input_box_dir=str(box_dir), use_box=0, norm_box_feat=0)
    got = E.batch_boxes(Loader(), opt, data, 6, 'cpu')
    assert got.shape == (2, 6, 4) and got.dtype == torch.float32
    assert np.array_equal(got[0, :3].numpy(), raw['7']) and not got[0, 3:].any()
    assert np.array_equal(got[1, :5].numpy(), raw['9']) and not got[1, 5:].any()
    # use_box: the loader re-orders the region rows by area, descending; the boxes follow
    opt.use_box = 1
    got = E.batch_boxes(Loader(), opt, data, 6, 'cpu')
    for i, (img, h, w) in enumerate((('7', 80, 100), ('9', 60, 90))):
        area = fl.box_columns(raw[img], h, w)[:, 4]
        order = sorted(range(len(area)), key=lambda j: -area[j])
        assert np.array_equal(got[i, :len(order)].numpy(), raw[img][order])
        rows = fl.append_boxes(np.arange(len(area), dtype=np.float32)[:, None], raw[img], h, w)       # a feature that names its row
        assert rows[:, 0].astype(int).tolist() == order
    # fewer columns than regions: cut, as the features are
    assert E.batch_boxes(Loader(), opt, data, 4, 'cpu').shape == (2, 4, 4)
    # no box directory, or the synthetic loader: no boxes
    assert E.batch_boxes(Loader(), argparse.Namespace(input_json='x.json', input_box_dir=str(tmp_path / 'none')), data, 6, 'cpu') is None
    assert E.batch_boxes(Loader(), argparse.Namespace(input_json='', input_box_dir=str(box_dir)), data, 6, 'cpu') is None
