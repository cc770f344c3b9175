"""Knowledge distillation on the MI355X: capmi_distill_loss_fwd / _bwd against the float64 restatement (tests/distill_ref64.py), the
fused route of DistillCriterion against its generic route through the teacher-forced backward of three families, the teacher's
mixture, and tools/train.py with --distill_from."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT
from distill_ref64 import distill64
from test_model_api_gpu import tiny_opt, DEV

pytestmark = pytest.mark.gpu
PKG = os.path.join(ROOT, 'imagecaptioning', 'pytorch_amd')
KW = {'updown': {}, 'newfc': dict(caption_model='newfc'),
      'transformer': dict(caption_model='transformer', N_enc=2, N_dec=2, d_model=16, d_ff=32, num_att_heads=2, dropout=0.0)}
N, T, LD, TT = 6, 5, 9, 7          # B 3 x n 2 rows, T = 5 steps out of tok_ld = mask_ld = 9, a teacher of 7 steps


# ---------------------------------------------------------------------------------------------------------------- the kernels
def _inputs(V1, layout, seed, N=N, T=T):
    """fp32 device inputs: the student near the teacher; layout 'cut': the teacher is the [:, :T] part of a [N, TT, V1 + 3] buffer
    (row stride above V1, a longer sample pitch; rows off the student's alignment), 'plain': [N, T, V1] contiguous (the float4 body
    wherever V1 allows).  Masks with zero positions mid-row and a fully masked sample."""
    LD, TT = T + 4, T + 2
    g = torch.Generator().manual_seed(seed)
    lt = torch.log_softmax(2 * torch.randn(N, TT, V1, generator=g), 2)
    ls = torch.log_softmax(lt[:, :T] + 0.5 * torch.randn(N, T, V1, generator=g), 2)
    tok = torch.randint(0, V1, (N, LD), generator=g)
    mask = (torch.rand(N, LD, generator=g) > 0.3).float()
    mask[:, 0] = 1
    mask[1, 2] = 0
    mask[4, 1] = 0
    mask[3] = 0
    if layout == 'cut':
        buf = torch.full((N, TT, V1 + 3), float('nan'))
        buf[:, :, :V1] = lt
        lt_dev = buf.to(DEV)[:, :, :V1]
    else:
        lt_dev = lt[:, :T].contiguous().to(DEV)
    return ls.to(DEV), lt_dev, tok.to(DEV), mask.to(DEV)


def _check_kernel(ls, lt, tok, mask, lam, tau, per_row):
    """the tolerances of tests/test_ppo_gpu.py for its KL rows (2e-5 of the sum of |terms| + 1e-6), its losses (2e-5 of the scale of
    the summed terms) and its dense gradient (2e-5 relative + 1e-6 of the largest entry)"""
    from imagecaptioning.pytorch_amd import ops
    u = torch.linspace(0.5, 1.5, ls.shape[0], device=DEV) if per_row else torch.tensor([0.7], device=DEV)
    out, loss_rows, rs, msum = ops.distill_loss_fwd(ls, lt, tok, mask, lam, tau, per_row)
    grad = torch.full_like(ls, float('nan'))                 # NaN-filled: every entry must be overwritten
    ops.distill_loss_bwd(ls, lt, tok, mask, rs, msum, u, lam, tau, per_row, out=grad)
    torch.cuda.synchronize()
    ref = distill64(ls, lt, tok, mask, lam, tau, per_row, u=(u if per_row else 0.7))
    m = ref['mask'] > 0
    kl, nll = rs[2].double().cpu(), rs[3].double().cpu()
    e_kl = float(((kl - ref['kl']).abs() / (2e-5 * ref['kl_bound'] + 1e-6))[m].max())
    assert e_kl <= 1.0, ('kl', e_kl)
    assert torch.equal(nll[m], ref['nll'][m])
    assert torch.equal(rs[:, ~m.to(DEV)], torch.zeros_like(rs[:, ~m.to(DEV)]))
    w_kd = lam * tau * tau
    scale = w_kd * float(ref['kl_bound'][m].mean()) + (1 - lam) * float(ref['nll'][m].abs().mean()) + 1e-6
    assert abs(float(out[0]) - float(ref['lm_loss'])) <= 2e-5 * (float(ref['nll'][m].abs().mean()) + 1e-6)
    assert abs(float(out[1]) - float(ref['kd_loss'])) <= 2e-5 * (float(ref['kl_bound'][m].mean()) + 1e-6)
    live = m.sum(1) > 0
    if per_row:
        lr = loss_rows.double().cpu()
        assert bool(torch.isnan(lr[~live]).all()) and bool(torch.isfinite(lr[live]).all())      # NaN in the masked sample only
        assert float((lr[live] - ref['loss'][live]).abs().max()) <= 2e-5 * (scale + float(ref['loss'][live].abs().max()))
        assert torch.equal(msum.cpu().double(), ref['mask'].sum(1))
    else:
        assert abs(float(out[2]) - float(ref['loss'])) <= 2e-5 * scale
        assert float(msum) == float(ref['mask'].sum())
    gref = ref['grad']
    err = (grad.double().cpu() - gref).abs()
    e_g = float((err / (2e-5 * gref.abs() + 1e-6 * float(gref.abs().max()) + 1e-30)).max())
    assert e_g <= 1.0, ('grad', e_g)
    assert torch.equal(grad[~m.to(DEV)], torch.zeros_like(grad[~m.to(DEV)]))       # masked rows: exact zeros over the NaN fill
    return out, rs, grad


@pytest.mark.parametrize('per_row', (False, True))
@pytest.mark.parametrize('layout', ('cut', 'plain'))
@pytest.mark.parametrize('V1', (1, 3, 31, 32, 4099))
def test_kernel_against_fp64(V1, layout, per_row):
    """V1: below one float4; odd (rows off the 16-byte boundary); aligned; several trips per lane plus a tail"""
    ls, lt, tok, mask = _inputs(V1, layout, seed=V1 * 7 + per_row)
    for lam in (0.0, 0.3, 1.0):
        for tau in (0.5, 1.0, 2.0):
            _check_kernel(ls, lt, tok, mask, lam, tau, per_row)


@pytest.mark.parametrize('per_row', (False, True))
@pytest.mark.parametrize('layout', ('cut', 'plain'))
@pytest.mark.parametrize('V1', (3, 31))
def test_kernel_against_fp64_more_rows_than_fold_threads(V1, layout, per_row):
    """N * T = 1100: the finish kernel's 1024 threads take a second trip over the rows; a fully masked sample as above"""
    ls, lt, tok, mask = _inputs(V1, layout, seed=V1 * 11 + per_row, N=50, T=22)
    for lam in (0.0, 0.3, 1.0):
        _check_kernel(ls, lt, tok, mask, lam, 2.0, per_row)


def test_two_runs_are_bit_equal_and_identity_is_zero():
    from imagecaptioning.pytorch_amd import ops
    ls, lt, tok, mask = _inputs(4099, 'plain', seed=5)
    u = torch.tensor([1.3], device=DEV)
    runs = []
    for _ in range(2):
        out, _, rs, msum = ops.distill_loss_fwd(ls, lt, tok, mask, 0.3, 2.0, False)
        grad = ops.distill_loss_bwd(ls, lt, tok, mask, rs, msum, u, 0.3, 2.0, False)
        runs.append((out.clone(), rs.clone(), grad.clone()))
    torch.cuda.synchronize()
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    # teacher == student at lambda 1: loss 0 and gradient 0, exactly (the two rows go through the same operations)
    out, _, rs, msum = ops.distill_loss_fwd(ls, ls.clone(), tok, mask, 1.0, 2.0, False)
    grad = ops.distill_loss_bwd(ls, ls.clone(), tok, mask, rs, msum, u, 1.0, 2.0, False)
    assert float(out[1]) == 0.0 and float(out[2]) == 0.0 and float(grad.abs().max()) == 0.0


def test_kernel_edge_cases():
    """a teacher column of probability 0 contributes an exact 0; non-finite values in masked rows are not read; a token outside the
    vocabulary gives NaN; invalid arguments are refused, N == 0 succeeds"""
    from imagecaptioning.pytorch_amd import _lib, ops
    from imagecaptioning.pytorch_amd._lib import CapmiError
    V1 = 37
    ls, lt, tok, mask = _inputs(V1, 'plain', seed=9)
    lt = lt.clone()
    lt[:, :, 4] = -float('inf')
    lt = torch.log_softmax(lt, 2)
    ls[3] = float('nan')                                                 # sample 3 is fully masked
    lt[1, 2] = -float('inf')                                             # so is position (1, 2)
    out, _, rs, msum = ops.distill_loss_fwd(ls, lt, tok, mask, 0.6, 1.0, False)
    grad = ops.distill_loss_bwd(ls, lt, tok, mask, rs, msum, torch.ones(1, device=DEV), 0.6, 1.0, False)
    torch.cuda.synchronize()
    assert torch.isfinite(out).all() and torch.isfinite(grad).all()
    clean_s, clean_t = torch.nan_to_num(ls, nan=0.0), lt.clone()
    clean_t[1, 2] = clean_t[0, 0]
    ref = distill64(clean_s, clean_t, tok, mask, 0.6, 1.0)
    assert abs(float(out[2]) - float(ref['loss'])) <= 2e-5 * (abs(float(ref['loss'])) + 1e-6)
    bad_tok = tok.clone()
    bad_tok[0, 0] = V1
    out2 = ops.distill_loss_fwd(ls, lt, bad_tok, mask, 0.6, 1.0, False)[0]
    assert torch.isnan(out2[0]) and torch.isnan(out2[2]) and torch.isfinite(out2[1])
    for lam, tau in ((0.5, 0.0), (0.5, -1.0), (0.5, float('inf')), (0.5, float('nan')), (-0.1, 1.0), (1.1, 1.0), (float('nan'), 1.0)):
        with pytest.raises(CapmiError):
            ops.distill_loss_fwd(ls, lt, tok, mask, lam, tau, False)
        with pytest.raises(CapmiError):
            ops.distill_loss_bwd(ls, lt, tok, mask, rs, msum, torch.ones(1, device=DEV), lam, tau, False)
    with pytest.raises(CapmiError):
        ops.distill_loss_fwd(ls.double(), lt, tok, mask, 0.5, 1.0, False)
    with pytest.raises(CapmiError):
        ops.distill_loss_fwd(ls.cpu(), lt, tok, mask, 0.5, 1.0, False)

    # the entry points themselves: strides below V1, pitches below T, NULL pointers
    def desc():
        p = ops._distill_desc(lt, tok, mask, N, T, V1, 0.5, 1.0, False, 'test')
        o3, g1 = torch.empty(3, device=DEV), torch.ones(1, device=DEV)
        gbuf = torch.empty_like(ls)
        p.lp_s, p.row_stats, p.msum, p.out, p.g_out, p.grad = (x.data_ptr() for x in (ls, rs, msum, o3, g1, gbuf))
        p._keep = (o3, g1, gbuf)
        return p
    st = _lib.stream_ptr()
    assert _lib.lib.capmi_distill_loss_fwd(C.byref(desc()), st) == 0 and _lib.lib.capmi_distill_loss_bwd(C.byref(desc()), st) == 0
    for field, val in (('ld_s', V1 - 1), ('ld_t', V1 - 1), ('t_rows', T - 1), ('tok_ld', T - 1), ('mask_ld', T - 1), ('lp_s', None),
                       ('lp_t', None), ('tok', None), ('mask', None), ('row_stats', None), ('msum', None), ('T', 0), ('V1', 0), ('N', -1)):
        p = desc()
        setattr(p, field, val)
        assert _lib.lib.capmi_distill_loss_fwd(C.byref(p), st) == _lib.EINVAL, field
        assert _lib.lib.capmi_distill_loss_bwd(C.byref(p), st) == _lib.EINVAL, field
    for field, val in (('out', None),):
        p = desc()
        setattr(p, field, val)
        assert _lib.lib.capmi_distill_loss_fwd(C.byref(p), st) == _lib.EINVAL, field
    for field, val in (('ld_grad', V1 - 1), ('grad', None), ('g_out', None)):
        p = desc()
        setattr(p, field, val)
        assert _lib.lib.capmi_distill_loss_bwd(C.byref(p), st) == _lib.EINVAL, field
    p = desc()
    p.per_row = 1                                                        # per_row without loss_rows
    assert _lib.lib.capmi_distill_loss_fwd(C.byref(p), st) == _lib.EINVAL
    p = desc()
    p.N = 0
    assert _lib.lib.capmi_distill_loss_fwd(C.byref(p), st) == 0 and _lib.lib.capmi_distill_loss_bwd(C.byref(p), st) == 0
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------- models
def family_model(fam):
    from imagecaptioning.pytorch_amd.captioning import models
    z = np.load(os.path.join(GOLDEN, fam + '_tiny.npz'))
    model = models.setup(tiny_opt(**KW[fam]))
    model.load_state_dict({k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith('P.')})
    return model.to(DEV)


def _batch():
    u = np.load(os.path.join(GOLDEN, 'updown_tiny.npz'))
    return tuple(torch.from_numpy(u[k]).to(DEV) for k in ('fc', 'att', 'att_masks', 'labels', 'masks'))


def _teacher(student, fams, weights):
    from imagecaptioning.pytorch_amd.captioning.modules import losses
    opt = tiny_opt(distill_weight=0.7, distill_temperature=2.0, distill_from=list(fams), distill_weights=list(weights))
    return losses.DistillTeacher(opt, student, members=[family_model(f) for f in fams])


def _grads(model):
    return {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}


@pytest.mark.parametrize('red', ('mean', 'none'))
@pytest.mark.parametrize('fam', ('updown', 'newfc', 'transformer'))
def test_fused_route_equals_generic_route(fam, red):
    """same student, same batch, a two-member teacher of the two other families: the fused route (capmi_distill_loss_*) and the
    generic ATen route give the same losses and, after the teacher-forced backward, the same parameter gradients -- the dense
    gradient reaches all three backward paths"""
    from imagecaptioning.pytorch_amd.captioning.modules import losses
    model = family_model(fam).train()
    teacher = _teacher(model, [f for f in KW if f != fam], (0.25, 0.75))
    crit = losses.DistillCriterion(0.7, 2.0)
    fc, att, am, labels, masks = _batch()
    res = {}
    for route in ('fused', 'generic'):
        model.zero_grad(set_to_none=True)
        logp = model(fc, att, labels[..., :-1], am)
        lt = teacher(fc, att, labels[..., :-1], am, logp.size(1))
        o = (crit if route == 'fused' else crit.generic)(logp, lt, labels[..., 1:], masks[..., 1:], reduction=red)
        assert (type(o['loss'].grad_fn).__name__ == '_FusedDistillBackward') == (route == 'fused')
        (o['loss'] if red == 'mean' else o['loss'].sum()).backward()
        res[route] = (o, _grads(model))
    (oa, ga), (ob, gb) = res['fused'], res['generic']
    for k in ('loss', 'lm_loss', 'kd_loss'):
        assert torch.allclose(oa[k], ob[k], atol=1e-5, rtol=1e-4), (k, oa[k], ob[k])
    assert float(oa['kd_loss']) > 0
    floor = 1e-6 * max(float(v.abs().max()) for v in gb.values())
    assert set(ga) == set(gb) and len(ga) > 0
    for k in ga:
        assert float((ga[k] - gb[k]).abs().max()) <= 2e-4 * float(gb[k].abs().max()) + floor, k


def test_teacher_mixture_is_the_weighted_mean_of_probabilities():
    """two members of different families with weights (0.25, 0.75): log(0.25 e^l1 + 0.75 e^l2) in float64, cut to the student's T"""
    model = family_model('updown')
    teacher = _teacher(model, ('newfc', 'transformer'), (1.0, 3.0))
    fc, att, am, labels, masks = _batch()
    seq = labels[..., :-1]
    Ts = model(fc, att, seq, am).size(1)
    with torch.no_grad():
        l1, l2 = (m(fc, att, seq, am)[:, :Ts].double() for m in teacher.members)
    got = teacher(fc, att, seq, am, Ts)
    want = torch.log(0.25 * l1.exp() + 0.75 * l2.exp())
    assert tuple(got.shape[:2]) == (l1.shape[0], Ts) and not got.requires_grad
    # (positions behind the longest caption are masked in every criterion; there the families' early stops leave different rows)
    on = masks[..., 1:].reshape(l1.shape[0], -1)[:, :Ts] > 0
    assert bool(on[:, 0].all()) and float((got.double() - want)[on].abs().max()) <= 1e-5
    assert all(not p.requires_grad for m in teacher.members for p in m.parameters())


# ---------------------------------------------------------------------------------------------------------------- end to end
def _kd(text):
    """(lm_loss, kd_loss) of every log line of a distillation run"""
    rows = []
    for ln in text.splitlines():
        if 'kd_loss =' in ln:
            f = dict(x.split(' = ') for x in ln.split(', ')[1:])
            rows.append((float(f['lm_loss']), float(f['kd_loss'])))
    return rows


def test_train_py_distills_an_ensemble(tmp_path, capsys):
    sys.path.insert(0, PKG)
    from imagecaptioning.pytorch_amd.tools import train as T
    from captioning.utils import opts
    small = ['--rnn_size', '32', '--input_encoding_size', '32', '--att_hid_size', '16', '--fc_feat_size', '24', '--att_feat_size', '24',
             '--vocab_size', '40', '--synthetic_regions', '5', '--seq_length', '6', '--max_length', '6', '--batch_size', '4',
             '--seq_per_img', '2', '--synthetic_images', '4', '--losses_log_every', '1', '--drop_prob_lm', '0']
    tf = ['--caption_model', 'transformer', '--d_model', '32', '--d_ff', '64', '--N_enc', '1', '--N_dec', '1', '--num_att_heads', '4',
          '--dropout', '0']
    # the teachers: two checkpoints of two families, a handful of iterations each
    T.train(opts.parse_opt(small + ['--max_iters', '4', '--save_checkpoint_every', '4', '--id', 'A', '--checkpoint_path',
                                    str(tmp_path / 'log_A')]))
    T.train(opts.parse_opt(small + tf + ['--max_iters', '4', '--save_checkpoint_every', '4', '--id', 'B', '--checkpoint_path',
                                         str(tmp_path / 'log_B')]))
    teachers = {k: torch.load(tmp_path / ('log_%s' % k) / 'model.pth') for k in 'AB'}
    capsys.readouterr()
    kd = ['--distill_log_root', str(tmp_path), '--distill_temperature', '2', '--learning_rate', '0.01']
    # lambda = 1 on one repeated batch (4 images, batch 4): the student moves towards the ensemble
    s = tmp_path / 'student'
    loss = T.train(opts.parse_opt(small + kd + ['--distill_from', 'A', 'B', '--distill_weights', '1', '3', '--distill_weight', '1',
                                                '--max_iters', '20', '--save_checkpoint_every', '20', '--id', 'S',
                                                '--checkpoint_path', str(s)]))
    rows = _kd(capsys.readouterr().out)
    assert np.isfinite(loss) and len(rows) == 20 and all(np.isfinite(r).all() for r in rows)
    assert rows[-1][1] < rows[0][1], rows
    trained = torch.load(s / 'model.pth')
    assert set(trained) == set(teachers['A'])                            # the student's own keys: no teacher in the checkpoint
    assert any(not torch.equal(trained[k], teachers['A'][k]) for k in trained)
    for k in 'AB':                                                       # the teachers' files are untouched
        again = torch.load(tmp_path / ('log_%s' % k) / 'model.pth')
        assert all(torch.equal(again[x], teachers[k][x]) for x in again)
    # --start_from resumes a distillation
    loss = T.train(opts.parse_opt(small + kd + ['--distill_from', 'A', 'B', '--distill_weight', '0.7', '--max_iters', '22', '--id', 'S',
                                                '--start_from', str(s), '--checkpoint_path', str(s)]))
    rows = _kd(capsys.readouterr().out)
    assert np.isfinite(loss) and len(rows) == 2
    # a student that starts from the single teacher's weights: kd_loss of its first iteration is 0 to the kernel's tolerance
    T.train(opts.parse_opt(small + kd + ['--distill_from', 'A', '--distill_weight', '0.7', '--max_iters', '1', '--id', 'S2',
                                         '--start_from', str(tmp_path / 'log_A'), '--checkpoint_path', str(tmp_path / 's2')]))
    rows = _kd(capsys.readouterr().out)
    assert len(rows) == 1 and abs(rows[0][1]) <= 1.5e-6 and rows[0][0] > 0.1, rows
