"""CPU checks of transformer_ref64.py: the float64 closed forms against torch autograd, the arms the case tables claim against the
planner restatement (and that against capmi_mha_plan, which is host code), the sizes of the tables, and the measurement behind
LN_BWD_TOL."""
import ctypes

import pytest
import torch

import transformer_ref64 as T


def ln_autograd(d):
    x, a, b = (T.d64(d[k]).requires_grad_(True) for k in ('x', 'a', 'b'))
    y = a * (x - x.mean(-1, keepdim=True)) / (x.std(-1, keepdim=True) + T.EPS) + b            # TransformerModel.py:84-87
    (y * T.d64(d['dy'])).sum().backward()
    return y.detach(), x.grad, a.grad, b.grad


@pytest.mark.parametrize('M,D', [(7, 8), (7, 261), (33, 1028), (7, 2052)])
def test_layernorm_closed_forms_equal_autograd(M, D):
    d = T.ln_inputs(M, D, seed=D + M)
    rows = [r for r in range(M) if r != d['plant']]
    y, dx, da, db = ln_autograd(d)
    y_ref, mean, inv = T.ln_fwd_ref(d['x'], d['a'], d['b'])
    dx_ref, gs, _, _ = T.ln_bwd_ref(d['dy'], d['x'], d['a'])
    assert T.rel_err(y[rows], y_ref[rows]) < 1e-10
    assert T.rel_err(dx[rows], dx_ref[rows]) < 1e-10
    # parameter gradients over the ordinary rows (autograd of the constant row divides by eps; the planted row is stated, not derived)
    d2 = {k: (v[rows] if torch.is_tensor(v) and v.dim() == 2 else v) for k, v in d.items()}
    _, _, da2, db2 = ln_autograd(d2)
    _, _, da_ref, db_ref = T.ln_bwd_ref(d2['dy'], d2['x'], d2['a'])
    assert T.rel_err(da2, da_ref) < 1e-10 and T.rel_err(db2, db_ref) < 1e-10
    # the planted row: y = b, inv = 1 / eps, dx = inv (g - mean g)
    p = d['plant']
    assert torch.equal(y_ref[p], T.d64(d['b'])) and float(mean[p]) == 0.5 and abs(float(inv[p]) * T.EPS - 1) < 1e-12
    g = T.d64(d['dy'][p]) * T.d64(d['a'])
    assert torch.allclose(dx_ref[p], (g - g.mean()) / T.EPS, rtol=1e-12, atol=0)


def test_layernorm_tables_reach_every_instance():
    for table in (T.LN_FWD, T.LN_BWD):
        ds = {D for _, D in table}
        assert {8, 256, 260, 512, 516, 1024, 1028, 2048, 2052} <= ds
        assert {T.ne_bucket(D) for D in ds} == {4, 8, 16, 32, 0}
        assert any(D % 4 for D in ds) and any(D < 64 for D in ds)
        assert {M for M, _ in table} == {1, 7, 33}
    assert [T.ne_bucket(D) for D in (256, 257, 512, 513, 1024, 1025, 2048, 2049)] == [4, 8, 8, 16, 16, 32, 32, 0]
    assert {T.ne_bucket(D) for _, D, _ in T.LN_PARTS} == {4, 8, 16, 32} and all(D <= 2048 for _, D, _ in T.LN_PARTS)
    assert {(M, T.ln_parts_rows(M)) for M, _, _ in T.LN_PARTS} == {(9, 2), (17, 3)}
    assert {acc for _, _, acc in T.LN_PARTS} == {0, 1}
    assert {T.ne_bucket(D) for _, D, _, _ in T.LN_SLABS} == {4, 8, 16, 32} and all(D % 4 == 0 for _, D, _, _ in T.LN_SLABS)
    assert {(a, b) for _, _, a, b in T.LN_SLABS} == {(1, 1), (3, 2), (5, 9)}
    assert all(8 * M * D <= T.MAX_FLOATS for M, D in T.LN_BWD) and all((5 + 2 * 9 + 6) * M * D <= T.MAX_FLOATS for M, D, _, _ in T.LN_SLABS)


def test_layernorm_bwd_bound_is_derived_from_float32():
    """LN_BWD_TOL = max(4 x the float32 closed form's error against float64 over the tables, 5e-6)"""
    worst = dict(dx=0.0, g_scaled=0.0, d_a=0.0, d_b=0.0)
    cases = [(M, D) for M, D in T.LN_BWD] + [(M, D) for M, D, _ in T.LN_PARTS] + [(M, D) for M, D, _, _ in T.LN_SLABS]
    for i, (M, D) in enumerate(cases):
        d = T.ln_inputs(M, D, seed=i)
        rows = [r for r in range(M) if r != d['plant']]
        if not rows:
            continue
        x, dy = d['x'][rows], d['dy'][rows]
        _, mean, inv = T.ln_fwd_ref(x, d['a'], d['b'])
        got = T.ln_bwd_f32(dy.numpy(), x.numpy(), d['a'].numpy(), mean.float().numpy(), inv.float().numpy())
        for k, g, r in zip(worst, got, T.ln_bwd_ref(dy, x, d['a'])):
            worst[k] = max(worst[k], T.rel_err(torch.from_numpy(g), r))
    print('float32 closed form vs float64:', ', '.join('%s %.2e' % kv for kv in worst.items()))
    assert max(worst.values()) <= T.LN_BWD_F32_MEASURED
    assert T.LN_BWD_TOL == max(4 * T.LN_BWD_F32_MEASURED, 5e-6)


def mha_autograd_free_check(r, d, o, p):
    """o from p, drop and v without autograd"""
    Nkv, qpk, Tq, Tk, h, dk = (r[k] for k in ('Nkv', 'qpk', 'Tq', 'Tk', 'h', 'dk'))
    vh = T.d64(d['v']).view(Nkv, Tk, h, dk).transpose(1, 2).repeat_interleave(qpk, 0)
    pd = p * T.d64(d['drop']) if d['drop'] is not None else p
    return (pd @ vh).transpose(1, 2).reshape(o.shape)


def test_mha_reference_properties():
    for i, r in enumerate(T.MHA):
        if T.mha_floats(r) > 200000:
            continue
        d = T.mha_inputs(r, seed=i)
        o, p, dq, dk, dv = T.mha_ref(r, d)
        assert all(bool(torch.isfinite(t).all()) for t in (o, p, dq, dk, dv)), r['name']
        assert float((p.sum(-1) - 1).abs().max()) < 1e-12
        assert T.rel_err(mha_autograd_free_check(r, d, o, p), o) < 1e-12
        if r['causal']:
            for t in range(r['Tq']):
                assert float(p[:, :, t, r['q_pos0'] + t + 1:].abs().sum()) == 0.0
                assert r['mask'] is not None or float(p[:, :, t, r['q_pos0'] + t].min()) > 0.0
        if r['mask'] is not None:
            m = d['mask'] if r['mask'] in ('q1', 'qT') else d['mask'].repeat_interleave(r['qpk'], 0)
            assert float(p.masked_select(~m.unsqueeze(1).expand_as(p)).abs().sum()) == 0.0


def test_mha_table_reaches_every_arm():
    reached = set()
    for r in T.MHA:
        got = T.mha_arms(r)
        assert set(r['arms']) <= got, (r['name'], set(r['arms']) - got)
        reached |= set(r['arms'])
    assert reached == set(T.MHA_ARMS), set(T.MHA_ARMS) ^ reached
    # the one row with a short last pass on the matrix pipe, spelt out
    r = next(r for r in T.MHA if 'fwd:short_last_mfma' in r['arms'])
    ch, _, mfma, _ = T.mha_plan('fwd', r['Nkv'] * r['qpk'], r['qpk'], r['Tq'], r['Tk'], r['h'], r['dk'])
    assert mfma == 1 and ch == 16 and 1 <= r['qpk'] * r['Tq'] - ch <= 15


def test_mha_table_sizes():
    for r in T.MHA:
        for kind in ('fwd', 'bwd') if r['bwd'] else ('fwd',):
            assert T.mha_plan(kind, r['Nkv'] * r['qpk'], r['qpk'], r['Tq'], r['Tk'], r['h'], r['dk'])[3] <= 160 * 1024, (r['name'], kind)
        assert T.mha_floats(r) <= T.MAX_FLOATS, r['name']
        assert r['dk'] % 4 == 0 and (r['layout'] != 'packed' or (r['qpk'] == 1 and r['Tq'] == r['Tk']))
    # what the refusals test relies on
    assert T.mha_plan('fwd', 1, 1, 4, 200, 1, 128)[3] > 160 * 1024


def test_mha_plan_equals_capmi_mha_plan():
    """capmi_mha_plan is host code: the Python restatement is held to it here as well as on the GPU machine"""
    from imagecaptioning.pytorch_amd import _lib
    shapes = [(r['Nkv'] * r['qpk'], r['qpk'], r['Tq'], r['Tk'], r['h'], r['dk']) for r in T.MHA]
    shapes += [(Nkv * qpk, qpk, Tq, Tk, h, dk) for Nkv in (1, 40) for qpk in (1, 5) for Tq in (1, 21, 40, 77) for Tk in (7, 36, 100)
               for h in (1, 8) for dk in (16, 64, 128)]
    for s in shapes:
        for bwd in (0, 1):
            ch, th, mf = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
            lds = ctypes.c_int64()
            rc = _lib.lib.capmi_mha_plan(bwd, *s, ctypes.byref(ch), ctypes.byref(th), ctypes.byref(mf), ctypes.byref(lds))
            want = T.mha_plan('bwd' if bwd else 'fwd', *s)
            assert (ch.value, th.value, mf.value, lds.value) == want, (s, bwd)
            assert rc == (_lib.EINVAL if want[3] > 160 * 1024 else 0)


def test_fused_references_equal_torch():
    import torch.nn.functional as F
    for kind in (T.CTX_GLU, T.CTX_RELU, T.CTX_LSTM):
        d = T.fused_inputs(kind, 7, 36, 5, True, seed=kind)
        saved, c, out, oa, ob = T.fused_ref(kind, d)
        pre = d['pre']
        if kind == T.CTX_GLU:
            want = F.glu(pre, -1)
            assert torch.equal(saved, pre)
        elif kind == T.CTX_RELU:
            want = F.relu(pre)
            assert saved is None
        else:
            cell = torch.nn.LSTMCell(4 * 36, 36, bias=False).double()
            with torch.no_grad():
                cell.weight_ih.copy_(torch.eye(4 * 36, dtype=T.F64))                  # gates = the input itself
                cell.weight_hh.zero_()
                want, cw = cell(pre, (torch.zeros(7, 36, dtype=T.F64), T.d64(d['c_prev'])))
            assert T.rel_err(c, cw) < 1e-12
            assert T.rel_err(saved, torch.cat([torch.sigmoid(pre[:, :72]), torch.tanh(pre[:, 72:108]), torch.sigmoid(pre[:, 108:])], 1)) < 1e-12
        assert T.rel_err(out, want) < 1e-12
        assert T.rel_err(oa, (out + T.d64(d['resid'])) * T.d64(d['mask_a'])) < 1e-12 and T.rel_err(ob, out * T.d64(d['mask_b'])) < 1e-12
    assert {s for _, _, s, _ in T.GLU_FUSED} == {1, 4, 5, 9} and {(M, R) for M, R, _, _ in T.GLU_FUSED} >= {(1, 4), (7, 36), (64, 36)}
    assert {k for k, *_ in T.CTX_FUSED} == {0, 1, 2} and all(M <= 64 for _, M, *_ in T.CTX_FUSED)
    assert {s for _, _, s, _ in T.RELU_BWD} == {None, 1, 8, 9} == {s for _, _, s, _ in T.GLU_BWD}
    assert {s for _, _, s, _ in T.SPLIT_HALVES} == {1, 8, 9}


def test_pointwise_backward_references_equal_autograd():
    for M, R, s, am in T.GLU_BWD[:6] + T.GLU_BWD[-2:]:
        d = T.add_inputs(M, R, s, am, seed=M + R, glu=True)
        pre = T.d64(d['pre']).requires_grad_(True)
        (torch.nn.functional.glu(pre, -1) * T.add_grad(d)).sum().backward()
        assert T.rel_err(pre.grad, T.glu_bwd_ref(d)) < 1e-10
    for M, R, s, am in T.RELU_BWD[:6] + T.RELU_BWD[-2:]:
        d = T.add_inputs(M, R, s, am, seed=M + R, glu=False)
        ref = T.relu_bwd_ref(d)
        assert float(ref[T.d64(d['out']) <= 0].abs().sum()) == 0.0 and int((d['out'] == 0).sum()) >= M * R // 3
        assert torch.equal(ref[d['out'] > 0], T.add_grad(d)[d['out'] > 0])
