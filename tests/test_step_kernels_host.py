"""The float64 references of step_kernels_ref64.py, anchored outside themselves: the LSTM cell against torch.nn.LSTMCell, the maxout
(att2in2) cell and the additive attention against att2in2_ref64.step, the AdaAtt cell against adaatt_ref64.step -- and the properties of
the shared case tables that the GPU tests lean on (planted extremes, finite references, the maxout tie cap).  No GPU."""
import pytest
import torch

import adaatt_ref64
import att2in2_ref64
import step_kernels_ref64 as S

F64 = torch.float64


def close(a, b, tol=1e-12):
    return float((a - b).abs().max()) <= tol * (1.0 + float(b.abs().max()))


def test_lstm_reference_is_torch_lstmcell():
    g = S.gen(1)
    N, R, E = 6, 5, 7
    cell = torch.nn.LSTMCell(E, R).double()
    x, h, c = (torch.randn(N, k, generator=g, dtype=F64, requires_grad=True) for k in (E, R, R))
    h1, c1 = cell(x, (h, c))
    dh, dc = torch.randn(N, R, generator=g, dtype=F64), torch.randn(N, R, generator=g, dtype=F64)
    ((h1 * dh).sum() + (c1 * dc).sum()).backward()
    # the operands as the kernel receives them: one slab list per product, both biases, nothing else
    pre = S.presum(N, 4 * R, [((x @ cell.weight_ih.t()).detach()[None], 0), ((h @ cell.weight_hh.t()).detach()[None], 0)],
                   biases=[(cell.bias_ih.detach(), 0), (cell.bias_hh.detach(), 0)])
    hh, cc, _ = S.lstm_point(pre, c.detach())
    assert close(hh, h1.detach()) and close(cc, c1.detach())
    d_pre, d_c = S.cell_backward(S.lstm_point, pre, c.detach(), dh, dc)
    assert close(d_c, c.grad)
    assert close(d_pre @ cell.weight_ih.detach(), x.grad) and close(d_pre @ cell.weight_hh.detach(), h.grad)


def test_row_bias_and_fc_gates_indexing():
    g = S.gen(2)
    N, W = 10, 3
    rb = torch.randn(4, W, generator=g, dtype=F64)
    idx = torch.tensor([3, 0, 0, 2, 1, 3, 3, 0, 2, 1], dtype=torch.int32)
    assert torch.equal(S.presum(N, W, row_bias=rb, row_idx=idx), rb[idx.long()])
    assert torch.equal(S.presum(N, W, row_bias=rb, row_div=5), rb[:2].repeat_interleave(5, 0))
    assert torch.equal(S.presum(N, W, fc_gates=rb[:2], n=5), rb[:2].repeat_interleave(5, 0))


def _lin(g, o, i):
    return torch.randn(o, i, generator=g, dtype=F64) * 0.4, torch.randn(o, generator=g, dtype=F64)


def test_maxout_and_attention_references_are_the_att2in2_step():
    g = S.gen(3)
    B, n, K, R, E, A, V = 3, 2, 4, 5, 6, 7, 9
    N = B * n
    P = {'embed.0.weight': torch.randn(V, E, generator=g, dtype=F64)}
    for name, (o, i) in {'core.attention.h2att': (A, R), 'core.attention.alpha_net': (1, A), 'core.i2h': (5 * R, E),
                         'core.h2h': (5 * R, R), 'core.a2c': (2 * R, R), 'logit': (V, R)}.items():
        P[name + '.weight'], P[name + '.bias'] = _lin(g, o, i)
    it = torch.randint(0, V, (N,), generator=g)
    h, c = torch.randn(N, R, generator=g, dtype=F64), torch.randn(N, R, generator=g, dtype=F64)
    att, p_att = torch.randn(B, K, R, generator=g, dtype=F64), torch.randn(B, K, A, generator=g, dtype=F64)
    mask = torch.tensor([[1., 0, 0, 0], [1, 1, 1, 0], [1, 1, 1, 1]], dtype=F64)
    _, h_ref, c_ref = att2in2_ref64.step(P, it, h, c, att, p_att, mask, n)
    att_h = h @ P['core.attention.h2att.weight'].t() + P['core.attention.h2att.bias']
    ctx, alpha, _ = S.attention_fwd(att_h, p_att, att, mask, P['core.attention.alpha_net.weight'].reshape(-1),
                                    P['core.attention.alpha_net.bias'], torch.arange(N) // n)
    assert close(alpha.sum(1), torch.ones(N, dtype=F64)) and float(alpha[:n, 1:].abs().max()) == 0.0
    xt = torch.relu(P['embed.0.weight'][it])
    pre = S.presum(N, 5 * R, [((xt @ P['core.i2h.weight'].t())[None], 0), ((ctx @ P['core.a2c.weight'].t())[None], 3 * R)],
                   addend=h @ P['core.h2h.weight'].t(),
                   biases=[(P['core.i2h.bias'], 0), (P['core.h2h.bias'], 0), (P['core.a2c.bias'], 3 * R)])
    hh, cc, saved = S.maxout_point(pre, c)
    assert close(hh, h_ref) and close(cc, c_ref)
    assert torch.equal(saved[:, 3 * R:], pre[:, 3 * R:])


@pytest.mark.parametrize('maxout', [0, 1])
def test_adaatt_reference_is_the_adaatt_step(maxout):
    g = S.gen(4 + maxout)
    B, n, K, R, V = 2, 3, 4, 6, 9
    N, G = B * n, (5 if maxout else 4) * R
    P = {'embed.0.weight': torch.randn(V, R, generator=g, dtype=F64)}
    for name, (o, i) in {'core.lstm.w2h': (G, R), 'core.lstm.v2h': (G, R), 'core.lstm.h2h.0': (G, R), 'core.lstm.r_w2h': (R, R),
                         'core.lstm.r_v2h': (R, R), 'core.lstm.r_h2h': (R, R), 'core.attention.fr_linear.0': (R, R),
                         'core.attention.fr_embed': (R, R), 'core.attention.ho_linear.0': (R, R), 'core.attention.ho_embed': (R, R),
                         'core.attention.alpha_net': (1, R), 'core.attention.att2h': (R, R), 'logit': (V, R)}.items():
        P[name + '.weight'], P[name + '.bias'] = _lin(g, o, i)
    it = torch.randint(0, V, (N,), generator=g)
    h, c, fc = (torch.randn(k, R, generator=g, dtype=F64) for k in (N, N, B))
    att, p_att = torch.randn(B, K, R, generator=g, dtype=F64), torch.randn(B, K, R, generator=g, dtype=F64)
    _, h_ref, c_ref = adaatt_ref64.step(P, it, h, c, fc, att, p_att, None, n)
    xt = torch.relu(P['embed.0.weight'][it])
    lin = lambda k, x: x @ P[k + '.weight'].t() + P[k + '.bias']          # noqa: E731
    # as the driver lays it out: (w2h | r_w2h) and (h2h | r_h2h) stacked, the fc products with all biases folded into fc_gates
    xs = torch.cat([xt @ P['core.lstm.w2h.weight'].t(), xt @ P['core.lstm.r_w2h.weight'].t()], 1)
    hs = torch.cat([h @ P['core.lstm.h2h.0.weight'].t(), h @ P['core.lstm.r_h2h.weight'].t()], 1)
    bias = torch.cat([P['core.lstm.w2h.bias'] + P['core.lstm.h2h.0.bias'], P['core.lstm.r_w2h.bias'] + P['core.lstm.r_h2h.bias']])
    fcg = torch.cat([lin('core.lstm.v2h', fc), lin('core.lstm.r_v2h', fc)], 1) + bias
    pre = S.presum(N, G + R, [(hs[None], 0)], addend=xs, fc_gates=fcg, n=n)
    hh, cc, fake, saved = S.adaatt_point(pre, c, maxout)
    assert close(hh, h_ref) and close(cc, c_ref)
    assert close(fake, torch.sigmoid(pre[:, -R:]) * torch.tanh(c_ref)) and saved.shape == (N, G + R)


def test_attention_batched_reference_is_autograd():
    """the closed forms of the time-batched pass against autograd over T independent steps"""
    g = S.gen(6)
    T, B, n, K, A, R = 2, 2, 3, 4, 5, 6
    N = B * n
    img = torch.arange(N) // n
    lv = lambda *s: torch.randn(*s, generator=g, dtype=F64, requires_grad=True)        # noqa: E731
    p_att, att, w, b = lv(B, K, A), lv(B, K, R), lv(A), lv(1)
    att_h, d_ctx = torch.randn(T, N, A, generator=g, dtype=F64), torch.randn(T, N, R, generator=g, dtype=F64)
    al, de = [], []
    for t in range(T):
        ctx, a, e = S.attention_fwd(att_h[t], p_att, att, None, w, b, img)
        e.retain_grad()
        (ctx * d_ctx[t]).sum().backward()
        al.append(a.detach()); de.append(e.grad)
    d_att, d_p_att, d_w, d_b, rows = S.attention_batched(d_ctx, att_h, torch.stack(al), torch.stack(de), p_att.detach(), w.detach(), B, n)
    assert close(d_att, att.grad) and close(d_p_att, p_att.grad) and close(d_w, w.grad)
    assert float((d_b - b.grad).abs().max()) < 1e-12 and rows.shape == (B, K, A)


CELL_CASES = S.cell_rows()


@pytest.mark.parametrize('i', range(len(CELL_CASES)))
def test_cell_inputs_plant_the_extremes_and_saturate(i):
    """the inputs the GPU tests draw (same rows, same seeds)"""
    kind, N, R, s1, s2, flags, seed = CELL_CASES[i]
    d = S.cell_inputs(kind, N, R, s1, s2, flags, seed)
    pre, p = d['pre'], d['plant']
    want = S.extremes_row(R, d['gates'])
    assert float((pre[p] - want).abs().max()) <= 2e-3          # 1e4 +- an fp32 ulp of the compensating slab entry
    if N > 1:
        body = torch.cat([pre[:p], pre[p + 1:]])
        # standard deviation 3: >= 768 elements, and a bias shared by the rows is one draw per column (>= 16 columns, at most 2/3 of
        # the variance): the estimate scatters by a few per cent, 20 % is far outside it
        assert body.numel() >= 768 and 2.4 < float(body.std()) < 3.6
    point = {'lstm': S.lstm_point, 'maxout': S.maxout_point}.get(kind) or (lambda a, b: S.adaatt_point(a, b, kind == 'adaattmo'))
    for out in point(pre, d['c_prev'].double()):
        assert bool(torch.isfinite(out).all())


MAXOUT_ROWS = S.maxout_rows()


@pytest.mark.parametrize('i', range(len(MAXOUT_ROWS)))
def test_maxout_near_ties_stay_under_the_cap(i):
    """every maxout case row, forward and backward: the share of elements whose two chunks are closer than TIE (expected 4e-5 at
    these draws) stays under TIE_CAP, so the comparison of d_sums[3], d_sums[4] leaves next to nothing out"""
    kind, N, R, s1, s2, flags, seed = MAXOUT_ROWS[i]
    d = S.cell_inputs(kind, N, R, s1, s2, flags, seed)
    assert float(S.tie_mask(d['pre'], R).double().mean()) <= S.TIE_CAP
