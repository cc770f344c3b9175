"""The float64 references of reduce_ref64.py, anchored outside themselves (torch.sum, index_add_, torch.optim.Adam), and the properties
of the shared case tables that test_reduce_kernels_gpu.py leans on: arm() of every row is the arm the row names, every required arm
is named by a row, the inputs are well conditioned for the relative metric, and the Adam bounds come from the float32 restatement.
No GPU."""
import pytest
import torch

import optim_ref64 as O
import reduce_ref64 as R

F64 = torch.float64


def close(a, b, tol=1e-12):
    return float((a - b).abs().max()) <= tol * (1.0 + float(b.abs().max()))


# ------------------------------------------------------------------------------------------------ the tables
@pytest.mark.parametrize('entry', sorted(R.TABLES))
def test_arm_of_every_row_is_the_arm_it_names(entry):
    for row in R.TABLES[entry]:
        assert R.arm(entry, row) == row[-1], (entry, row, R.arm(entry, row))


@pytest.mark.parametrize('entry', sorted(R.REQUIRED))
def test_every_required_arm_is_named_by_a_row(entry):
    missing = [t for t in R.REQUIRED[entry] if not R.names(entry, t)]
    assert not missing, (entry, missing)
    assert set(R.REQUIRED) == set(R.TABLES)


def test_dispatch_constants_of_the_issue_shapes():
    """the thresholds the rows were chosen around, restated from the sources"""
    assert R.colsum_rsplit(1100, 8) == 4 and R.colsum_rsplit(1023, 8) == 1 and R.colsum_rsplit(1024, 4096) == 1
    assert R.colsum_rsplit(6720, 512) == 16
    # deterministic embedding gradient: 64 B of static LDS beside the dynamic block; 12 272 positions are the last below 64 KB
    assert R.embed_bwd_det_lds(12272) + 64 == R.LDS_DEFAULT and R.embed_bwd_det_lds(12273) + 64 > R.LDS_DEFAULT
    assert R.embed_bwd_det_lds(R.EBD_MAX_ROWS) == 72 * 1024
    assert len(R.COLSUM_BATCH) == R.COLSUM_ARGS_MAX
    # adam2_kernel: a second trip of the outer loop needs more than 2 * 2048 * 256 quads = 4 buffers of more than 16 MiB: over 64 MB
    assert R._arm_adam((4 * 2 * R.GRID_CAP * 256 + 4,)) == 'adam2 two clamped trip2'
    assert 4 * 4 * (4 * 2 * R.GRID_CAP * 256 + 4) > 64 * 1024 * 1024


# ------------------------------------------------------------------------------------------------ sums
@pytest.mark.parametrize('i', range(len(R.COLSUM)))
def test_colsum_reference_is_torch_sum_and_float32_has_room(i):
    rows, cols, ld, off, acc, _ = R.COLSUM[i]
    x = R.pitched(rows, cols, ld, seed=i)
    assert bool(torch.isnan(x[:, cols:]).all()) and bool(torch.isfinite(x[:, :cols]).all())
    out0 = torch.randn(cols, generator=R.gen(100 + i)) if acc else None
    ref = R.colsum(x, cols, out0)
    want = torch.sum(x[:, :cols].contiguous().double(), 0) + (out0.double() if acc else 0)
    assert close(ref, want)
    f32 = torch.sum(x[:, :cols].contiguous(), 0) + (out0 if acc else 0)
    assert R.rel_err(f32, ref) * 2 < R.COLSUM_TOL, R.rel_err(f32, ref)


def test_colsum_batch_references_have_room():
    for i, (rows, cols, ld, off, acc, out2, _) in enumerate(R.COLSUM_BATCH):
        x = R.pitched(rows, cols, ld, seed=200 + i)
        out0 = torch.randn(cols, generator=R.gen(300 + i)) if acc else None
        ref = R.colsum(x, cols, out0)
        f32 = torch.sum(x[:, :cols].contiguous(), 0) + (out0 if acc else 0)
        assert R.rel_err(f32, ref) * 2 < R.COLSUM_TOL, (i, R.rel_err(f32, ref))


@pytest.mark.parametrize('i', range(len(R.GROUP_ROWSUM)))
def test_group_rowsum_reference_is_torch_sum_and_float32_has_room(i):
    c = R.GROUP_ROWSUM[i]
    T, groups, group, cols, pad_rows = c[:5]
    x = R.group_rowsum_input(c, seed=i)
    ref = R.group_rowsum(x, c)
    rows3 = x[:, :(groups * group + pad_rows) * cols].view(T, groups * group + pad_rows, cols)
    assert pad_rows == 0 or bool(torch.isnan(rows3[:, groups * group:]).all())
    want = torch.stack([torch.sum(rows3[:, k * group:(k + 1) * group].double().reshape(-1, cols), 0) for k in range(groups)])
    assert close(ref, want)
    f32 = torch.stack([torch.sum(rows3[:, k * group:(k + 1) * group].reshape(-1, cols), 0) for k in range(groups)])
    assert R.rel_err(f32, ref) * 2 < R.COLSUM_TOL


# ------------------------------------------------------------------------------------------------ embeddings
def test_embed_fwd_reference_is_the_module_forward():
    it, E, mask = R.embed_fwd_inputs(R.EMBED_FWD[3], seed=1)
    emb = torch.nn.Embedding(R.EMBED_V, E.shape[1]).double()
    with torch.no_grad():
        emb.weight.copy_(E)
        want = torch.relu(emb(it[:, 0])) * mask.double()
    assert torch.equal(R.embed_fwd(it, E.double(), mask, True), want)
    assert torch.equal(R.embed_fwd(it, E, None, False), E[it[:, 0]])


@pytest.mark.parametrize('i', range(len(R.EMBED_BWD)))
def test_embed_bwd_reference_is_index_add_and_autograd(i):
    rows, Ed, V = R.EMBED_BWD[i][:3]
    tok, dx, xs, m = R.embed_bwd_inputs(i)
    ref = R.embed_bwd(tok, dx, xs, m, V)
    gr = dx.double() * (m.double() if m is not None else 1.0) * ((xs > 0).double() if xs is not None else 1.0)
    want = torch.zeros(V, Ed, dtype=F64).index_add_(0, tok, gr)
    assert close(ref, want)
    if i == 0:                  # ... and what autograd gives for x = relu(E[tok]) * mask, x_saved = x
        E = torch.randn(V, Ed, generator=R.gen(9), dtype=F64, requires_grad=True)
        x = torch.relu(E[tok]) * m.double()
        (x * dx.double()).sum().backward()
        assert close(R.embed_bwd(tok, dx, x.detach().float(), m, V), E.grad)


def test_embed_bwd_tokens_of_the_long_case():
    rows, Ed, V, relu, mask, off, hot = R.EMBED_BWD[1][:7]
    tok = R.embed_tokens(rows, V, hot, 401)
    assert int((tok == 3).sum()) > 128                                  # the 8-in-flight loop runs
    assert int((tok == V - 1).nonzero().min()) >= 1024                  # a leader only the second pass of the scan finds
    assert (Ed + 255) // 256 == 2 and (Ed - 256) // 4 == 1              # blockIdx.y = 1 has one live lane


@pytest.mark.parametrize('i', range(len(R.EMBED_PE_BWD)))
def test_embed_pe_references_are_autograd_and_index_add(i):
    N, T, D, tok_ld, drop, V, _ = R.EMBED_PE_BWD[i]
    tok, E, pe, dr, dx = R.embed_pe_inputs(N, T, D, tok_ld, V, 600 + i, T + 2)
    dr = dr if drop else None
    ref = R.embed_pe_bwd(tok, dx, dr, T, V)
    gr = dx.double() * R.pe_scale(D) * (dr.double() if drop else 1.0)
    assert close(ref, torch.zeros(V, D, dtype=F64).index_add_(0, tok[:, :T].reshape(-1), gr.view(-1, D)))
    if N * T < 100:
        E64 = E.double().requires_grad_(True)
        x = (E64[tok[:, :T]] * R.pe_scale(D) + pe.double()[2:2 + T]) * (dr.double() if drop else 1.0)
        assert close(R.embed_pe_fwd(tok, E, pe, dr, T, 2)[0], x.detach())
        (x * dx.double()).sum().backward()
        assert close(ref, E64.grad)


# ------------------------------------------------------------------------------------------------ Jacobians
def test_relu_jacobians_are_autograd():
    dy, y, mask = R.relu_inputs(R.RELU_COUNT, seed=1)
    assert [float(v) for v in y[:3]] == [0.0, 0.0, float(torch.tensor(1e-30))] and bool(torch.signbit(y[1])) and float(y[2]) > 0
    pre = y.double().clone().requires_grad_(True)
    out = torch.relu(pre) * mask.double()
    (out * dy.double()).sum().backward()
    assert torch.equal(R.relu_mask_bwd(dy.double(), y, mask), pre.grad)
    # the scale form: y_ref is the output AFTER the mask, the mask's kept value is the scale
    assert torch.equal(R.relu_scale_bwd(dy.double(), out.detach(), 2.0), pre.grad)
    assert torch.equal(R.relu_mask_bwd(dy, None, None), dy)


# ------------------------------------------------------------------------------------------------ Adam
@pytest.mark.parametrize('name', sorted(R.ADAM_SETS))
def test_adam_reference_is_torch_optim_adam(name):
    hp, s = R.ADAM_HP, R.ADAM_SETS[name]
    p0, grads = R.adam_inputs(1003)
    ours = R.adam64(p0, grads, **s)
    lr, b1, b2, eps, wd, clip, scale = (O.f32(v) for v in (hp['lr'], hp['b1'], hp['b2'], hp['eps'], s['wd'], s['clip'], s['scale']))
    p = p0.double().clone().requires_grad_(True)
    opt = torch.optim.Adam([p], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
    for t, gr in enumerate(grads):
        gr = gr.double() * scale
        p.grad = gr.clamp(-clip, clip) if clip > 0 else gr
        opt.step()
        st = opt.state[p]
        assert close(ours[t][0], p.detach()) and close(ours[t][1], st['exp_avg']) and close(ours[t][2], st['exp_avg_sq'])


@pytest.mark.parametrize('name', sorted(R.ADAM_SETS))
def test_adam_bounds_come_from_the_float32_restatement(name):
    err = R.adam_f32_error(name)
    print('adam %s: float32 restatement rel_err p %.3e m %.3e v %.3e -> bounds %s' % ((name,) + err + (R.adam_bounds(name),)))
    assert all(1e-9 < e < 1e-6 for e in err), err           # units of float32 rounding (2^-24 = 6e-8), never zero
    bp, bm, bv = R.adam_bounds(name)
    assert (bm, bv) == (4 * err[1], 4 * err[2])
    assert bp == (1e-6 if name == 'clip' else 4 * err[0])
    if name == 'clip':
        assert err[0] * 4 < R.ADAM_P_TOL                    # the project's bound for p is the looser one


def test_step_record_formula():
    r = R.step_record(3)
    assert (r['epoch'], r['adam_step']) == (3, 3)
    b1, b2 = O.f32(0.9), O.f32(0.999)
    assert abs(float(r['bc1']) - (1 - b1 ** 3)) < 3e-8 and abs(float(r['bc2_sqrt']) - (1 - b2 ** 3) ** 0.5) < 4e-9      # half an ulp
