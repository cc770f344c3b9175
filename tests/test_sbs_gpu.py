"""Stochastic beam search on the device (csrc/sbs.hip, beam.stochastic_beam_search_steps, opt['sample_method'] = 'sbs') against the
float64 replay tests/sbs_ref64.py: one selection step with injected noise at every shape and variant, the backtrack, the whole
search on a tiny model of every family, and sampling in earnest with the in-kernel Philox noise.

Fixture seeds of the selection cases: the replay must separate the bd-th from the (bd+1)-th candidate of every image by more than
1e-3 (then the chosen set cannot depend on float32 rounding).  A case's seed is the first of seed0 + 100003 * i, i = 0, 1, ..., that
does so, with seed0 = 7919 * bd + 31 * V1 + 3 * B + cur + 1009 * variant + 500 * step0 (variant: its index in VARIANTS); the choice
reads the replay alone, never the device.  i = 0 serves 244 of the 246 cases and i = 1 the other two; two more shapes (bd = 16 at
V1 = 5 from the root) cannot supply bd candidates and are checked to be refused."""
import numpy as np
import pytest
import torch

import sbs_ref64 as S
from test_att_trace_host import tiny_opt

pytestmark = pytest.mark.gpu
DEV = 'cuda'
FAMILIES = ('updown', 'newfc', 'att2in2', 'adaatt', 'adaattmo', 'transformer', 'aoa')
VARIANTS = ('plain', 'dead', 'inf', 'force_end')
worst = {'phi': 0.0, 'g': 0.0}          # the largest errors of the selection cases (printed; DESIGN.md quotes them)


def _case(B, bd, V1, cur, variant, seed, step0=False):
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(B, cur, V1)) * 2.0
    if variant == 'inf' and V1 > 2:
        x[rng.random(size=x.shape) < 0.3] = -np.inf
        x[..., 1] = rng.normal(size=(B, cur))                                # every row keeps a finite column
    with np.errstate(divide='ignore'):
        logp = S.log_softmax(np.where(np.isneginf(x), -1e30, x)) + np.where(np.isneginf(x), -np.inf, 0.0)
    phi = -rng.uniform(0, 20, size=(B, cur))
    g = phi + rng.gumbel(size=(B, cur))
    alive = np.ones((B, cur), dtype=bool)
    if variant == 'dead':
        alive[:, rng.integers(0, cur)] = False
    if step0:
        phi[:], g[:] = 0.0, 0.0
    noise = rng.gumbel(size=(B, cur, V1))
    f32 = lambda a: a.astype(np.float32)                                     # noqa: E731
    return f32(logp), f32(phi), f32(g), alive, f32(noise)


LONG_V1 = 25601     # 26 chunks: at bd = 16 a row's lists take 3328 bytes, and only 14 of the 16 rows are staged at once


def _cases(bd, V1):
    """(B, cur, step0, variant) of one (bd, V1); variant None: the image cannot supply bd candidates and the call is refused"""
    if V1 == LONG_V1:                                                        # one case: the merge kernel's staging, not the variants
        yield 1, bd, False, 'plain'
        return
    for B in (1, 3):
        for cur, step0 in ((1, True), (bd, False)):
            if cur * V1 < bd:
                yield B, cur, step0, None
                continue
            for variant in VARIANTS:
                if variant == 'dead' and (step0 or V1 * (cur - 1) < bd - 1):
                    continue                                                 # the root is never dead; the others must fill the beam
                if variant == 'inf' and (V1 <= 2 or 0.5 * V1 * cur < 4 * bd):
                    continue                                                 # too few columns to block some and still fill the beam
                yield B, cur, step0, variant


def _fixture(B, bd, V1, cur, step0, variant):
    """the first seed of the documented sequence whose replay has a gap above 1e-3 -> (seed, its index, inputs, replay)"""
    seed0 = 7919 * bd + 31 * V1 + 3 * B + cur + 1009 * VARIANTS.index(variant) + (500 if step0 else 0)
    for i in range(50):
        seed = seed0 + 100003 * i
        inputs = _case(B, bd, V1, cur, variant, seed, step0)
        ref = S.select_step(*inputs, bd, step0=step0, force_end=variant == 'force_end')
        if ref['gap'].min() > 1e-3:
            return seed, i, inputs, ref
    raise AssertionError('no seed separates the candidates')


def _run_select(inputs, bd, step0, force_end, gumbel=True, **kw):
    from imagecaptioning.pytorch_amd import ops
    logp, phi, g, alive, noise = inputs
    B, cur, V1 = logp.shape
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)          # noqa: E731
    return ops.sbs_select(t(logp.reshape(B * cur, V1)), t(phi), t(g), t(alive.astype(np.uint8)), bd, step0=step0, force_end=force_end,
                          gumbel=t(noise.reshape(B * cur, V1)) if gumbel else None, **kw)


@pytest.mark.parametrize('bd', (1, 2, 5, 16))
@pytest.mark.parametrize('V1', ('bd', 5, 37, 257, 1031, LONG_V1))
def test_select_against_the_replay(bd, V1):
    """B in {1, 3}; the root step (cur = 1) and cur = bd; plain, one row not alive, -inf columns, force_end.  V1 = 25601: B = 1,
    cur = bd, plain only -- at bd = 16 the chunk lists of an image's rows no longer fit the merge kernel's LDS in one batch"""
    from imagecaptioning.pytorch_amd import _lib
    V1 = bd if V1 == 'bd' else V1
    used = []
    for B, cur, step0, variant in _cases(bd, V1):
        if variant is None:
            z = np.zeros((B, cur, V1), np.float32)
            with pytest.raises(_lib.CapmiError):
                _run_select((z, z[..., 0], z[..., 0], np.ones((B, cur), bool), z), bd, step0, False)
            continue
        seed, i, inputs, ref = _fixture(B, bd, V1, cur, step0, variant)
        used.append(i)
        parent, token, phi_o, g_o, alive_o = (x.cpu().numpy() for x in
                                              _run_select(inputs, bd, step0, variant == 'force_end'))
        what = (B, bd, V1, cur, step0, variant, seed)
        assert np.array_equal(parent, ref['parent']), what
        assert np.array_equal(token, ref['token']), what
        assert np.array_equal(alive_o.astype(bool), ref['alive']), what
        e_phi, e_g = np.abs(phi_o - ref['phi']).max(), np.abs(g_o - ref['g']).max()
        worst['phi'], worst['g'] = max(worst['phi'], float(e_phi)), max(worst['g'], float(e_g))
        print('sbs_select', what, 'max |phi err| %.3g  max |g err| %.3g' % (e_phi, e_g))
        assert e_phi <= 1e-4 and e_g <= 1e-4, what
        assert (np.diff(g_o, axis=1) <= 0).all(), what
        if variant == 'force_end':
            assert not alive_o.any()
        if variant == 'dead':                                        # the carried hypothesis: token 0, g bit for bit
            _, phi_in, g_in, alive_in, _ = inputs
            for b in range(B):
                j = int(np.flatnonzero(~alive_in[b])[0])
                hit = np.flatnonzero((parent[b] == j))
                assert len(hit) <= 1
                for q in hit:
                    assert token[b, q] == 0 and g_o[b, q].tobytes() == g_in[b, j].tobytes() and \
                        phi_o[b, q].tobytes() == phi_in[b, j].tobytes() and not alive_o[b, q]
    print('sbs_select worst so far', worst, 'seed indices', used)


def test_select_order_and_ties():
    """equal values: the lower flat index row * V1 + token first, at the root and across rows; no noise"""
    lp = np.log(np.array([0.1, 0.3, 0.05, 0.3, 0.25], dtype=np.float64)).astype(np.float32)
    zero = np.zeros((1, 1, 5), np.float32)
    one = (lp.reshape(1, 1, 5), np.zeros((1, 1), np.float32), np.zeros((1, 1), np.float32), np.ones((1, 1), bool), zero)
    parent, token, phi_o, g_o, alive_o = (x.cpu().numpy() for x in _run_select(one, 4, True, False))
    assert token.tolist() == [[1, 3, 4, 0]] and parent.tolist() == [[0] * 4] and alive_o.tolist() == [[1, 1, 1, 0]]
    assert g_o[0, 0] == g_o[0, 1] == lp[1] and np.array_equal(phi_o, g_o)
    # two identical rows below the root.  Columns 1 and 3 tie for the row maximum: both inherit g = 0.5 exactly (s = Z), so four
    # candidates are equal and come out by flat index
    def two(row):
        return (np.tile(row.reshape(1, 1, 5), (1, 2, 1)), np.full((1, 2), -1.0, np.float32), np.full((1, 2), 0.5, np.float32),
                np.ones((1, 2), bool), np.zeros((1, 2, 5), np.float32))
    parent, token, _, g_o, _ = (x.cpu().numpy() for x in _run_select(two(lp), 2, False, False))
    assert parent.tolist() == [[0, 0]] and token.tolist() == [[1, 3]] and g_o.tolist() == [[0.5, 0.5]]
    parent, token, _, g_o, _ = (x.cpu().numpy() for x in _run_select(two(lp), 4, False, False))
    assert parent.tolist() == [[0, 0, 1, 1]] and token.tolist() == [[1, 3, 1, 3]] and g_o.tolist() == [[0.5] * 4]
    # one maximum per row: the arg-maxes (g = 0.5) by row, then the rows' equal second children by row
    lp1 = np.log(np.array([0.1, 0.4, 0.05, 0.2, 0.25], dtype=np.float64)).astype(np.float32)
    parent, token, _, g_o, _ = (x.cpu().numpy() for x in _run_select(two(lp1), 4, False, False))
    assert parent.tolist() == [[0, 1, 0, 1]] and token.tolist() == [[1, 1, 4, 4]] and g_o[0, 1] == 0.5 and g_o[0, 2] == g_o[0, 3] < 0.5
    ref = S.select_step(*two(lp1), 4)
    assert ref['parent'].tolist() == parent.tolist() and ref['token'].tolist() == token.tolist()


def test_select_is_reproducible_and_seeded():
    """in-kernel Philox: the same (seed, offset) gives the same bits, another seed or offset another draw"""
    inputs = _case(3, 5, 1031, 5, 'plain', 4242)
    a = _run_select(inputs, 5, False, False, gumbel=False, seed=99, offset=3)
    b = _run_select(inputs, 5, False, False, gumbel=False, seed=99, offset=3)
    c = _run_select(inputs, 5, False, False, gumbel=False, seed=100, offset=3)
    d = _run_select(inputs, 5, False, False, gumbel=False, seed=99, offset=4)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert not torch.equal(a[3], c[3]) and not torch.equal(a[3], d[3])


@pytest.mark.parametrize('L', (1, 2, 7))
def test_backtrack_against_numpy(L):
    from imagecaptioning.pytorch_amd import ops
    B, bd = 3, 4
    rng = np.random.default_rng(50 + L)
    parent = np.zeros((L, B, bd), np.int32)
    token = np.zeros((L, B, bd), np.int64)
    alive = np.zeros((L, B, bd), np.uint8)
    prev = np.ones((B, 1), bool)
    for t in range(L):
        cur = prev.shape[1]
        parent[t] = rng.integers(0, cur, size=(B, bd))
        token[t] = rng.integers(0, 4, size=(B, bd))
        if t == 0:
            token[0, 0, 0] = 0                                               # a beam that ends at step 0 ...
        parent[t, 0, 0] = 0
        parent[t, 1, 1], token[t, 1, 1] = (1 if t else 0), 3                  # ... and one that runs to step L - 1
        was = prev[np.arange(B)[:, None], parent[t]]
        token[t][~was] = 0
        alive[t] = was & (token[t] != 0) & (t != L - 1)
        prev = alive[t].astype(bool)
    seq, length, lineage = (x.cpu().numpy() for x in ops.sbs_backtrack(*(torch.from_numpy(a).to(DEV) for a in (parent, token, alive))))
    want = S.backtrack(parent, token, alive)
    assert np.array_equal(seq, want[0]) and np.array_equal(length, want[1]) and np.array_equal(lineage, want[2])
    assert length[0] == 1 and length[1 * bd + 1] == L and (seq[bd + 1] == 3).all()
    assert seq.dtype == np.int64 and length.dtype == np.int32 and lineage.dtype == np.int32


# ---------------------------------------------------------------------------------------------------------------------------
# the whole search
# ---------------------------------------------------------------------------------------------------------------------------
B_, K_, L_, VOC = 3, 4, 6, 40


def _family(name):
    from imagecaptioning.pytorch_amd.captioning import models
    torch.manual_seed(31 + FAMILIES.index(name))
    opt = tiny_opt(name, vocab_size=VOC, rnn_size=32, input_encoding_size=32, att_hid_size=32, d_model=32, d_ff=64, seq_length=L_,
                   max_length=L_, vocab={str(i): 'w%d' % i for i in range(1, VOC + 1)})
    return models.setup(opt).to(DEV).eval()


def _feats():
    gen = torch.Generator().manual_seed(5)
    return torch.randn(B_, 20, generator=gen).to(DEV), torch.randn(B_, 5, 20, generator=gen).to(DEV)


def _sample(model, seed=11, **opt):
    fc, att = _feats()
    torch.manual_seed(seed)
    model._rng_calls = 0
    with torch.no_grad():
        return model(fc, att, None, opt=opt, mode='sample')


@pytest.mark.parametrize('name', FAMILIES)
def test_search_on_a_tiny_model(name):
    model = _family(name)
    seq, logp = _sample(model, sample_method='sbs', sample_n=K_)
    V1 = VOC + 1
    assert seq.shape == (B_ * K_, L_) and logp.shape == (B_ * K_, L_, V1) and seq.dtype == torch.long
    last = model.last_sbs
    assert sorted(last) == ['g', 'log_w', 'phi'] and all(v.shape == (B_, K_) and v.is_cuda for v in last.values())
    rows = seq.view(B_, K_, L_).cpu().tolist()
    for img in rows:
        assert len({tuple(r) for r in img}) == K_, img                      # pairwise distinct
        for r in img:                                                        # nothing behind the end token
            assert 0 not in r or not any(r[r.index(0):]), r
    assert (last['g'][:, 1:] <= last['g'][:, :-1]).all()
    np.testing.assert_allclose(last['phi'].cpu().numpy().reshape(-1), logp.gather(2, seq.unsqueeze(2)).squeeze(2).sum(1).cpu().numpy(),
                               rtol=1e-4)
    lw = last['log_w']
    assert lw.dtype == torch.float64 and torch.isneginf(lw[:, -1]).all() and torch.allclose(lw.exp().sum(1), lw.new_ones(B_))
    # the same seed: the same bits; another seed: another draw
    seq2, logp2 = _sample(model, sample_method='sbs', sample_n=K_)
    assert torch.equal(seq, seq2) and torch.equal(logp, logp2) and all(torch.equal(last[k], model.last_sbs[k]) for k in last)
    seq3, _ = _sample(model, seed=12, sample_method='sbs', sample_n=K_)
    assert not torch.equal(seq, seq3)
    # k = 1 is Gumbel-max sampling: the same injected noise, the same captions
    noise = torch.from_numpy(np.random.default_rng(9).gumbel(size=(L_, B_, V1)).astype(np.float32)).to(DEV)
    one, _ = _sample(model, sample_method='sbs', sample_n=1, _gumbel=noise)
    assert model.last_sbs['log_w'].tolist() == [[0.0]] * B_
    ref, _ = _sample(model, sample_method='gumbel', sample_n=1, _gumbel=noise)
    assert torch.equal(one, ref), (one, ref)
    assert model.last_sbs is None


@pytest.mark.parametrize('name', ('updown', 'adaatt'))
def test_search_with_constraints_and_attention(name):
    """the options of the beam path: rows renormalised under the constraints, the trace along the lineage"""
    model = _family(name)
    model.bad_endings_ix = [3, 4, 5]
    seq, logp = _sample(model, sample_method='sbs', sample_n=K_, decoding_constraint=1, remove_bad_endings=1, temperature=0.7,
                        return_attention=1)
    rows = seq.cpu().numpy()
    for r in rows:
        n = int((r != 0).sum()) if 0 in r else L_
        assert n < 2 or (r[1:n] != r[:n - 1]).all(), r                       # no word twice in a row
        if 0 in r and n > 0:
            assert r[n - 1] not in (3, 4, 5), r                              # no bad ending before the end token
    live = torch.cat([torch.ones_like(seq[:, :1]), (seq[:, :-1] != 0).long().cumprod(1)], 1).bool()      # steps up to the end token
    mass = logp.exp().sum(2)
    assert torch.allclose(mass[live], torch.ones_like(mass[live]), atol=1e-4) and (logp[~live] == 0).all()
    np.testing.assert_allclose(model.last_sbs['phi'].cpu().numpy().reshape(-1),
                               logp.gather(2, seq.unsqueeze(2)).squeeze(2).sum(1).cpu().numpy(), rtol=1e-4)
    att = model.last_attention['att']
    assert att.shape[:2] == (B_ * K_, L_)
    s = att.sum(2)
    assert torch.allclose(s[live], torch.ones_like(s[live]), atol=1e-4) and (s[~live] == 0).all()


def test_sampling_in_earnest():
    """4096 identical images over a table decoder, in-kernel Philox noise: the first row of every image is a sample from the model
    (each of the 21 sequences within 5 binomial standard deviations), and no image holds a sequence twice"""
    from imagecaptioning.pytorch_amd import beam
    from imagecaptioning.pytorch_amd.captioning.models.CaptionModel import CaptionModel

    class Bare(CaptionModel):
        _sbs_refusal = None
    V1, L, k, n = 5, 2, 2, 4096
    tree = S.make_tree(V1, L, seed=10, scale=0.5)           # chosen on the CPU: the rarest of the 21 sequences expects 60 of 4096
    seqs, p = S.sequences(tree)
    assert len(p) == 21 and p.min() * n >= 50
    model = Bare().eval()
    torch.manual_seed(3)
    seq, logp = beam.stochastic_beam_search_steps(model, lambda rows: S.TableDecoder(tree, n, rows, DEV), n, V1, L,
                                                  dict(sample_method='sbs', sample_n=k), DEV)
    rows = seq.view(n, k, L).cpu().numpy()
    assert (rows[:, 0] != rows[:, 1]).any(1).all()
    code = {tuple(s): i for i, s in enumerate(seqs.tolist())}
    first = np.bincount([code[tuple(r)] for r in rows[:, 0].tolist()], minlength=21)
    z = np.abs(first - n * p) / np.sqrt(n * p * (1 - p))
    print('sampling in earnest: max z', float(z.max()))
    assert z.max() <= 5.0, (int(z.argmax()), float(z.max()))
    np.testing.assert_allclose(model.last_sbs['phi'].cpu().numpy(), np.log(p)[[[code[tuple(r)] for r in img] for img in rows.tolist()]],
                               atol=1e-5)
