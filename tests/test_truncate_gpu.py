"""Min-p, epsilon, eta and locally typical sampling on a real MI355X: csrc/truncate.hip (capmi_truncate_rows) against the float64
restatement tests/truncate_ref64.py at every wave, workgroup, float4 and register-arm edge, the draw through capmi_select_logp,
the host loops of decode.py on every model family against a float64 replay, and the command line.

Bounds: the kept set and its size are exact -- the inputs carry their decision margins (truncate_ref64.check_margins) -- and q,
kept_mass and seqLogprobs are held to 5e-5, the bound of decode-option rows.  Seeds of the model cases: the
injected Gumbel noise is -log(-log u), u = torch.rand of the first seed 7000 + i (7100 + i with group_size 2) whose float64 replay separates the winner of
every live row and step from the runner-up by more than 1e-3; the choice reads the replay alone."""
import json
import math
import os

import pytest
import torch

import truncate_ref64 as R
from test_att_trace_host import tiny_opt

pytestmark = pytest.mark.gpu
DEV = 'cuda'
TOL = 5e-5
V1S = (1, 2, 5, 63, 64, 65, 257, 1023, 1024, 4099, 9488, 12288, 12292)
REG_MAX = 12288


def _lib():
    from imagecaptioning.pytorch_amd import _lib as L
    return L


def _place(x, off, ld, fill=float('nan')):
    """the rows of x in a device buffer of leading dimension ld that starts `off` floats behind a 16-byte boundary; the padding
    holds `fill` (a kernel that reads it shows NaN).  Returns (buffer, view [N, V1])"""
    N, V1 = x.shape
    buf = torch.full((off + N * ld + 4,), fill, dtype=torch.float32, device=DEV)
    assert buf.data_ptr() % 16 == 0
    view = buf[off:off + N * ld].view(N, ld)[:, :V1]
    view.copy_(x.to(DEV))
    return buf, view


def _run(x, kind, param, T, off=0, stream=False, unf=None, want_store=True):
    """one call on rows x [N, V1] (float32, CPU) -> dict of CPU results; ld, ld_q, store_ld > V1 and a multiple of 4"""
    L = _lib()
    N, V1 = x.shape
    ld = (V1 + 3) // 4 * 4 + 4
    xb, xv = _place(x, off, ld)
    qb, qv = _place(torch.zeros(N, V1), off, ld + 4, fill=7.0)
    sb, sv = _place(torch.zeros(N, V1), 0, ld + 8, fill=7.0)
    kept = torch.full((N,), -1, dtype=torch.int32, device=DEV)
    mass = torch.full((N,), -1.0, device=DEV)
    flags = None if unf is None else unf.to(DEV)
    rc = L.lib.capmi_truncate_rows(xv.data_ptr(), ld, qv.data_ptr(), ld + 4, N, V1, R.KIND_ID[kind] | (R.STREAM if stream else 0),
                                   float(param), float(T), kept.data_ptr(), mass.data_ptr(), sv.data_ptr() if want_store else None,
                                   ld + 8, L.ptr(flags), L.stream_ptr())
    assert rc == 0, rc
    torch.cuda.synchronize()
    pad_q = qb[off:off + N * (ld + 4)].view(N, ld + 4)[:, V1:]
    pad_s = sb[:N * (ld + 8)].view(N, ld + 8)[:, V1:]
    assert bool((pad_q == 7.0).all()) and bool((pad_s == 7.0).all())              # nothing is written behind a row
    return dict(q=qv.cpu(), kept=kept.cpu(), mass=mass.cpu(), store=sv.cpu(), q_dev=qv, hold=(xb, qb, sb))


def _against(got, x, kind, param, T, unf, what):
    """kept set and count exact, q and kept_mass within TOL, the store rows bit for bit; returns the worst errors"""
    ref = R.truncate_ref(x, kind, param, T)
    kept = torch.isfinite(got['q'])
    assert not bool(torch.isnan(got['q']).any()), what
    assert torch.equal(kept, ref['kept']), (what, (kept != ref['kept']).nonzero()[:8].tolist())
    assert torch.equal(got['kept'].long(), ref['count']), (what, got['kept'].tolist(), ref['count'].tolist())
    assert bool(torch.isneginf(got['q'][~kept]).all()), what
    eq = float((got['q'].double() - ref['q'])[kept].abs().max())
    em = float((got['mass'].double() - ref['mass']).abs().max())
    assert eq < TOL and em < TOL, (what, eq, em)
    flag = torch.ones(x.shape[0], 1) if unf is None else unf.float().view(-1, 1)
    want = torch.where(flag.bool(), x, x * 0.0)
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got['store']), nan), what
    assert torch.equal(got['store'].view(torch.int32)[~nan], want.view(torch.int32)[~nan]), what
    return eq, em


@pytest.mark.parametrize('V1', V1S)
def test_kernel_against_the_restatement(V1):
    """every rule with both parameters at both temperatures; N rotates through 1, 3, 7.  Rows on 16-byte boundaries run the register
    arm (V1 <= 12288) and, with CAPMI_TRUNCATE_STREAM, the streaming arm on the same rows: the two agree bit for bit.  The same rows
    one float off a 16-byte boundary run the streaming arm with a three-float head.  Every second call carries unfinished flags."""
    worst_q = worst_m = 0.0
    i = 0
    for kind in R.KINDS:
        for param in R.PARAMS[kind]:
            for T in (1.0, 0.7):
                N = (1, 3, 7)[(V1 + i) % 3]
                x = R.rows_for(N, V1, kind, param, T, 1000 * V1 + i)
                unf = torch.tensor(([1, 0, 1, 1, 0, 1, 1])[:N], dtype=torch.uint8) if i % 2 else None
                what = (V1, kind, param, T, N)
                a = _run(x, kind, param, T, unf=unf)
                eq, em = _against(a, x, kind, param, T, unf, what + ('aligned',))
                worst_q, worst_m = max(worst_q, eq), max(worst_m, em)
                if V1 <= REG_MAX:
                    b = _run(x, kind, param, T, stream=True, unf=unf)
                    for k in ('q', 'mass', 'kept'):
                        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), what + ('arms differ in', k)
                    _against(b, x, kind, param, T, unf, what + ('stream',))
                c = _run(x, kind, param, T, off=1, unf=unf)
                eq, em = _against(c, x, kind, param, T, unf, what + ('one float off',))
                worst_q, worst_m = max(worst_q, eq), max(worst_m, em)
                i += 1
    print('truncate V1 %d: worst |q - q64| %.3g, worst |kept_mass - mass64| %.3g' % (V1, worst_q, worst_m))


@pytest.mark.parametrize('V1', (5, 64, 4099))
def test_uniform_one_hot_and_barred_rows(V1):
    for kind in R.KINDS:
        for param in R.PARAMS[kind] + ((1.0,) if kind == 'minp' else ()):
            for T in (1.0, 0.7):
                x = R.special_rows(V1)
                x[3:] = R.plant(x[3:].double(), kind, param, T, R.gen(V1))
                for off, stream in ((0, False), (0, True), (1, False)):
                    got = _run(x, kind, param, T, off=off, stream=stream)
                    _against(got, x, kind, param, T, None, (V1, kind, param, T, off, stream))
                    assert got['kept'][:3].tolist() == [V1, 1, 1]
                    assert float((got['q'][0] + math.log(V1)).abs().max()) < TOL and float(got['q'][1, V1 // 2]) == 0.0
                    assert not bool(torch.isfinite(got['q'][3][torch.isneginf(x[3])]).any())


def test_minp1_is_the_arg_max():
    x = R.rows_for(7, 4099, 'minp', 0.5, 1.0, 5)
    for off in (0, 1):
        got = _run(x, 'minp', 1.0, 0.7, off=off)
        assert got['kept'].tolist() == [1] * 7 and torch.equal(got['q'].argmax(1), x.argmax(1))
        assert bool((got['q'].max(1)[0] == 0.0).all()) and float((got['mass'].double() - R.truncate_ref(x, 'minp', 1.0, 0.7)['mass']).abs().max()) < TOL


def test_bad_arguments():
    L = _lib()
    N, V1 = 3, 40
    x = torch.randn(N, V1, device=DEV)
    q = torch.empty(N, V1, device=DEV)
    st = torch.empty(N, V1, device=DEV)

    def call(**kw):
        a = dict(logp=x.data_ptr(), ld=V1, q=q.data_ptr(), ld_q=V1, N=N, V1=V1, kind=0, param=0.5, T=1.0, store=None, store_ld=0)
        a.update(kw)
        return L.lib.capmi_truncate_rows(a['logp'], a['ld'], a['q'], a['ld_q'], a['N'], a['V1'], a['kind'], a['param'], a['T'], None, None,
                                         a['store'], a['store_ld'], None, L.stream_ptr())
    assert call() == 0 and call(store=st.data_ptr(), store_ld=V1) == 0 and call(N=0) == 0
    for bad in (dict(logp=None), dict(q=None), dict(ld=V1 - 1), dict(ld_q=V1 - 1), dict(V1=0), dict(N=-1), dict(kind=4), dict(kind=-1),
                dict(param=0.0), dict(param=-0.5), dict(param=float('nan')), dict(param=1.5), dict(kind=1, param=1.0),
                dict(kind=2, param=1.0), dict(kind=3, param=1.0), dict(T=0.0), dict(T=-1.0), dict(T=float('nan')),
                dict(q=x.data_ptr()), dict(q=x.data_ptr() + 4 * V1 * (N - 1)), dict(store=st.data_ptr(), store_ld=V1 - 1),
                dict(store=x.data_ptr(), store_ld=V1), dict(store=q.data_ptr(), store_ld=V1), dict(logp=x.data_ptr() + 2)):
        assert call(**bad) == L.EINVAL, bad
    assert call(kind=0, param=1.0) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ the draw
@pytest.mark.parametrize('kind,off', [('minp', 0), ('eps', 1), ('eta', 0), ('typ', 1), ('typ', 0)])
def test_philox_draws_match_the_truncated_distribution(kind, off):
    """test_philox_sampling_matches_the_filtered_distribution of test_select_gpu.py on q: V1 = 16, 4096 rows x 8 seeds = 32768 draws,
    T = 0.7; frequencies within 0.01 of exp(q64) (3.6 sigma of the largest binomial deviation at 32768 draws) and exactly 0 outside
    the kept set"""
    L = _lib()
    V1, N, T = 16, 4096, 0.7
    param = {'minp': 0.05, 'eps': 0.02, 'eta': 0.05, 'typ': 0.9}[kind]
    row = R.rows_for(1, V1, kind, param, T, 13, scale=1.0)
    ref = R.truncate_ref(row, kind, param, T)
    kept = ref['kept'][0]
    assert 4 <= int(kept.sum()) <= 6
    got = _run(row.repeat(N, 1), kind, param, T, off=off, want_store=False)
    q = got['q_dev'].contiguous()
    seq = torch.zeros(N, 1, dtype=torch.long, device=DEV)
    it = torch.zeros(N, dtype=torch.long, device=DEV)
    unf = torch.ones(N, dtype=torch.uint8, device=DEV)
    counts = torch.zeros(V1)
    for s in range(8):
        L.check(L.lib.capmi_select_logp(q.data_ptr(), N, V1, 0, 1, 1, 1.0, None, 1234 + s, seq.data_ptr(), 1, it.data_ptr(), unf.data_ptr(),
                                        None, None, 0, None, L.stream_ptr()), 'capmi_select_logp')
        counts += torch.bincount(seq[:, 0].cpu(), minlength=V1).float()
    freq = counts / counts.sum()
    want = ref['q'][0].exp().float()
    print('%s: max |freq - want| %.4f' % (kind, float((freq - want).abs().max())))
    assert float((freq - want).abs().max()) < 0.01
    assert float(freq[~kept].max()) == 0.0


# ------------------------------------------------------------------------------------------------ the models
B_, N_, L_, VOC = 2, 2, 6, 12
V1_ = VOC + 1
RULE = {'updown': 'typ0.8', 'newfc': 'minp0.2', 'att2in2': 'eps0.05', 'adaatt': 'eta0.1', 'transformer': 'typ0.6', 'aoa': 'minp0.5'}
FAMILIES = tuple(RULE)


def _model(name):
    from imagecaptioning.pytorch_amd.captioning import models
    torch.manual_seed(50 + FAMILIES.index(name))
    model = models.setup(tiny_opt(name)).to(DEV).eval()
    model.bad_endings_ix = [3, 5]
    gen = torch.Generator().manual_seed(8)
    return model, torch.randn(B_, 20, generator=gen).to(DEV), (torch.randn(B_, 4, 20, generator=gen) * 0.7).to(DEV)


def _noise(seed, shape):
    u = torch.rand(shape, generator=torch.Generator().manual_seed(seed)).clamp_min(1e-20)
    return -torch.log(-torch.log(u))


def _replay(model, fc, att, method, T, noise, rows=N_, **opts):
    from imagecaptioning.pytorch_amd.captioning.models.utils import parse_truncation
    kind, param = parse_truncation(method)
    with torch.no_grad():
        st = model._decode_stepper(fc, att, None, L_)(rows)
        return R.sample_loop(lambda t, it: st.step(t, it.to(DEV), rows).clone().cpu(), B_ * rows, B_, V1_, L_, kind, param, T, noise,
                             bad_endings=model.bad_endings_ix, **opts)


def _case(model, fc, att, method, T, **opts):
    """the first noise whose float64 replay has a winner gap above 1e-3 at every live row and step"""
    for i in range(20):
        noise = _noise(7000 + i, (L_, B_ * N_, V1_))
        seq, lps, was, gap = _replay(model, fc, att, method, T, noise, **opts)
        if gap > 1e-3:
            return noise, seq, lps, was, gap
    raise AssertionError('no seed separates the winners')


def _check_model(name, method, T, **opts):
    model, fc, att = _model(name)
    noise, seq64, lps, was, gap = _case(model, fc, att, method, T, **opts)
    assert gap > 1e-3                                                                 # on the replay alone
    with torch.no_grad():
        seq, logp = model(fc, att, None, opt=dict(opts, sample_method=method, temperature=T, sample_n=N_, _gumbel=noise.to(DEV)),
                          mode='sample')
    assert seq.shape == (B_ * N_, L_) and logp.shape == (B_ * N_, L_, V1_)
    assert torch.equal(seq.cpu(), seq64), (name, method, seq.cpu().tolist(), seq64.tolist())
    # seqLogprobs: the constrained log-softmax of the stepper on the steps a row was unfinished (finite entries; a constraint's -inf
    # stays -inf), logprobs * 0 behind them
    got, live = logp.double().cpu(), was[:, :, None].expand_as(lps)
    fin = torch.isfinite(lps) & live
    assert torch.equal(torch.isneginf(got) & live, torch.isneginf(lps) & live)
    err = float((got - lps)[fin].abs().max())
    print('%s %s T %s: winner gap %.3g, max |seqLogprobs - log_softmax64| %.3g' % (name, method, T, gap, err))
    assert err < TOL
    dead = ~live & torch.isfinite(lps)
    assert bool((got[dead] == 0).all())
    return model, fc, att, noise, seq


@pytest.mark.parametrize('name', FAMILIES)
def test_family_against_the_float64_replay(name):
    _check_model(name, RULE[name], 0.7 if name in ('updown', 'aoa') else 1.0)


@pytest.mark.parametrize('method', ('minp0.3', 'eps0.04', 'eta0.15'))
def test_updown_runs_every_rule(method):
    _check_model('updown', method, 1.0)


def test_constraints_and_trigram_blocking_come_before_the_rule():
    _check_model('updown', 'typ0.8', 1.0, decoding_constraint=1, block_trigrams=1, remove_bad_endings=1)


def test_minp1_is_greedy():
    model, fc, att = _model('att2in2')
    noise = _noise(3, (L_, B_ * N_, V1_)).to(DEV)
    with torch.no_grad():
        seq, logp = model(fc, att, None, opt={'sample_method': 'minp1', 'sample_n': N_, '_gumbel': noise}, mode='sample')
        greedy, glogp = model(fc, att, None, opt={'sample_method': 'greedy', 'sample_n': N_}, mode='sample')
    assert torch.equal(seq, greedy) and float((logp - glogp).abs().max()) < TOL


def test_group_size_two():
    model, fc, att = _model('updown')
    from imagecaptioning.pytorch_amd.captioning.models.utils import parse_truncation
    G, T, lam, method = 2, 0.8, 0.6, 'typ0.8'
    kind, param = parse_truncation(method)
    for i in range(20):
        noise = _noise(7100 + i, (L_, G, B_, V1_))
        with torch.no_grad():
            st = model._decode_stepper(fc, att, None, L_)(G)
            seq64, slp64, gap = R.diverse_loop(lambda t, it: st.step(t, it.to(DEV), G).clone().cpu(), B_, G, V1_, L_, kind, param, T, lam,
                                               noise)
        if gap > 1e-3:
            break
    assert gap > 1e-3
    with torch.no_grad():
        seq, slp = model(fc, att, None, opt={'sample_method': method, 'group_size': G, 'temperature': T, 'diversity_lambda': lam,
                                             '_gumbel': noise.to(DEV)}, mode='sample')
    assert seq.shape == (B_ * G, L_) and slp.shape == (B_ * G, L_)
    assert torch.equal(seq.cpu(), seq64), (seq.cpu().tolist(), seq64.tolist())
    err = float((slp.double().cpu() - slp64).abs().max())
    print('group_size 2: winner gap %.3g, max |sel_logp - q64[token]| %.3g' % (gap, err))
    assert err < TOL


def test_return_attention_and_in_kernel_noise():
    """the recording stepper, and draws with the kernel's own Philox: every token lies in the float64 kept set of its step"""
    model, fc, att = _model('updown')
    torch.manual_seed(4)
    with torch.no_grad():
        seq, logp = model(fc, att, None, opt={'sample_method': 'eps0.05', 'sample_n': 3, 'return_attention': 1}, mode='sample')
    assert seq.shape == (B_ * 3, L_) and model.last_attention is not None
    p = torch.softmax(logp.double().cpu(), 2)
    for r in range(B_ * 3):
        for t in range(L_):
            if t > 0 and seq[r, t - 1] == 0:
                break
            tok = int(seq[r, t])
            assert tok == int(p[r, t].argmax()) or float(p[r, t, tok]) >= 0.05 * (1 - 1e-3), (r, t, tok, float(p[r, t, tok]))


# ------------------------------------------------------------------------------------------------ the command line
def test_eval_entrypoint_sample_n_with_eta(tmp_path):
    """tools/eval.py on the synthetic split: --sample_n 3 --sample_n_method eta0.002 --language_eval 1 writes the single-caption file
    and the _n.json of eval_multi with its usual fields"""
    from test_langeval_gpu import SMALL, _opts
    from imagecaptioning.pytorch_amd.tools import eval as E
    out_dir = tmp_path / 'eta'
    loss, preds, lang_stats = E.main(_opts(SMALL + ['--num_images', '6', '--language_eval', '1', '--split', 'val', '--eval_results_dir',
                                                    str(out_dir), '--sample_n', '3', '--sample_n_method', 'eta0.002']))
    assert loss == loss and len(preds) >= 6 and all(math.isfinite(v) for v in lang_stats.values())
    assert sorted(os.listdir(out_dir)) == ['capmi_val.json', 'capmi_val_n.json']
    out = json.load(open(out_dir / 'capmi_val_n.json'))
    assert set(out) == {'div_stats', 'self_cider', 'oracle'} and len(out['self_cider']['imgToEval']) == 6      # SMALL asks for the oracle
    for v in out['div_stats']['ImgToEval'].values():
        assert len(v['individuals']) == 3 and all(isinstance(c['caption'], str) for c in v['individuals'])
