"""No GPU: the float64 restatement of capmi_gemm_f32 (tests/gemm_ref64.py) anchored to torch's own float64 linear algebra, the shape
of the case table, the descriptors the entry point has to refuse before any launch, and the route the planner (capmi_gemm_plan)
gives every row of the table."""
import ctypes as C
import os

import pytest
import torch
import torch.nn.functional as F

import gemm_ref64 as R
from conftest import ROOT

LIB = os.path.join(ROOT, 'imagecaptioning', 'pytorch_amd', 'libcapmi.so')


def _ref(c):
    t = R.draw(c)
    ref, mag = R.gemm64(c, t)
    return t, ref, mag


def _stored(c, t, s, which):
    """segment s's operand as stored, float64"""
    K, div, M, N = c['Ks'][s], c['divs'][s], c['M'], c['N']
    if which == 'A':
        rows, cols = ((M + div - 1) // div, K) if c['al'] == 0 else (K, M)
        return torch.as_strided(t['A'][s], (rows, cols), (cols + c['lda_pad'], 1), c['a_off']).double()
    rows, cols = (N, K) if c['bl'] == 0 else (K, N)
    return torch.as_strided(t['B'][s], (rows, cols), (cols + c['ldb_pad'], 1), 0).double()


@pytest.mark.parametrize('lda_pad,ldb_pad,a_off', [(0, 0, 0), (3, 5, 1)])
def test_gemm64_is_linear_for_row_major_operands(lda_pad, ldb_pad, a_off):
    c = R.make_case('nt', '-', 'kernel', 7, 9, 11, bias=True, lda_pad=lda_pad, ldb_pad=ldb_pad, a_off=a_off, seed=1)
    t, ref, _ = _ref(c)
    want = F.linear(_stored(c, t, 0, 'A'), _stored(c, t, 0, 'B'), t['bias'].double())
    assert torch.allclose(ref, want, rtol=0, atol=1e-12)


@pytest.mark.parametrize('al,bl', [(0, 1), (1, 0), (1, 1)])
def test_gemm64_is_addmm_for_the_other_layouts(al, bl):
    c = R.make_case('l', '-', 'kernel', 6, 10, 13, al=al, bl=bl, bias=True, lda_pad=2, ldb_pad=1, seed=2)
    t, ref, _ = _ref(c)
    A, B = _stored(c, t, 0, 'A'), _stored(c, t, 0, 'B')
    want = torch.addmm(t['bias'].double(), A.t() if al else A, B if bl else B.t())
    assert torch.allclose(ref, want, rtol=0, atol=1e-12)


@pytest.mark.parametrize('al,bl', [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_gemm64_walks_segments_like_a_concatenation_along_k(al, bl):
    c = R.make_case('seg', '-', 'kernel', 5, 8, (3, 32, 7, 4), al=al, bl=bl, seed=3)
    t, ref, _ = _ref(c)
    A = torch.cat([_stored(c, t, s, 'A').t() if al else _stored(c, t, s, 'A') for s in range(4)], 1)
    B = torch.cat([_stored(c, t, s, 'B') if bl else _stored(c, t, s, 'B').t() for s in range(4)], 0)
    assert torch.allclose(ref, A @ B, rtol=0, atol=1e-12)


def test_gemm64_row_sharing_is_repeat_interleave():
    """a_row_div replaces models/utils.py repeat_tensors: every stored row serves `div` consecutive operand rows; the last group may be
    partly filled"""
    c = R.make_case('div', '-', 'kernel', 11, 6, (8, 5), divs=(3, 1), seed=4)
    t, ref, _ = _ref(c)
    A0 = _stored(c, t, 0, 'A')
    assert A0.shape[0] == 4
    A = torch.cat([A0.repeat_interleave(3, 0)[:11], _stored(c, t, 1, 'A')], 1)
    want = F.linear(A, torch.cat([_stored(c, t, s, 'B') for s in range(2)], 1))
    assert torch.allclose(ref, want, rtol=0, atol=1e-12)


@pytest.mark.parametrize('acc', ['C', 'addend'])
def test_gemm64_epilogue_order(acc):
    """bias + bias2 + row_bias[(m // div) * N + n], then ReLU, then the mask, then the addend (or C's previous content at pitch ldc)"""
    c = R.make_case('epi', '-', 'kernel', 7, 4, 5, acc=acc, eoff=1, seed=5, **R.FULL)
    t, ref, mag = _ref(c)
    M, N = 7, 4
    pre = F.linear(_stored(c, t, 0, 'A'), _stored(c, t, 0, 'B'))
    rb = t['row_bias'][1:].double().view(2, N)
    prev = t[('addend' if acc == 'addend' else 'C')].double()
    off = 1 if acc == 'addend' else c['c_off']
    for m in range(M):
        for n in range(N):
            v = pre[m, n] + t['bias'][1 + n].double() + t['bias2'][1 + n].double() + rb[m // 5, n]
            v = max(v, 0.0) * t['mask'][1 + m * N + n].double() + prev[off + m * c['ldc'] + n]
            assert abs(float(v) - float(ref[m, n])) < 1e-12
    assert bool((mag >= ref.abs() - 1e-12).all())
    assert set(t['mask'].tolist()) <= {0.0, 2.0}


def test_gemm64_mag_is_the_formula_on_absolute_values():
    c = R.make_case('mag', '-', 'kernel', 6, 5, (4, 3), acc='addend', seed=6, **R.FULL)
    t = R.draw(c)
    ta = {k: [x.abs() for x in v] if isinstance(v, list) else v.abs() for k, v in t.items()}
    _, mag = R.gemm64(c, t)
    ref_abs, _ = R.gemm64(c, ta)
    assert torch.allclose(mag, ref_abs, rtol=0, atol=1e-12)


def test_measure_counts_a_wrong_masked_element():
    ref = torch.tensor([[1.0, 0.0]], dtype=torch.float64)
    mag = torch.tensor([[2.0, 0.0]], dtype=torch.float64)
    assert R.measure(torch.tensor([[1.5, 0.0]]), ref, mag) == 0.25
    assert R.measure(torch.tensor([[1.0, 1e-30]]), ref, mag) == float('inf')


def test_sentinel_is_finite_and_varied():
    s = R.sentinel(1000)
    assert bool(torch.isfinite(s).all()) and len(set(s.tolist())) == 101 and float(s.abs().max()) < 1


# ---- the table --------------------------------------------------------------------------------------------------------------------
def test_table_names_are_unique_and_routes_known():
    names = [c['name'] for c in R.CASES]
    assert len(names) == len(set(names))
    assert len(R.ROUTES) == 11
    assert {c['route'] for c in R.CASES} == set(R.ROUTES)
    assert {c['epi'] for c in R.CASES} == {'kernel', 'reduce', 'slabs'}


def test_table_has_a_kernel_and_a_reduce_row_with_everything_on_for_every_route_that_owns_an_epilogue():
    def full(c):
        return c['bias'] and c['bias2'] and c['row_bias'] == 5 and c['M'] % 5 and c['relu'] and c['mask'] and c['acc']
    for route in R.OWNS_EPILOGUE:
        rows = [c for c in R.CASES if c['route'] == route]
        for epi in ('kernel', 'reduce'):
            assert any(c['epi'] == epi and full(c) for c in rows), (route, epi)
        assert any(c['epi'] == 'slabs' for c in rows), route
        assert {c['acc'] for c in rows if full(c)} == {'C', 'addend'}, route
    half = [c for c in R.CASES if c['route'] == 'ares_x3_half']
    assert half and all(c['epi'] == 'reduce' and full(c) for c in half)
    # the element-wise forms: the reduce kernel and the swapped wide epilogue with every epilogue operand one float off
    for route, epi in (('x3', 'reduce'), ('x3w_swap', 'reduce'), ('x3w_swap', 'kernel')):
        assert any(c['route'] == route and c['epi'] == epi and full(c) and c['eoff'] == 1 and c['ldc'] % 4 and c['N'] % 4 == 0
                   for c in R.CASES), (route, epi)


def test_table_windows_pitches_and_edges():
    for c in R.CASES:
        assert c['c_off'] > 0 and c['ldc'] in (c['N'] + 12, c['N'] + 13), c['name']
        assert len(c['Ks']) <= R.MAX_SEG and all(k > 0 for k in c['Ks'])
        assert c['al'] == 0 or set(c['divs']) == {1}
        assert (c['epi'] == 'slabs') == c['defer']
    assert any(len(c['Ks']) == R.MAX_SEG and c['route'] == 'x3' for c in R.CASES)
    assert any(c['a_off'] == 1 and c['route'] == 't64x64' for c in R.CASES)
    for route in ('t64x64', 't128', 'ares_x3'):
        assert any(c['route'] == route and max(c['divs']) > 1 for c in R.CASES), route
    assert {(c['al'], c['bl']) for c in R.CASES if c['route'] == 'x3' and c['M'] == 516} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert any(c['route'] == 't128' and c['al'] == 1 and c['M'] % 4 for c in R.CASES)
    for route in ('lc', 'ares_x3', 'ares_f32'):
        assert {c['bl'] for c in R.CASES if c['route'] == route} == {0, 1}, route
    assert any(c['route'] == 'lc' and c['bcols'] for c in R.CASES)
    assert all(c['planes'] == (c['route'] == 'lc') for c in R.CASES)
    assert any(0 < c['Ks'][-1] % 32 < 4 for c in R.CASES)           # a last K tile with fewer than four valid k
    assert any(c['lda_pad'] and c['ldb_pad'] for c in R.CASES)


def test_table_rows_fit_the_flop_cap_and_the_workspace():
    for c in R.CASES:
        if c['route'] in R.CAP_EXEMPT:
            assert R.flops(c) <= 1.1 * R.CAP_EXEMPT[c['route']], c['name']
        else:
            assert R.flops(c) <= R.FLOP_CAP, (c['name'], R.flops(c))
        assert R.slab_floats_bound(c) <= R.WS_FLOATS, c['name']
    assert set(R.CAP_EXEMPT) == {'t64x128', 'ares_x3_half'}
    assert sum(R.flops(c) for c in R.CASES if c['route'] in R.CAP_EXEMPT) < 1.2e9


# ---- the argument contract: refused before any launch, so no device is needed ---------------------------------------------------------
FAKE = 0x7f0000100000         # never dereferenced: every descriptor below is refused while the host code validates it


@pytest.fixture(scope='module')
def capmi():
    if not os.path.exists(LIB):
        from imagecaptioning.pytorch_amd import build
        build.build(verbose=False)
    from imagecaptioning.pytorch_amd import _lib
    return _lib


def _desc(_lib, **over):
    d = _lib.GemmDesc()
    d.nseg, d.M, d.N, d.ldc, d.C = 1, 8, 8, 8, FAKE
    for s in range(4):
        d.seg[s].A, d.seg[s].B, d.seg[s].lda, d.seg[s].ldb, d.seg[s].K, d.seg[s].a_row_div = FAKE, FAKE, 64, 64, 64, 1
    for k, v in over.items():
        setattr(d, k, v)
    return d


def _bcol_desc(_lib, n_bcol=1, B=FAKE, ldb=8, n=8, **over):
    over.setdefault('b_layout', 1)
    d = _desc(_lib, n_bcol=n_bcol, **over)
    for i in range(min(max(n_bcol, 0), 3)):
        d.bcol_B[i], d.bcol_ldb[i], d.bcol_n[i] = B, ldb, n
    return d


def _plan(_lib, d):
    """(rc, route, splits, epi) of capmi_gemm_plan"""
    route, epi, splits = C.c_char_p(), C.c_char_p(), C.c_int(-1)
    rc = _lib.lib.capmi_gemm_plan(C.byref(d), C.byref(route), C.byref(splits), C.byref(epi))
    return rc, route.value and route.value.decode(), splits.value, epi.value and epi.value.decode()


def _refused(_lib, d):
    """by the call and by the planner alike, and the planner leaves the descriptor as it was"""
    before = bytes(d)
    return _plan(_lib, d) == (_lib.EINVAL, None, -1, None) and bytes(d) == before and \
        _lib.lib.capmi_gemm_f32(C.byref(d), None) == _lib.EINVAL


def test_gemm_refuses_bad_descriptors(capmi):
    L = capmi
    assert _refused(L, _desc(L, nseg=0))
    assert _refused(L, _desc(L, nseg=5))
    assert _refused(L, _desc(L, C=None))
    assert _refused(L, _desc(L, M=0)) and _refused(L, _desc(L, N=0))
    assert _refused(L, _desc(L, a_layout=2)) and _refused(L, _desc(L, b_layout=-1))
    for K in (0, -4):
        d = _desc(L)
        d.seg[0].K = K
        assert _refused(L, d)
    for which in ('A', 'B'):
        d = _desc(L, nseg=2)
        setattr(d.seg[1], which, None)
        assert _refused(L, d)
    d = _desc(L, a_layout=1)
    d.seg[0].a_row_div = 2
    assert _refused(L, d)


def test_gemm_refuses_bad_column_segments(capmi):
    L = capmi
    assert _refused(L, _bcol_desc(L, n_bcol=-1))
    assert _refused(L, _bcol_desc(L, n_bcol=4))
    assert _refused(L, _bcol_desc(L, nseg=2))
    assert _refused(L, _bcol_desc(L, b_layout=0))
    assert _refused(L, _bcol_desc(L, B=None))
    assert _refused(L, _bcol_desc(L, n=0))
    assert _refused(L, _bcol_desc(L, n=6, ldb=8, N=6))          # ncol % 4
    assert _refused(L, _bcol_desc(L, ldb=10))                   # ldb % 4
    assert _refused(L, _bcol_desc(L, ldb=4))                    # ldb < ncol
    assert _refused(L, _bcol_desc(L, B=FAKE + 4))               # 16-byte alignment
    assert _refused(L, _bcol_desc(L, N=12))                     # the segments do not add up to N
    assert _refused(L, _bcol_desc(L))                           # well formed, but without planes no kernel reads column segments


def test_gemm_refuses_a_deferred_call_whose_slabs_do_not_fit(capmi):
    L = capmi
    # (one float short of a single [M][N] slab: no K split the planner may choose fits)
    d = _desc(L, splits=2, defer_reduce=1, partial=FAKE, partial_capacity=R.COUNTER_FLOATS + 8 * 8 - 1)
    assert _refused(L, d)
    assert _refused(L, _desc(L, splits=2, defer_reduce=1))      # no workspace at all


# ---- the planner: every row's route, K split and epilogue place from the descriptor alone ---------------------------------------------
_BUFS = ('A', 'B', 'Bc', 'C', 'bias', 'bias2', 'row_bias', 'mask', 'addend', 'planes', 'ws')


class _Fake:
    """stands where a device tensor would: a 16-byte aligned address per buffer, 16 MB apart, never dereferenced"""

    def __init__(self, key, s=None):
        self.addr = FAKE + ((_BUFS.index(key) * R.MAX_SEG + (s or 0)) << 24)
        self.buf, self.capacity = self, R.COUNTER_FLOATS + R.WS_FLOATS          # (as a workspace)

    def data_ptr(self):
        return self.addr


def _fake_desc(c):
    planes = [_Fake('planes', s) for s in range(len(c['Ks']))] if c['planes'] else None
    return R.descriptor(c, _Fake, planes, _Fake('ws'))


@pytest.mark.parametrize('name', [c['name'] for c in R.CASES])
def test_plan_gives_every_row_its_route(capmi, name):
    c = R.BY_NAME[name]
    d = _fake_desc(c)
    assert (d.splits, d.defer_reduce, d.allow_wide_deferred) == (c['splits'], int(c['defer']), int(c['allow_wide']))
    assert all(bool(d.a_planes[s]) == c['planes'] for s in range(d.nseg)) and d.n_bcol == len(c['bcols'] or ())
    rc, route, splits, epi = _plan(capmi, d)
    assert rc == 0
    assert (route, epi) == (c['route'], c['epi'])
    assert 1 <= splits <= R.k_tiles(c)


def test_plan_does_not_write_the_descriptor(capmi):
    for c in R.CASES:
        d = _fake_desc(c)
        d.splits_used = -7
        before = bytes(d)
        assert _plan(capmi, d)[0] == 0
        assert bytes(d) == before and d.splits_used == -7, c['name']
    # out pointers are optional
    assert capmi.lib.capmi_gemm_plan(C.byref(d), None, None, None) == 0
