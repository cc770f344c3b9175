"""capmi_xe_loss_fwd / _bwd (LanguageModelCriterion and LabelSmoothing as kernels, losses.py:204-265) without a GPU: the two
entry points exist through header, ctypes tables and the built library; CPU and float64 inputs keep the generic route and the
values of tests/golden/criteria.npz; the eligibility rule of the fused route, CAPMI_FUSED_XE=0 included."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, 'imagecaptioning', 'pytorch_amd'))
HEADER = os.path.join(ROOT, 'include', 'capmi.h')
NAMES = ('capmi_xe_loss_fwd', 'capmi_xe_loss_bwd')


def test_entry_points_are_declared_bound_and_exported():
    src = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    from imagecaptioning.pytorch_amd import _lib
    exported = subprocess.check_output(['nm', '-D', '--defined-only', _lib.LIB_PATH]).decode()
    for name in NAMES:
        assert re.search(r'\bint\s+%s\s*\(const capmi_xe_loss \*p, void \*stream\)\s*;' % name, src), name
        assert len(_lib.SIGNATURES[name]) == 2, name
        assert re.search(r' T %s\b' % name, exported), name
        assert getattr(_lib.lib, name).argtypes is not None
    # the ctypes mirror lists the fields of the header's struct in its order
    body = re.search(r'typedef struct capmi_xe_loss \{([^{}]*?)\} capmi_xe_loss;', src, flags=re.S).group(1)
    fields = [re.findall(r'(\w+)$', part.strip())[0] for stmt in body.split(';') if stmt.strip() for part in stmt.split(',')]
    assert fields == [f[0] for f in _lib.XeLoss._fields_]


CRIT = np.load(os.path.join(ROOT, 'tests', 'golden', 'criteria.npz'))


@pytest.mark.parametrize('name', ['lm', 'ls'])
@pytest.mark.parametrize('red', ['mean', 'none'])
@pytest.mark.parametrize('dtype', [torch.float64, torch.float32])
def test_cpu_inputs_keep_the_generic_route_and_its_values(name, red, dtype, monkeypatch):
    from captioning.modules import losses as L
    from imagecaptioning.pytorch_amd import ops
    monkeypatch.setattr(ops, 'xe_loss_fwd', lambda *a, **k: pytest.fail('a CPU tensor reached the kernel route'))
    x = torch.log_softmax(torch.from_numpy(CRIT['logits']), 2).to(dtype).requires_grad_(True)
    tgt, mask = torch.from_numpy(CRIT['target']), torch.from_numpy(CRIT['mask'])
    N = x.shape[0]
    if name == 'lm':
        loss = L.LanguageModelCriterion()(x, tgt, mask, reduction=red)
    else:
        loss = L.LabelSmoothing(smoothing=0.2)(x, tgt.view(N, -1), mask.view(N, -1), reduction=red)
    ref = torch.from_numpy(CRIT['%s_%s_loss' % (name, red)])
    tol = dict(rtol=1e-10, atol=1e-12) if dtype == torch.float64 else dict(rtol=1e-5, atol=1e-6)
    assert loss.dtype == dtype and loss.shape == ref.shape and torch.allclose(loss.double(), ref, **tol), (loss, ref)
    w = torch.linspace(0.5, 1.5, loss.numel(), dtype=dtype).view_as(loss) if red == 'none' else None
    (loss if w is None else (loss * w).sum()).backward()
    gtol = dict(rtol=1e-9, atol=1e-12) if dtype == torch.float64 else dict(rtol=1e-5, atol=1e-7)
    assert torch.allclose(x.grad.double(), torch.from_numpy(CRIT['%s_%s_grad' % (name, red)]), **gtol)


class _Fake:
    """the attributes of a tensor that the eligibility rule reads (no device is touched)"""

    def __init__(self, shape, dtype, cuda=True, requires_grad=False, strides=None, sink=None):
        self.shape, self.dtype, self.is_cuda, self.requires_grad = tuple(shape), dtype, cuda, requires_grad
        self.ndim = len(shape)
        self.device = torch.device('cuda', 0) if cuda else torch.device('cpu')
        if strides is None:
            strides, k = [], 1
            for s in reversed(shape):
                strides.insert(0, k)
                k *= s
        self._strides = tuple(strides)
        if sink is not None:
            self._capmi_sink = sink

    def stride(self, i):
        return self._strides[i]

    def is_contiguous(self):
        return _Fake(self.shape, self.dtype)._strides == self._strides


def test_eligibility_rule(monkeypatch):
    from imagecaptioning.pytorch_amd import sparse_logp as S
    monkeypatch.delenv('CAPMI_FUSED_XE', raising=False)
    monkeypatch.setattr(S, '_DENSE', False)
    f32, f64, i64 = torch.float32, torch.float64, torch.int64
    N, T, V1 = 4, 5, 11
    tok, mask = _Fake((N, T), i64), _Fake((N, T), f32)
    wide_tok, wide_mask = _Fake((N, T), i64, strides=(T + 2, 1)), _Fake((N, T + 2), f32)
    route = S.fused_xe_route
    assert route(_Fake((N, T, V1), f32), tok, mask) == 'forward'                       # validation loss: no gradient asked for
    assert route(_Fake((N, T, V1), f32), wide_tok, wide_mask, 0.1) == 'forward'        # cut views of wider buffers
    assert route(_Fake((N, T, V1), f32, requires_grad=True, sink=S.LogpSink()), tok, mask) == 'sink'
    assert route(_Fake((N, T, V1), f32, requires_grad=True, sink=S.LogpSink()), tok, mask, 0.1) == 'sink'
    with torch.no_grad():
        assert route(_Fake((N, T, V1), f32, requires_grad=True), tok, mask) == 'forward'
    # everything else keeps today's lines
    assert route(_Fake((N, T, V1), f32, requires_grad=True), tok, mask) is None        # wants a dense gradient
    taken = S.LogpSink()
    taken.sel_taken = True
    assert route(_Fake((N, T, V1), f32, requires_grad=True, sink=taken), tok, mask) is None
    summed = S.LogpSink()
    summed.sum_taken = True
    assert route(_Fake((N, T, V1), f32, requires_grad=True, sink=summed), tok, mask, 0.1) is None
    assert route(_Fake((N, T, V1), f32, requires_grad=True, sink=summed), tok, mask, 0.0) == 'sink'
    assert route(_Fake((N, T, V1), f32, cuda=False), _Fake((N, T), i64, cuda=False), _Fake((N, T), f32, cuda=False)) is None
    assert route(_Fake((N, T, V1), f64), tok, mask) is None
    assert route(_Fake((N, T, V1), f32, strides=(T * V1 * 2, V1 * 2, 2)), tok, mask) is None
    assert route(_Fake((N, 0, V1), f32), _Fake((N, 0), i64), _Fake((N, 0), f32)) is None
    assert route(_Fake((N, T, V1), f32), _Fake((N, T), torch.int32), mask) is None
    assert route(_Fake((N, T, V1), f32), _Fake((N, T - 1), i64), mask) is None
    assert route(_Fake((N, T, V1), f32), _Fake((N, T), i64, strides=(0, 1)), mask) is None      # an expanded row
    assert route(_Fake((N, T, V1), f32), tok, _Fake((N, T), f32, requires_grad=True)) is None
    assert route(_Fake((N, T, V1), f32), tok, mask, 1.0) is None
    assert route(_Fake((N, T, 1), f32), tok, mask, 0.1) is None
    # the switches
    monkeypatch.setenv('CAPMI_FUSED_XE', '0')
    assert route(_Fake((N, T, V1), f32), tok, mask) is None
    assert route(_Fake((N, T, V1), f32, requires_grad=True, sink=S.LogpSink()), tok, mask, 0.1) is None
    monkeypatch.setenv('CAPMI_FUSED_XE', '1')
    assert route(_Fake((N, T, V1), f32), tok, mask) == 'forward'
    monkeypatch.setattr(S, '_DENSE', True)
    assert route(_Fake((N, T, V1), f32), tok, mask) is None
