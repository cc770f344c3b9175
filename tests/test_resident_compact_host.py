"""The compact resident feature store on the host side (captioning/data/resident.py, --resident_dtype): the C ABI of
capmi_rows_narrow / capmi_resident_gather against its binding, the option and its start-up check, a CPU-device store per dtype against
the fp32 store rounded once, and the capacity of a budget at 16 bits."""
import os
import re
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
from test_abi import declared, HEADER
from test_feature_loader import make_dataset

PKG = os.path.join(ROOT, 'imagecaptioning', 'pytorch_amd')
TORCH = {'fp32': torch.float32, 'bf16': torch.bfloat16, 'fp16': torch.float16}


def _opts(argv):
    sys.path.insert(0, PKG)
    from captioning.utils import opts
    return opts.parse_opt(argv)


def _store(args, dtype, **kw):
    sys.path.insert(0, PKG)
    from captioning.data.feature_loader import FeatureLoader
    from captioning.data.resident import ResidentFeatures
    return ResidentFeatures(FeatureLoader(_opts(args + ['--batch_size', '4', '--seq_per_img', '3'])), 'cpu', dtype=dtype, **kw)


def test_prototypes_and_constants_match_the_binding():
    from imagecaptioning.pytorch_amd import _lib, ops, build
    d = declared()
    assert d['capmi_rows_l2norm'] == 4 == len(_lib.SIGNATURES['capmi_rows_l2norm'])
    assert int(re.search(r'#define CAPMI_ROWS_L2NORM_DMAX (\d+)', open(HEADER).read()).group(1)) == _lib.ROWS_L2NORM_DMAX
    assert d['capmi_rows_narrow'] == 5 == len(_lib.SIGNATURES['capmi_rows_narrow'])
    assert d['capmi_resident_gather'] == 10 == len(_lib.SIGNATURES['capmi_resident_gather'])
    src = open(HEADER).read()
    for name, val in (('F32', _lib.ROWS_F32), ('BF16', _lib.ROWS_BF16), ('FP16', _lib.ROWS_FP16)):
        assert int(re.search(r'#define CAPMI_ROWS_%s (\d+)' % name, src).group(1)) == val
    assert {k: v[1] for k, v in ops.ROWS_DTYPES.items()} == {'fp32': _lib.ROWS_F32, 'bf16': _lib.ROWS_BF16, 'fp16': _lib.ROWS_FP16}
    assert {k: v[0] for k, v in ops.ROWS_DTYPES.items()} == TORCH
    assert 'resident.hip' in [os.path.basename(s) for s in build.sources()]


def test_invalid_arguments_are_einval():
    """decided on the host before anything is launched: the pointers below are host buffers that are never dereferenced on the device"""
    from imagecaptioning.pytorch_amd import _lib
    buf = np.zeros(64, dtype=np.float32)
    p = buf.ctypes.data
    nar, gat = _lib.lib.capmi_rows_narrow, _lib.lib.capmi_resident_gather
    for a in ((None, p, 8, _lib.ROWS_BF16), (p, None, 8, _lib.ROWS_FP16), (p, p, 0, _lib.ROWS_BF16), (p, p, -1, _lib.ROWS_BF16),
              (p, p, 8, _lib.ROWS_F32), (p, p, 8, 3), (p + 2, p, 8, _lib.ROWS_BF16), (p, p + 1, 8, _lib.ROWS_BF16)):
        assert nar(*a, None) == _lib.EINVAL, a
    for a in ((None, 2, 8), (p, 0, 8), (p, -1, 8), (p, 2, 0), (p, 2, -4), (p, 2, _lib.ROWS_L2NORM_DMAX + 1), (p + 2, 2, 8)):
        assert _lib.lib.capmi_rows_l2norm(*a, None) == _lib.EINVAL, a
    tab = np.array([[1, 2], [3, 1]], dtype=np.int32)
    t = tab.ctypes.data
    ok = dict(rows=p, dtype=_lib.ROWS_BF16, F=4, th=t, t=t, B=2, kmax=2, att=p, mask=p)
    bad = [dict(rows=None), dict(th=None), dict(t=None), dict(att=None), dict(mask=None), dict(B=0), dict(B=-1), dict(kmax=0), dict(F=0),
           dict(F=-3), dict(dtype=3), dict(dtype=-1), dict(kmax=1), dict(rows=p + 1), dict(att=p + 2), dict(dtype=_lib.ROWS_F32, rows=p + 2)]
    for change in bad:
        a = dict(ok, **change)
        assert gat(a['rows'], a['dtype'], a['F'], a['th'], a['t'], a['B'], a['kmax'], a['att'], a['mask'], None) == _lib.EINVAL, change
    for neg in ([[1, -1], [3, 1]], [[-1, 2], [3, 1]]):
        th = np.array(neg, dtype=np.int32)
        assert gat(p, _lib.ROWS_BF16, 4, th.ctypes.data, t, 2, 2, p, p, None) == _lib.EINVAL, neg


def test_resident_dtype_option(capsys):
    sys.path.insert(0, PKG)
    from captioning.utils import opts
    from captioning.data.resident import ResidentFeatures
    assert opts.DEFAULTS['resident_dtype'] == 'fp32' and _opts([]).resident_dtype == 'fp32'
    assert _opts(['--resident_dtype', 'bf16']).resident_dtype == 'bf16' and _opts(['--resident_dtype', 'fp16']).resident_dtype == 'fp16'
    for bad in ('fp8', 'float16', ''):
        with pytest.raises(SystemExit):
            _opts(['--resident_dtype', bad])
        msg = capsys.readouterr().err
        assert all(n in msg for n in ('fp32', 'bf16', 'fp16')), msg
        with pytest.raises(ValueError, match='fp32.*bf16.*fp16'):
            ResidentFeatures(None, 'cpu', dtype=bad)


def test_tools_pass_the_option_to_the_store():
    for tool in ('train.py', 'eval.py'):
        text = open(os.path.join(PKG, 'tools', tool)).read()
        calls = re.findall(r'ResidentFeatures\(([^\n]*(?:\n[^\n]*)?)', text)
        assert calls and all('resident_dtype' in c for c in calls), tool


@pytest.fixture(scope='module')
def fp32_batches(tmp_path_factory):
    """the fp32 store's batches over three epochs of the ragged set (odd images have no fc file), computed once"""
    tmp = tmp_path_factory.mktemp('compact')
    args = make_dataset(tmp)
    res = _store(args, 'fp32', first_rows=8)
    n = 3 * ((len(res.split_ix['train']) + 3) // 4) + 1
    return args, [res.get_batch('train') for _ in range(n)], res


@pytest.mark.parametrize('dtype', ['fp32', 'bf16', 'fp16'])
def test_cpu_store_equals_the_fp32_batches_rounded_once(fp32_batches, dtype):
    args, want, ref = fp32_batches
    res = _store(args, dtype, first_rows=8)
    changed = False
    for it, x in enumerate(want):
        y = res.get_batch('train')
        changed |= not torch.equal(y['att_feats'], x['att_feats'])
        assert y['att_feats'].dtype == torch.float32
        assert torch.equal(y['att_feats'], x['att_feats'].to(TORCH[dtype]).float()), (it, dtype)
        assert torch.equal(y['fc_feats'], x['fc_feats']), (it, 'fc stays fp32, the mean of the fp32 rows where there is no fc file')
        assert (x['att_masks'] is None) == (y['att_masks'] is None)
        if x['att_masks'] is not None:
            assert torch.equal(x['att_masks'], y['att_masks']) and x['att_masks']._capmi_kmax == y['att_masks']._capmi_kmax
        assert torch.equal(x['labels'], y['labels']) and x['infos'] == y['infos']
    assert res.rows.dtype == TORCH[dtype] and res.fc.dtype == torch.float32
    assert res.streamed == 0 and res.misses == ref.misses and res.slot == ref.slot
    assert res.resident_bytes == ref.resident_bytes // (1 if dtype == 'fp32' else 2)
    assert changed == (dtype != 'fp32'), 'the features of the set are not representable at 16 bits: the rounding must show'


@pytest.mark.parametrize('dtype', ['bf16', 'fp16'])
def test_a_budget_of_r_fp32_rows_holds_2r_rows(tmp_path, dtype):
    """every image has 5 regions of 24 features; a budget of exactly r = 11 fp32 rows (the zero row + 2 images) holds 22 rows at 16
    bits (the zero row + 4 images) before anything is streamed"""
    args = make_dataset(tmp_path, fixed_regions=5)
    r = 11
    stores = {d: _store(args, d, budget_bytes=r * 24 * 4, first_rows=4) for d in ('fp32', dtype)}
    for res in stores.values():
        for _ in range(4):
            res.get_batch('train')
    wide, compact = stores['fp32'], stores[dtype]
    assert len(wide.slot) == 2 and wide.used == r and wide.resident_bytes == r * 24 * 4 and wide.streamed > 0
    assert len(compact.slot) == 4 and compact.used == 2 * r - 1 and compact.resident_bytes == (2 * r - 1) * 24 * 2
    assert compact.rows.shape[0] == 2 * r and compact.resident_bytes <= compact.budget_bytes
    assert sorted(compact.slot.values()) == [(1 + 5 * i, 5) for i in range(4)]
    # 16 draws over 7 images: the first four distinct images are resident, every draw of another one is streamed
    assert compact.streamed == compact.misses - 4 and compact.streamed < wide.streamed
    first = _store(args, dtype, budget_bytes=r * 24 * 4, first_rows=4)
    first.get_batch('train')                                  # one batch of 4 distinct images: all of them fit, none is streamed
    assert first.streamed == 0 and len(first.slot) == 4 and first.used == 21
