"""Every route of the capmi_gemm_f32 dispatcher (csrc/gemm_f32.hip) against the float64 restatement of its contract, on the case table
of tests/gemm_ref64.py: each kernel's own epilogue and operand fetch at the shapes where they can go wrong, output windows inside
a wider buffer, row sharing, segment and pitch edges, misaligned epilogue operands, and the route each row actually took.

The measure is element-wise: max |out - ref64| / mag over the window, mag being the same formula on absolute values.  The bound is
the project's rule for fp32-grade GEMMs (test_gemm_fat_bf16x3_is_fp32_grade): 1.5 x the same measure of a plain torch fp32 evaluation
of the same formula on the same device inputs, + 1e-7 -- measured against the vendor evaluation, never against the kernel."""
import os
import re
import subprocess
import sys

import pytest
import torch

import gemm_ref64 as R
from conftest import ROOT

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def ws(dev):
    from imagecaptioning.pytorch_amd import ops
    return ops.Workspace(dev, R.WS_FLOATS)


def _bits(x):
    return x.view(torch.int32)


@pytest.mark.parametrize('name', [c['name'] for c in R.CASES])
def test_gemm_route_vs_float64(dev, ws, name):
    """Measured on an MI355X, worst e_ours / bound per route: t32x128 0.66, t64x64 0.71, t64x128 0.40, t128 0.59, x3 0.69, x3w 0.84,
    x3w_swap 0.66, ares_x3 0.74, ares_f32 0.30, ares_x3_half 0.06, lc 0.38.  Row t64w_full_acc found the 64 x 128 configuration
    outside the bound (2.214e-07 against 1.5 x 7.154e-08 + 1e-7) while it summed all 2017 products of an element in one fp32
    accumulator chain; with its blocked summation (gemm_f32.hip, FLUSH) the row measures 8.146e-08."""
    c = R.BY_NAME[name]
    t = R.to_device(R.draw(c), dev)
    before = t['C'].clone()
    slabs = c['epi'] == 'slabs'
    ref, mag = R.evaluate(c, t, torch.float64, raw=slabs)
    f32, _ = R.evaluate(c, t, torch.float32, raw=slabs)
    from imagecaptioning.pytorch_amd import ops
    d = R.device_descriptor(c, t, ws)
    plan = ops.gemm_plan(d)
    splits = R.run(d)
    torch.cuda.synchronize()
    assert 1 <= splits <= R.k_tiles(c)
    # the planner, asked alone about the same descriptor, says what the call did
    assert plan == (c['route'], splits, c['epi'])
    # the ticket words in front of the slabs are zero again
    assert int(_bits(ws.buf[:R.COUNTER_FLOATS]).abs().max()) == 0
    after = t['C']
    if slabs:
        # a deferred call leaves C alone; its [splits][M][N] slabs sum to the raw product
        assert torch.equal(_bits(after), _bits(before))
        out = ws.slabs[:splits * c['M'] * c['N']].view(splits, c['M'], c['N']).double().sum(0)
    else:
        # every element outside the [M, N] window keeps the sentinel's bits
        a, b = after.clone(), before.clone()
        R.window(c, a).zero_()
        R.window(c, b).zero_()
        assert torch.equal(_bits(a), _bits(b)), 'wrote outside the window'
        out = R.window(c, after)
        assert bool(torch.isfinite(out).all())
    e_ours, e_f32 = R.measure(out, ref, mag), R.measure(f32, ref, mag)
    print('gemm_route %s route=%s epi=%s splits=%d e_ours=%.3e e_fp32=%.3e' % (name, c['route'], c['epi'], splits, e_ours, e_f32))
    assert e_ours <= 1.5 * e_f32 + 1e-7, (e_ours, e_f32)


def test_every_row_takes_the_route_it_names():
    """CAPMI_GEMM_LOG=1 prints one census line per successful capmi_gemm_f32 call; the k-th line belongs to the k-th row.  A planner
    change that moves a row off the route it was written for fails here.  (The knob is read once per process: a fresh child.)"""
    env = dict(os.environ, CAPMI_GEMM_LOG='1')
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'gemm_routes_child.py')], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    names = r.stdout.split()
    assert names == [c['name'] for c in R.CASES]
    lines = [m.group(1) for m in (re.match(r'capmi_gemm (.*)', ln) for ln in r.stderr.splitlines()) if m]      # (scripts/gemm_census.py)
    assert len(lines) == len(names), (len(lines), len(names))
    wrong, seen = [], set()
    for c, line in zip(R.CASES, lines):
        f = dict(kv.split('=') for kv in line.split())
        assert list(f)[:10] == ['M', 'N', 'tiles', 'al', 'bl', 'x3', 'wide', 'splits', 'defer', 'acc'], line
        assert (int(f['M']), int(f['N']), int(f['tiles'])) == (c['M'], c['N'], R.k_tiles(c)), (c['name'], line)
        if (f['route'], f['epi']) != (c['route'], c['epi']):
            wrong.append((c['name'], c['route'], c['epi'], line))
        seen.add(f['route'])
    assert not wrong, wrong
    assert seen == set(R.ROUTES)
