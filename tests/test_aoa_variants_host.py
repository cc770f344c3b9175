"""AoANet's ablation switches (AoAModel.py:100-226) on the host: construction, the reference's parameter tree for every variant of
tests/golden/aoa_variants.npz (keys in registration order, shapes, a strict load_state_dict), the refusals that stay, and the
layout of the new C struct.  No GPU: nothing is computed."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT

import aoa_variants_ref64 as V

TAGS = sorted(V.VARIANTS)


@pytest.fixture(scope='module')
def fixture():
    return np.load(os.path.join(GOLDEN, 'aoa_variants.npz'))


@pytest.mark.parametrize('tag', TAGS)
def test_variant_constructs_with_the_references_parameter_tree(fixture, tag):
    from imagecaptioning.pytorch_amd.captioning import models
    model = models.setup(V.variant_opt(tag))
    keys, shapes, _, _, _ = V.fixture_variant(fixture, tag)
    sd = model.state_dict()
    assert list(sd) == keys
    assert [n for n, _ in model.named_parameters()] == keys
    for k in keys:
        assert tuple(sd[k].shape) == shapes[k], k
    want = V.variant_opt(tag)
    assert ('fc_embed.0.weight' in sd) == (not want.mean_feats)
    assert any(k.startswith('refiner.') for k in sd) == bool(want.refine)
    res = model.load_state_dict(V.load_weights(fixture, tag), strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    for k, w in V.load_weights(fixture, tag).items():
        assert torch.equal(model.state_dict()[k], w), k
    # the flat-buffer groups name only parameters that exist
    names = set(keys)
    for grp in model._flat_groups():
        assert set(grp) <= names, grp
    assert bool(model._flat_groups()) == bool(want.refine)


@pytest.mark.parametrize('key,value', [('use_multi_head', 0), ('multi_head_scale', 2)])
def test_unsupported_attention_options_still_raise_and_name_the_option(key, value):
    from imagecaptioning.pytorch_amd.captioning import models
    with pytest.raises(NotImplementedError, match=key):
        models.setup(V.variant_opt('A', **{key: value}))


def test_ctx_step_struct_matches_header():
    """field order of _lib.CtxStep == capmi_ctx_step in include/capmi.h (parsed as tests/test_abi.py parses the others)"""
    from imagecaptioning.pytorch_amd import _lib
    src = open(os.path.join(ROOT, 'include', 'capmi.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    body = re.search(r'typedef struct (?:capmi_ctx_step )?\{([^{}]*?)\} capmi_ctx_step;', src, flags=re.S).group(1)
    names = []
    for stmt in body.split(';'):
        for part in stmt.strip().split(',') if stmt.strip() else []:
            names.append(re.findall(r'(\w+)\s*(?:\[\w+\])?$', part.strip())[0])
    assert names == [f[0] for f in _lib.CtxStep._fields_]
    for name in ('GLU', 'RELU', 'LSTM'):
        assert int(re.search(r'#define CAPMI_CTX_%s (\d+)' % name, src).group(1)) == getattr(_lib, 'CTX_' + name)
    assert {'capmi_ctx_fwd_fused', 'capmi_relu_bwd_add'} <= set(_lib.SIGNATURES)


def test_opts_carry_the_switches_to_the_model():
    from imagecaptioning.pytorch_amd.captioning.utils import opts
    o = opts.parse_opt(['--caption_model', 'aoa', '--decoder_type', 'LSTM', '--out_res', '1', '--ctx_drop', '0', '--mean_feats', '0',
                        '--refine', '0', '--refine_aoa', '0', '--use_ff', '1'])
    assert (o.decoder_type, o.out_res, o.ctx_drop, o.mean_feats, o.refine, o.refine_aoa, o.use_ff) == ('LSTM', 1, 0, 0, 0, 0, 1)
    assert opts.DEFAULTS['out_res'] == 0 and opts.DEFAULTS['decoder_type'] == 'AoA'
