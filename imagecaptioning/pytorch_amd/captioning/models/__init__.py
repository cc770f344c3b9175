"""Model factory (reference captioning/models/__init__.py:20-73), hot-path models only."""
from .AttModel import AttModel, UpDownModel  # noqa: F401
from .AttEnsemble import AttEnsemble  # noqa: F401

_OUT_OF_SCOPE = ('fc', 'show_tell', 'language_model', 'att2in', 'att2all2', 'stackatt', 'denseatt', 'bert', 'm2transformer')


# use_bn (BatchNorm around att_embed, AttModel.py:80-85) runs for updown / topdown and att2in2; why the others refuse it
_USE_BN_REFUSED = {
    'newfc': 'the reference deletes att_embed there (NewFCModel), so the switch would do nothing',
    'transformer': 'its prefill goes through its own Lin objects, not the shared prefill that has the BatchNorm path',
    'aoa': 'its prefill goes through its own Lin objects, not the shared prefill that has the BatchNorm path',
    'adaatt': 'the AdaAtt prefill has no BatchNorm path',
    'adaattmo': 'the AdaAtt prefill has no BatchNorm path',
}


def setup(opt):
    name = opt.caption_model
    if getattr(opt, 'use_bn', 0) and name in _USE_BN_REFUSED:
        raise NotImplementedError('use_bn is not supported for caption_model %r: %s' % (name, _USE_BN_REFUSED[name]))
    if name in ('topdown', 'updown'):
        return UpDownModel(opt)
    if name == 'newfc':
        from .NewFCModel import NewFCModel
        return NewFCModel(opt)
    if name == 'transformer':
        from .TransformerModel import TransformerModel
        return TransformerModel(opt)
    if name == 'att2in2':
        from .Att2in2Model import Att2in2Model
        return Att2in2Model(opt)
    if name in ('adaatt', 'adaattmo'):
        from .AdaAttModel import AdaAttModel, AdaAttMOModel
        return (AdaAttMOModel if name == 'adaattmo' else AdaAttModel)(opt)
    if name == 'aoa':
        from .AoAModel import AoAModel
        return AoAModel(opt)
    if name in _OUT_OF_SCOPE:
        raise NotImplementedError('caption_model %r is outside the accelerated hot path (SURVEY.md 2.1); use the '
                                  'reference implementation for it' % name)
    raise Exception('Caption model not supported: {}'.format(name))
