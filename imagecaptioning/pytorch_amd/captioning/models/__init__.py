"""Model factory (reference captioning/models/__init__.py:20-73), hot-path models only."""
from .AttModel import AttModel, UpDownModel  # noqa: F401
from .AttEnsemble import AttEnsemble  # noqa: F401

_OUT_OF_SCOPE = ('fc', 'show_tell', 'language_model', 'att2in', 'att2all2', 'stackatt', 'denseatt', 'bert', 'm2transformer')


def setup(opt):
    name = opt.caption_model
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
