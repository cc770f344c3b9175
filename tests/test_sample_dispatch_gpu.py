"""CaptionModel._sample, the one sample dispatch of the six single-model families, against tests/golden/sample_dispatch.json: what
the five per-family ladders it replaced did for the same calls, recorded from the parent commit by
tests/golden/make_sample_dispatch.py (cases, shapes and what is recorded: its docstring).  Every case is run again here with the
generator's own run_case and compared for EQUALITY: the refusal's class and message, or the tokens, the sha256 of seq and of the
log-probabilities and the number of seeds drawn; and the ordered leaves that ran -- UpDown's native beam search and the
stepper-driven one return the same tokens, so equal outputs alone would not show that a call still takes its arm.

One refusal differs on purpose: the device check now has RecurrentModel's wording everywhere ('... (got a cpu tensor) ...'); both
wordings contain 'HIP device only', and that is what the 'cpu' case compares for the families that had the short one."""
import importlib.util
import json
import os

import pytest
import torch

from conftest import GOLDEN

_spec = importlib.util.spec_from_file_location('make_sample_dispatch', os.path.join(GOLDEN, 'make_sample_dispatch.py'))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)

with open(os.path.join(GOLDEN, 'sample_dispatch.json')) as f:
    WANT = json.load(f)


def test_fixture_covers_every_case_and_keeps_its_digests():
    assert sorted(WANT) == sorted('%s/%s' % (fam, case[0]) for fam in G.FAMILIES for case in G.CASES)
    loose = [k for k, rec in WANT.items() if rec.get('stable') is False]
    assert 10 * len(loose) <= len(WANT), loose        # a case whose two parent runs differed keeps tokens and leaves only


@pytest.mark.gpu
@pytest.mark.parametrize('family', G.FAMILIES)
def test_sample_dispatch_matches_the_parent(family):
    dev = torch.device('cuda')
    model, inputs = G.build(family, dev)
    bad = []
    for case in G.CASES:
        want = WANT['%s/%s' % (family, case[0])]
        got = G.run_case(model, inputs, case, dev)
        if want.get('stable') is False:
            got = {k: v for k, v in got.items() if k in ('tokens', 'error', 'message', 'leaves')}
            got['stable'] = False
        if case[0] == 'cpu' and 'HIP device only' in want.get('message', '') and 'HIP device only' in got.get('message', ''):
            got['message'] = want['message']
        if got != want:
            bad.append((case[0], {k: (want.get(k), got.get(k)) for k in set(want) | set(got) if want.get(k) != got.get(k)}))
    assert not bad, bad
