#!/usr/bin/env python3
"""Generate ``tests/golden/diveval_ref.npz``: the REAL reference's captioning/utils/div_utils.py (compute_div_n for n = 1, 2 and
compute_global_div_n for n = 1, the three numbers eval_multi.eval_div_stats reports) on token-id captions joined as strings.  Run
only where the reference checkout exists (never on the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_diveval.py

    groups [6, 5, 8] int64   6 images, 5 captions each, L = 8, vocabulary 12 (0 = end and pad); image 1 holds an empty caption,
                             image 2 five identical captions, image 3 a full-length row without a 0
    div1, div2 []            compute_div_n(caps, 1 | 2)[0]
    div1_img, div2_img [6]   compute_div_n(caps, 1 | 2)[1]
    gdiv1 []                 compute_global_div_n(caps, 1)[0]
"""
import importlib.util
import os

import numpy as np

REF = os.environ.get('CAPMI_REFERENCE', '/root/reference')
HERE = os.path.dirname(os.path.abspath(__file__))


def inputs():
    rng = np.random.default_rng(20241017)
    n_img, n, L, vocab = 6, 5, 8, 12
    groups = np.zeros((n_img, n, L), dtype=np.int64)
    for i in range(n_img):
        for s in range(n):
            ln = int(rng.integers(1, L + 1))
            groups[i, s, :ln] = rng.integers(1, vocab, size=ln)
    groups[1, 3] = 0                                                       # an empty caption
    groups[2, :] = groups[2, 0]                                            # identical captions
    groups[3, 0] = rng.integers(1, vocab, size=L)                          # no terminating 0
    return groups


def caption_string(row):
    words = []
    for t in row:
        if t == 0:
            break
        words.append(str(int(t)))
    return ' '.join(words)


def main():
    spec = importlib.util.spec_from_file_location('div_utils', os.path.join(REF, 'captioning', 'utils', 'div_utils.py'))
    div_utils = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(div_utils)
    groups = inputs()
    caps = {i: [caption_string(row) for row in g] for i, g in enumerate(groups)}
    div1, div1_img = div_utils.compute_div_n(caps, 1)
    div2, div2_img = div_utils.compute_div_n(caps, 2)
    gdiv1, _ = div_utils.compute_global_div_n(caps, 1)
    np.savez(os.path.join(HERE, 'diveval_ref.npz'), groups=groups, div1=np.float64(div1), div2=np.float64(div2),
             div1_img=np.asarray(div1_img, dtype=np.float64), div2_img=np.asarray(div2_img, dtype=np.float64), gdiv1=np.float64(gdiv1))


if __name__ == '__main__':
    main()
