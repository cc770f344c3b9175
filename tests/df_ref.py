"""Checker of the device document-frequency build (csrc/df_build.hip, tools/prepro_ngrams.py): a dict-based restatement of
scripts/prepro_ngrams.py:17-22 + CiderScorer.compute_doc_freq.  Per image, the set of n-grams (n = 1..4) over its captions; every
member adds 1.  ref_len is the number of images, one without captions included (cook_append adds an entry for each).

A corpus is a list (per image) of lists (per caption) of id lists; a caption is exactly its ids (the caller appended the <eos>).
tests/test_df_build_host.py pins this on oracle/ciderd.py::build_document_frequency and on ciderd.build_table / load_df_image.
"""
import numpy as np


def doc_freq(images):
    """-> ({n-gram tuple -> number of images that hold it, as float}, ref_len)"""
    df = {}
    for caps in images:
        seen = set()
        for cap in caps:
            cap = [int(t) for t in cap]
            for n in range(1, 5):
                for i in range(len(cap) - n + 1):
                    seen.add(tuple(cap[i:i + n]))
        for g in seen:
            df[g] = df.get(g, 0.0) + 1.0
    return df, len(images)


def ragged(images, tok_dtype=np.int64):
    """-> tok [total], cap_off int64 [n_caps + 1], img_off int64 [n_img + 1]"""
    caps = [c for img in images for c in img]
    cap_off = np.concatenate([[0], np.cumsum([len(c) for c in caps])]).astype(np.int64)
    img_off = np.concatenate([[0], np.cumsum([len(img) for img in images])]).astype(np.int64)
    tok = np.array([t for c in caps for t in c], dtype=tok_dtype)
    return tok, cap_off, img_off


def pairs(keys, vals):
    """the (key, value) set of a table image; slot positions are not part of it"""
    keys, vals = np.asarray(keys), np.asarray(vals)
    occ = keys != 0
    assert not vals[~occ].any(), 'an empty slot carries a value'
    out = set(zip(keys[occ].tolist(), vals[occ].tolist()))
    assert len(out) == int(occ.sum()), 'a key sits in two slots'
    return out


def random_images(rng, n_img, n_caps, max_len, vocab, min_len=1):
    """n_img images x n_caps captions of min_len..max_len ids in 1..vocab, each ended by 0"""
    return [[rng.integers(1, vocab + 1, size=int(rng.integers(min_len, max_len + 1))).tolist() + [0] for _ in range(n_caps)]
            for _ in range(n_img)]
