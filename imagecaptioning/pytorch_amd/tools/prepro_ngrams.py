#!/usr/bin/env python3
"""The CIDEr-D document-frequency table of a dataset's captions, counted on the GPU: the reference's scripts/prepro_ngrams.py
without its scorer package.

    python -m imagecaptioning.pytorch_amd.tools.prepro_ngrams --input_json data/dataset_coco.json --dict_json data/cocotalk.json \\
        --output_pkl data/coco-train --split train                      # -> data/coco-train-idxs.capmi.npz

The command line is the reference's.  The host half reads the captions as scripts/prepro_ngrams.py:25-54 does: the images of
--split (train also takes restval, all takes every image), every token that the vocabulary lacks replaced by UNK, <eos> (id 0)
appended to every caption, words mapped to ids.  The device half (capmi_df_count / capmi_df_finalize) counts, for n = 1..4, the
images that hold each n-gram and writes the flat hash image that `--cached_tokens <output_pkl>-idxs` (rewards.init_scorer) loads;
ref_len is the number of images of the split.

Deliberately not produced:
  * <output_pkl>-words.p, the table over words: this backend scores token ids only;
  * anything for a dict_json with a `bpe` entry: the captions would have to be segmented with subword_nmt first, which is not
    available here; the tool stops with a message.
No pickle is written either: <output_pkl>-idxs.capmi.npz is what tools/convert_df.py makes of the reference's -idxs.p.

A second mode serves users who hold only the training files:

    ... prepro_ngrams --from_labels --input_json data/cocotalk.json --input_label_h5 data/cocotalk_label.h5 --output_pkl data/coco-train

The captions are the label rows of the split's images (feature_loader.load_labels): a row's ids up to its first 0, plus the <eos>
when the row has room for one.  Deviation from the reference: the label file cuts a caption at its width W (prepro_labels'
max_length), so the n-grams that reach beyond W words and the <eos> n-grams of a cut caption are missing, and a caption of exactly
W words cannot be told from a cut one (it gets no <eos> either).  This is the table tools/train.py builds on the host when
--cached_tokens names no file.
"""
import argparse
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(HERE))))


def in_split(img_split, split):
    """prepro_ngrams.py:33-35"""
    return split == 'all' or img_split == split or (split == 'train' and img_split == 'restval')


def ragged(images):
    """list (per image) of lists (per caption) of id lists -> tok int64 [total], cap_off int64 [n_caps + 1], img_off int64 [n_img + 1]"""
    caps = [c for img in images for c in img]
    cap_off = np.zeros(len(caps) + 1, dtype=np.int64)
    np.cumsum([len(c) for c in caps], out=cap_off[1:])
    img_off = np.zeros(len(images) + 1, dtype=np.int64)
    np.cumsum([len(img) for img in images], out=img_off[1:])
    tok = np.fromiter((t for c in caps for t in c), dtype=np.int64, count=int(cap_off[-1]))
    return tok, cap_off, img_off


def corpus_from_json(imgs, ix_to_word, split):
    """the id captions of the split's images, <eos> appended (prepro_ngrams.py:25-48)"""
    wtoi = {w: int(i) for i, w in ix_to_word.items()}
    wtoi['<eos>'] = 0
    images = []
    for img in imgs:
        if not in_split(img.get('split'), split):
            continue
        caps = []
        for sent in img['sentences']:
            words = list(sent['tokens']) + ['<eos>']
            if 'UNK' not in wtoi and any(w not in wtoi for w in words):
                raise SystemExit('a caption of image %s holds a word the vocabulary lacks, and the vocabulary has no UNK'
                                 % img.get('cocoid', img.get('id', img.get('filename'))))
            caps.append([wtoi[w] if w in wtoi else wtoi['UNK'] for w in words])
        images.append(caps)
    return ragged(images)


def caption_of_label_row(row):
    """a label row (0 = end and pad) as the caption it stands for: its ids, and the <eos> when the row was not cut"""
    row = [int(t) for t in row]
    return row[:row.index(0) + 1] if 0 in row else row


def corpus_from_labels(info, lab, split):
    """the captions of the split's images out of the label arrays (an image without a split belongs to every split, as in the loader)"""
    images = []
    for ix, img in enumerate(info['images']):
        sp = img.get('split')
        if sp is not None and not in_split(sp, split):
            continue
        rows = lab['labels'][int(lab['label_start_ix'][ix]) - 1: int(lab['label_end_ix'][ix])]
        images.append([caption_of_label_row(r) for r in rows])
    return ragged(images)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--input_json', default='data/dataset_coco.json',
                    help='the dataset json with the tokenised captions (with --from_labels: the json of prepro_labels, e.g. cocotalk.json)')
    ap.add_argument('--dict_json', default='data/cocotalk.json', help='the json that holds ix_to_word')
    ap.add_argument('--output_pkl', default='data/coco-all', help='stem of the output: <output_pkl>-idxs.capmi.npz is written')
    ap.add_argument('--split', default=None, help='test, val, train (with restval) or all; default all, train with --from_labels')
    ap.add_argument('--from_labels', action='store_true', help='take the captions from --input_label_h5 (cut at the label width, see above)')
    ap.add_argument('--input_label_h5', default=None, help='the label file (.h5 or the .npz of tools/convert_labels.py) of --from_labels')
    args = ap.parse_args(argv)

    if args.from_labels:
        if not args.input_label_h5:
            raise SystemExit('--from_labels needs --input_label_h5')
        from imagecaptioning.pytorch_amd.captioning.data.feature_loader import load_labels
        info = json.load(open(args.input_json))
        if 'bpe' in info:
            raise SystemExit('%s has a bpe entry: its label ids are subword units, which this tool does not count' % args.input_json)
        corpus = corpus_from_labels(info, load_labels(args.input_label_h5), args.split or 'train')
    else:
        dict_json = json.load(open(args.dict_json))
        if 'bpe' in dict_json:
            raise SystemExit('%s has a bpe entry: the captions would have to be segmented with subword_nmt, which is not available '
                             'here. No table is written.' % args.dict_json)
        corpus = corpus_from_json(json.load(open(args.input_json))['images'], dict_json['ix_to_word'], args.split or 'all')
    tok, cap_off, img_off = corpus
    print('total imgs:', len(img_off) - 1)
    if len(img_off) < 2:
        raise SystemExit('no image in the split')

    from imagecaptioning.pytorch_amd.ciderd import build_df_image, save_table_image
    keys, vals, ref_len = build_df_image(tok, cap_off, img_off)
    print('count_refs:', int(ref_len))
    out = save_table_image(keys, vals, ref_len, args.output_pkl + '-idxs.capmi.npz')
    print(out)
    return out


if __name__ == '__main__':
    main()
