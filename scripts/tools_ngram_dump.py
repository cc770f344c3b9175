"""Runs every entry point of the n-gram family (csrc/ngram_metrics.h: CIDEr-D plain and cooked, LanguageEval, DiversityEval with
and without the oracle, bleu4, self_cider, nsc_advantage) once on fixed inputs and writes every output array to an .npz, so that
two builds of the library can be compared bit for bit:

    CAPMI_LIB=/path/to/other/libcapmi.so python scripts/tools_ngram_dump.py a.npz
    python scripts/tools_ngram_dump.py b.npz
    python scripts/tools_ngram_dump.py --compare a.npz b.npz        # np.array_equal on every array, exit 1 on a difference

Cases: vocab 12 and 9487 x L 5, 20, 64 x n 2, 5, 32; five images with 1..5 references in arrays narrower than the widest (so
pack_refs marks completely filled rows with -1); rows that are all 0, rows without a 0, a row whose first 0 is its last column,
token ids the table has never seen.  The cooked blobs are not dumped (their padding bytes are uninitialised LDS); the
document-frequency table of the evaluation is dumped as sorted (key, count) pairs (its slot order differs from run to run)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
B = 5


def inputs(vocab, L, n, rng):
    gts = []
    for i in range(B):
        g = np.zeros((1 + i, max(1, L - i % 3)), dtype=np.int64)
        for r in range(g.shape[0]):
            ln = g.shape[1] if r == 0 else int(rng.integers(1, g.shape[1] + 1))       # row 0: completely filled
            g[r, :ln] = rng.integers(1, vocab + 1, size=ln)
        gts.append(g)
    rows = np.zeros((B * n + B, L), dtype=np.int64)                # sampled rows, then one greedy row per image
    for r in range(rows.shape[0]):
        g = gts[r // n if r < B * n else r - B * n]
        src = g[int(rng.integers(0, len(g)))]
        rows[r, :min(L, len(src))] = src[:L]
        flip = rng.random(L) < 0.3
        rows[r][flip] = rng.integers(0, vocab + 1, size=int(flip.sum()))
    rows[0] = 0                                                    # all 0
    rows[1] = rng.integers(1, vocab + 1, size=L)                   # no 0
    rows[B * n - 1] = rng.integers(1, vocab + 1, size=L)
    rows[B * n - 1, L - 1] = 0                                     # the first 0 is the last column
    rows[B * n, :min(L, 3)] = [vocab + 7, vocab + 8, vocab + 9][:min(L, 3)]      # ids absent from the table
    rows[B * n + 1] = 0
    rows[B * n + 2] = rng.integers(1, vocab + 1, size=L)
    return gts, rows


def dump(path):
    from oracle import ciderd as OC
    from imagecaptioning.pytorch_amd import _lib
    from imagecaptioning.pytorch_amd.ciderd import DeviceCiderD, nsc_advantage
    from imagecaptioning.pytorch_amd.diveval import DiversityEval
    from imagecaptioning.pytorch_amd.langeval import LanguageEval
    from imagecaptioning.pytorch_amd._lib import lib, ptr, check, stream_ptr
    dev = torch.device('cuda:0')
    out = {}
    for vocab in (12, 9487):
        corpus = OC.synthetic_corpus(200, vocab, 5, 20, seed=vocab)
        df, ref_len = OC.build_document_frequency([[OC.tokens_of(r) for r in g] for g in corpus])
        sc = DeviceCiderD(df, ref_len, dev)
        for L in (5, 20, 64):
            for n in (2, 5, 32):
                gts, rows = inputs(vocab, L, n, np.random.default_rng(1000 * L + n))
                tag = 'v%d_L%d_n%d/' % (vocab, L, n)

                def put(name, t):
                    out[tag + name] = t.cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
                N = B * n
                hyp = torch.from_numpy(rows).to(dev)
                sampled = hyp[:N].contiguous()
                img = torch.cat([torch.arange(N, device=dev) // n, torch.arange(B, device=dev)]).to(torch.int32)
                packed = sc.pack_refs(gts)
                refs, n_refs = packed
                put('refs', refs)
                plain = sc.score(hyp, img, refs, n_refs)
                put('ciderd_plain', plain)
                put('ciderd_cooked', sc.score(hyp, img, refs, n_refs, packed.cooked))
                stats = torch.zeros(N + B, 10, dtype=torch.int32, device=dev)
                put('bleu4', sc.bleu4(hyp, img, packed, 1.0, 0.5, stats=stats))
                put('bleu4_stats', stats)
                put('bleu4_mixed', sc.bleu4(hyp, img, packed, 0.7, 0.3, base=plain.clone()))
                s, K, eig = sc.self_cider(sampled, n, parts=True)
                put('self_cider', s)
                put('self_cider_K', K)
                put('self_cider_eig', eig)
                norm = torch.zeros(N, 4, dtype=torch.float64, device=dev)
                dots = torch.zeros(N, n, 4, dtype=torch.float64, device=dev)
                s2 = torch.zeros(B, dtype=torch.float64, device=dev)
                check(lib.capmi_self_cider_reward(ptr(sampled), B, n, L, ptr(sc.keys), ptr(sc.vals), sc.cap, sc.log_ref_len, ptr(norm),
                                                  ptr(dots), ptr(s2), None, None, stream_ptr()), 'capmi_self_cider_reward')
                put('self_cider_norm', norm)
                put('self_cider_dots', dots)
                put('self_cider_again', s2)
                reward, adv = nsc_advantage(plain[:N].contiguous(), n, add=s, add_w=0.3)
                put('nsc_reward', reward)
                put('nsc_adv', adv)
                put('nsc_adv_plain', nsc_advantage(plain[:N].contiguous(), n)[1])

                ev = LanguageEval.from_gts(gts, dev)
                ev.add(list(range(B)), hyp[N:].contiguous())
                ev.compute()
                for k in ('_out', '_totals', 'cider', 'rouge', 'bleu_stats', 'lens', 'lcs', 'ref_norm'):
                    put('langeval_' + k.lstrip('_'), getattr(ev, k))
                keys, counts = ev.table_keys.cpu().numpy().view(np.uint64), ev.table_counts.cpu().numpy()
                order = np.argsort(keys[keys != 0])
                put('langeval_df_keys', keys[keys != 0][order])
                put('langeval_df_counts', counts[keys != 0][order])
                for oracle in (False, True):
                    dv = DiversityEval(ev, n, oracle=oracle)
                    dv.add(list(range(B)), sampled)
                    dv.compute()
                    for k in ('_out', '_totals', 'K', 'eig', 'self_cider', 'distinct', 'tokens', 'mbleu_stats', 'sent_bleu2', 'norm') + \
                            (('oracle_scores',) if oracle else ()):
                        put('diveval%d_' % oracle + k.lstrip('_'), getattr(dv, k))
    torch.cuda.synchronize()
    np.savez(path, **out)
    print('%s: %d arrays from %s' % (path, len(out), _lib.LIB_PATH))


def compare(a, b):
    za, zb = np.load(a), np.load(b)
    assert sorted(za.files) == sorted(zb.files), 'the two files hold different arrays'
    bad = [k for k in za.files if za[k].dtype != zb[k].dtype or not np.array_equal(za[k].view(np.uint8) if za[k].dtype.kind == 'f' else za[k],
                                                                                   zb[k].view(np.uint8) if zb[k].dtype.kind == 'f' else zb[k])]
    for k in bad:
        print('DIFFERS', k)
    print('%d arrays compared, %d differ' % (len(za.files), len(bad)))
    return 1 if bad else 0


if __name__ == '__main__':
    if sys.argv[1] == '--compare':
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    dump(sys.argv[1])
