"""Multi-process semantics of the data-parallel path on CPU (gloo, world_size 2): ONE all-reduce over the
flat fp32 gradient buffer, averaging across ranks, value-clipping AFTER averaging (SURVEY.md 8e;
train.py:194-195 clips the already-reduced gradient).  RCCL itself is exercised by bench.py --gpus N."""
import os
import socket

import torch
import torch.distributed as dist
import torch.multiprocessing as mp


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q):
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    from imagecaptioning.pytorch_amd.flat import FlatParams
    torch.manual_seed(0)                        # identical initial weights on every rank (as bench.py does)
    net = torch.nn.Sequential(torch.nn.Linear(7, 5), torch.nn.Linear(5, 3))
    flat = FlatParams(net)
    assert flat.total % 4 == 0
    g = torch.Generator().manual_seed(100 + rank)   # rank-specific "batch"
    for p in net.parameters():
        p.grad = torch.randn(p.shape, generator=g) * (rank + 1)
    local = [p.grad.clone() for p in net.parameters()]
    flat.collect_grads()
    # every parameter's .grad now IS a view of the flat buffer
    for n, p in zip(flat.names, flat.params):
        assert p.grad.data_ptr() == flat.grad_views[n].data_ptr()
    calls = {'n': 0}
    orig = dist.all_reduce

    def counting(*a, **k):
        calls['n'] += 1
        return orig(*a, **k)

    dist.all_reduce = counting
    scale = flat.all_reduce()
    dist.all_reduce = orig
    assert calls['n'] == 1, 'exactly one collective per step'
    assert abs(scale - 1.0 / world) < 1e-12
    avg = [p.grad * scale for p in net.parameters()]
    # (numpy copies: a torch tensor in a Queue is shared by file descriptor, which the parent can no longer fetch once this
    #  process has exited)
    q.put((rank, [t.numpy().copy() for t in local], [t.numpy().copy() for t in avg]))
    dist.barrier()
    dist.destroy_process_group()


def _worker_buckets(rank, world, port, q):
    """bucketed variant: buckets announced out of buffer order (as the BPTT finishes them), leftovers reduced at the
    end; the result must equal the single flat all-reduce and no element may be reduced twice."""
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    from imagecaptioning.pytorch_amd.flat import FlatParams
    torch.manual_seed(0)
    net = torch.nn.Sequential(torch.nn.Linear(7, 5), torch.nn.Linear(5, 3), torch.nn.Linear(3, 2))
    flat = FlatParams(net)
    flat.begin_overlap()
    g = torch.Generator().manual_seed(100 + rank)
    for n, p in zip(flat.names, flat.params):          # a native backward writes straight into the flat views
        flat.grad_views[n].copy_(torch.randn(p.shape, generator=g) * (rank + 1))
    local = flat.grad.clone()
    flat.end_backward()
    flat.on_grads_ready(['2.weight', '2.bias'])        # last layer first (adjacent -> one collective)
    flat.on_grads_ready(['0.bias', '1.bias'])          # two non-adjacent parameters -> two collectives
    flat.collect_grads()
    scale = flat.finish_overlap()                      # leftovers: 0.weight, 1.weight
    q.put((rank, local.numpy().copy(), (flat.grad * scale).numpy().copy(), flat.last_collectives))
    dist.barrier()
    dist.destroy_process_group()


def test_bucketed_overlapped_allreduce_equals_flat_allreduce():
    world = 2
    port = _free_port()
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker_buckets, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = {}
    for _ in range(world):
        rank, local, avg, n_coll = q.get(timeout=120)
        got[rank] = (torch.from_numpy(local), torch.from_numpy(avg), n_coll)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    want = (got[0][0] + got[1][0]) / 2
    for r in range(world):
        assert torch.allclose(got[r][1], want, atol=1e-6)
        assert got[r][2] == 5            # 1 + 2 announced buckets, 2 leftover gaps


def test_single_flat_allreduce_averages_gradients():
    world = 2
    port = _free_port()
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = {}
    for _ in range(world):
        rank, local, avg = q.get(timeout=120)
        got[rank] = ([torch.from_numpy(t) for t in local], [torch.from_numpy(t) for t in avg])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for i in range(len(got[0][0])):
        want = (got[0][0][i] + got[1][0][i]) / 2
        for r in range(world):
            assert torch.allclose(got[r][1][i], want, atol=1e-6)
        # clip-after-average (ours, and Lightning/DataParallel) differs from clip-before-average in general
        clipped_after = want.clamp(-0.1, 0.1)
        clipped_before = (got[0][0][i].clamp(-0.1, 0.1) + got[1][0][i].clamp(-0.1, 0.1)) / 2
        assert clipped_after.shape == clipped_before.shape


def _cpu_adam(p, g, m, v, lr, b1, b2, eps, wd, clip, scale, step):
    """reference arithmetic of capmi_adam_step (clip after scaling, bias-corrected Adam) for the CPU-only test"""
    g = g * scale
    if clip > 0:
        g = g.clamp(-clip, clip)
    if wd:
        g = g + wd * p
    m.mul_(b1).add_(g, alpha=1 - b1)
    v.mul_(b2).addcmul_(g, g, value=1 - b2)
    p.addcdiv_(m / (1 - b1 ** step), (v / (1 - b2 ** step)).sqrt() + eps, value=-lr)


def _worker_sharded(rank, world, port, q):
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    from imagecaptioning.pytorch_amd.flat import FlatParams
    out = []
    for mode in ('allreduce', 'sharded'):
        torch.manual_seed(0)
        net = torch.nn.Sequential(torch.nn.Linear(7, 5), torch.nn.Linear(5, 3), torch.nn.Linear(3, 2))
        flat = FlatParams(net)
        assert flat.total % 64 == 0 and flat.total >= flat.used
        for step in range(3):
            g = torch.Generator().manual_seed(100 * step + rank)
            for n, p in zip(flat.names, flat.params):
                flat.grad_views[n].copy_(torch.randn(p.shape, generator=g) * (rank + 1))
            flat.end_backward()
            if mode == 'allreduce':
                scale = flat.all_reduce()
                flat.step_count += 1
                _cpu_adam(flat.flat, flat.grad, flat.exp_avg, flat.exp_avg_sq, 1e-2, 0.9, 0.999, 1e-8, 0.0, 0.1, scale, flat.step_count)
            else:
                flat.sharded_step(1e-2, clip_value=0.1, adam=_cpu_adam)
        out.append(flat.flat.clone())
        assert all(torch.equal(p.data, flat.flat[o:o + p.numel()].view_as(p)) for p, o in zip(flat.params, flat.offsets))
    q.put((rank, out[0].numpy().copy(), out[1].numpy().copy()))
    dist.barrier()
    dist.destroy_process_group()


def test_sharded_step_reduce_scatter_adam_all_gather_equals_all_reduce():
    """reduce-scatter -> clip+Adam on the own shard -> all-gather of the parameters == all-reduce + full Adam, and every rank
    ends with the same, complete parameters"""
    world = 2
    port = _free_port()
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker_sharded, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = {}
    for _ in range(world):
        rank, a, b = q.get(timeout=120)
        got[rank] = (torch.from_numpy(a), torch.from_numpy(b))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert torch.equal(got[0][1], got[1][1])                     # replicas identical after the all-gather
    assert torch.allclose(got[0][0], got[0][1], atol=1e-7)       # same update as the all-reduce route


def _worker_partition(rank, world, port, q):
    """two ranks of tools/train.py's loaders over ONE dataset: what each rank sees in a pass"""
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    import argparse
    from conftest import GOLDEN
    from imagecaptioning.pytorch_amd.captioning.data.feature_loader import FeatureLoader
    from imagecaptioning.pytorch_amd.captioning.data.synthetic_loader import SyntheticLoader
    ds = os.path.join(GOLDEN, 'loader_ds')
    opt = argparse.Namespace(batch_size=2, seq_per_img=2, input_json=os.path.join(ds, 'dataset.json'),
                             input_label_h5=os.path.join(ds, 'labels.npz'), input_att_dir=os.path.join(ds, 'att'),
                             input_fc_dir=os.path.join(ds, 'fc'), use_fc=True, norm_att_feat=0, train_only=0, seed=123)
    ld = FeatureLoader(opt, workers=1, rank=rank, world=world)
    n_train = len(ld.full_order['train'])
    per_rank = len(ld.order['train'])
    passes = []
    for _ in range(3):                                      # three passes: the reshuffles must stay in step across the ranks
        seen = []
        while len(seen) < per_rank:
            d = ld.get_batch('train')
            seen += [i['ix'] for i in d['infos']]
        passes.append(seen[:per_rank])
        # (a batch may straddle two passes: put what belongs to the next pass back by rewinding to the pass boundary)
        ld.reset_iterator('train') if len(seen) > per_rank else None
    syn = SyntheticLoader(argparse.Namespace(batch_size=3, seq_per_img=5, seq_length=8, vocab_size=50, seed=5, synthetic_images=12,
                                             fc_feat_size=8, att_feat_size=8, synthetic_regions=4), rank=rank, world=world)
    syn_seen = [i['ix'] for _ in range(2) for i in syn.get_batch('train')['infos']]
    everything = [None] * world
    dist.all_gather_object(everything, {'passes': passes, 'n_train': n_train, 'per_rank': per_rank, 'val': list(ld.order['val']),
                                        'val_all': list(ld.full_order['val']), 'syn': syn_seen,
                                        'df': sorted(syn.document_frequency()[0].items())[:20]})
    if rank == 0:
        q.put(everything)
    dist.barrier()
    dist.destroy_process_group()


def test_ranks_partition_one_shuffled_pass():
    """VERDICT r3 missing #4 (tools/train_pl.py:60-73 + Lightning's DistributedSampler): the ranks share ONE permutation per epoch
    and take every world-th element -- disjoint, covering the split once (the tail padded from the head to equal counts) -- instead
    of independent shuffles that overlap within an epoch."""
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    world, port = 2, _free_port()
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker_partition, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = q.get(timeout=120)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    n_train, per_rank = got[0]['n_train'], got[0]['per_rank']
    assert per_rank == (n_train + world - 1) // world == got[1]['per_rank']
    orders = set()
    for k in range(3):
        a, b = got[0]['passes'][k], got[1]['passes'][k]
        both = a + b
        assert len(set(both)) == n_train, 'the ranks of a pass cover the whole train split'
        assert len(both) - len(set(both)) == (-n_train) % world, 'only the padding repeats an image'
        assert len(set(a)) == len(a) and len(set(b)) == len(b)
        orders.add(tuple(a))
    assert len(orders) > 1, 'the pass is reshuffled between epochs'
    assert sorted(got[0]['val'] + got[1]['val']) == sorted(got[0]['val_all']) and not set(got[0]['val']) & set(got[1]['val'])
    assert not set(got[0]['syn']) & set(got[1]['syn']), 'synthetic images are dealt out disjointly'
    assert got[0]['df'] == got[1]['df'], 'one corpus, one document-frequency table on every rank'
