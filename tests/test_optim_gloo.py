"""flat.sharded_step under a one-state rule on CPU (gloo, world_size 2), after test_ddp_gloo.py's Adam case: reduce-scatter ->
clip + RMSprop on the rank's shard of the parameters and of the SINGLE state buffer -> all-gather == all-reduce + the full update."""
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


def _cpu_rule(rule, p, g, s1, s2, lr, alpha, beta, eps, wd, clip, scale, step):
    """stands in for ops.optim_step (no HIP device here): the float64 replay's arithmetic on the fp32 views it is handed"""
    import optim_ref64 as R
    assert s2 is None                              # the one-state rules never see a second buffer
    pd, st = p.double(), {R.STATE_KEYS[rule][0]: s1.double()}
    R.step(rule, pd, g, st, lr, step, alpha=alpha, beta=beta, eps=eps, weight_decay=wd, clip=clip, grad_scale=scale)
    p.copy_(pd)
    s1.copy_(st[R.STATE_KEYS[rule][0]])


def _worker(rank, world, port, q):
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    from imagecaptioning.pytorch_amd.flat import FlatParams
    out = []
    for mode in ('allreduce', 'sharded'):
        torch.manual_seed(0)
        net = torch.nn.Sequential(torch.nn.Linear(7, 5), torch.nn.Linear(5, 3), torch.nn.Linear(3, 2))
        flat = FlatParams(net, 'rmsprop')
        assert not hasattr(flat, 'exp_avg_sq')
        for step in range(3):
            g = torch.Generator().manual_seed(100 * step + rank)
            for n, p in zip(flat.names, flat.params):
                flat.grad_views[n].copy_(torch.randn(p.shape, generator=g) * (rank + 1))
            flat.end_backward()
            if mode == 'allreduce':
                scale = flat.all_reduce()
                flat.step_count += 1
                _cpu_rule('rmsprop', flat.flat, flat.grad, flat.square_avg, None, 1e-2, 0.9, 0.999, 1e-8, 0.01, 0.1, scale, flat.step_count)
            else:
                flat.sharded_step(1e-2, weight_decay=0.01, clip_value=0.1, adam=_cpu_rule)
        out.append((flat.flat.clone(), flat.square_avg.clone()))
    q.put((rank, [t.numpy().copy() for pair in out for t in pair]))
    dist.barrier()
    dist.destroy_process_group()


def test_sharded_rmsprop_step_equals_all_reduce_and_updates_only_the_own_state_shard():
    world = 2
    port = _free_port()
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = {}
    for _ in range(world):
        rank, arrs = q.get(timeout=120)
        got[rank] = [torch.from_numpy(a) for a in arrs]          # p(all-reduce), sq(all-reduce), p(sharded), sq(sharded)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert torch.equal(got[0][2], got[1][2])                     # replicas identical after the all-gather
    assert torch.allclose(got[0][0], got[0][2], atol=1e-7)       # same update as the all-reduce route
    half = got[0][1].numel() // 2
    for r in range(world):
        full, own = got[r][1], got[r][3]
        lo, hi = r * half, (r + 1) * half
        assert torch.allclose(own[lo:hi], full[lo:hi], atol=1e-7) and float(own[lo:hi].abs().max()) > 0
        other = torch.cat([own[:lo], own[hi:]])
        assert float(other.abs().max()) == 0.0                   # the other rank's slice of the state buffer was never touched
