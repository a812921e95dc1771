"""Worker of tests/test_gpu_flat_optim.py: one of two ranks that share ONE MI355X (gloo backend, as tests/dp_gpu_worker.py).  Every
rank back-propagates its own gradients into the reducer's buckets; the bucket all-reduces leave SUMS (finish(mean=False)) and the flat
optimizer's update kernel applies 1 / world.  The result must equal torch's optimizer of the same name on the mean of the per-rank
gradients at the parity bar of tests/test_gpu_flat_optim.py — for the plain step and for the zeroing one issued during backward."""
import os
import sys

import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from svol_amd import parallel  # noqa: E402

SHAPES = [(64, 33), (33,), (7,), (128, 128), (5, 3, 2), (1,)]
DEAD = 2


def grads(step, rank):
    g = torch.Generator(device='cuda').manual_seed(1000 + 10 * step + rank)
    return [torch.randn(s, device='cuda', generator=g) * (1.0 + step) for s in SHAPES]


def main():
    rank, world = int(os.environ['RANK']), int(os.environ['WORLD_SIZE'])
    torch.cuda.set_device(0)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    torch.manual_seed(0)
    p0 = [torch.randn(s, device='cuda') for s in SHAPES]
    worst = {}
    for name, Flat, Torch, kw in (('sgd', parallel.FlatSGD, torch.optim.SGD, dict(lr=3e-3, momentum=0.9, weight_decay=0.05)),
                                  ('adam', parallel.FlatAdam, torch.optim.Adam, dict(lr=3e-3, weight_decay=0.05))):
        pb = [torch.nn.Parameter(p.clone()) for p in p0]
        ob = Torch([p for i, p in enumerate(pb) if i != DEAD], **kw)
        for step in range(4):
            per_rank = [grads(step, r) for r in range(world)]
            for i, p in enumerate(pb):
                if i != DEAD:
                    p.grad = sum(per_rank[r][i] for r in range(world)) / world
            ob.step()
        for early in (False, True):
            pa = [torch.nn.Parameter(p.clone()) for p in p0]
            red = parallel.BucketedGradAllReduce(pa, bucket_bytes=40000, skip=[pa[DEAD]])
            assert red.world == 2 and len(red.buckets) >= 2
            oa = Flat(red, params=pa, zero_grads=early, step_in_backward=early, **kw)
            for step in range(4):
                oa.zero_grad()
                mine = grads(step, rank)
                sum((p * g).sum() for i, (p, g) in enumerate(zip(pa, mine)) if i != DEAD).backward()   # dloss/dp = this rank's g
                red.finish(mean=False)
                assert red.pending_scale == 0.5
                oa.step()
                assert red.pending_scale == 1.0
            torch.cuda.synchronize()
            if early:
                assert all(bool((b['flat'] == 0).all()) for b in red.buckets)
            for i, (a, b) in enumerate(zip(pa, pb)):
                err, ref = float((a.detach() - b.detach()).abs().max()), max(1.0, float(b.detach().abs().max()))
                assert err <= 2e-6 * ref, (name, early, i, err)
                worst[name] = max(worst.get(name, 0.0), err / ref)
            assert torch.equal(pa[DEAD].detach(), p0[DEAD])
            red.remove()
    print(f'rank {rank}: flat optimizers == torch on the averaged gradients (worst rel diff {worst})', flush=True)
    dist.destroy_process_group()


if __name__ == '__main__':
    main()
