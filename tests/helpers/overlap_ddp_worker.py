"""Worker of tests/test_overlap_loss_ddp_gpu.py: launched twice by torch.distributed.run (gloo rendezvous, BOTH ranks on cuda:0).
Each rank holds half of a batch of 4 and runs TverskyLoss(group=WORLD) forward and backward on it.  The first half carries no
foreground pixel, so a T_c formed per rank would differ from the global batch's.  Asserted: the loss on both ranks equals the
float64 restatement's on the whole batch, and the two ranks' gradients, concatenated, equal its gradient -- both within 4 x the
floor of these inputs (tests/overlap_loss_ref.py's rule: the same formula in fp32 torch ops against float64, at least 2^-24) --
and equal what one process computes on the whole batch to the same bound."""
import os
import sys

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main():
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    from iswm_amd.utils.loss import TverskyLoss
    from tests import overlap_loss_ref as R

    g = R.gen(21)
    logits = torch.randn(4, 2, 65, 65, generator=g)
    labels = (torch.rand(4, 65, 65, generator=g) < 0.2).to(torch.uint8)
    labels[torch.rand(4, 65, 65, generator=g) < 0.1] = R.IGNORE
    labels[:2][labels[:2] == 1] = 0                                  # ranks' halves: [0:2] without foreground, [2:4] with
    weight = torch.tensor([1.0, 3.0])
    kw = dict(alpha=0.3, beta=0.7, gamma=0.75, smooth=1.0, classes="foreground", ce_weight=1.0, overlap_weight=2.0)
    ref = R.overlap_ref(logits, labels, weight, R.IGNORE, 1.0, 2.0, 0.3, 0.7, 0.75, 1.0, "foreground")
    per_rank = R.overlap_ref(logits[:2], labels[:2], weight, R.IGNORE, 1.0, 2.0, 0.3, 0.7, 0.75, 1.0, "foreground")
    assert abs(float(per_rank["loss"]) - float(ref["loss"])) > 1e-2   # a per-rank loss would be a different number

    sl = slice(2 * rank, 2 * rank + 2)
    z = logits[sl].to(dev).requires_grad_(True)
    loss = TverskyLoss(weight=weight, group=dist.group.WORLD, **kw).to(dev)(z, labels[sl].to(dev))
    loss.backward()
    torch.cuda.synchronize()
    losses = [torch.zeros(1) for _ in range(world)]
    dist.all_gather(losses, loss.detach().cpu().reshape(1))
    grads = [torch.zeros(2, 2, 65, 65) for _ in range(world)]
    dist.all_gather(grads, z.grad.cpu())
    grad = torch.cat(grads)

    ok = True
    if rank == 0:
        z1 = logits.to(dev).requires_grad_(True)
        single = TverskyLoss(weight=weight, **kw).to(dev)(z1, labels.to(dev))
        single.backward()
        low = R.overlap_ref(logits, labels, weight, R.IGNORE, 1.0, 2.0, 0.3, 0.7, 0.75, 1.0, "foreground", dtype=torch.float32)
        bl = 4 * max(R.rel_err(low["loss"], ref["loss"]), R.FLOOR_MIN)          # the floor rule, measured on these inputs
        bg = 4 * max(R.rel_err(low["grad"], ref["grad"]), R.FLOOR_MIN)
        e_loss = [R.rel_err(l, ref["loss"]) for l in losses]
        e_grad = R.rel_err(grad, ref["grad"])
        e_single = (R.rel_err(losses[0], single.detach().cpu()), R.rel_err(grad, z1.grad.cpu()))
        print("OVERLAP_DDP loss rank0 %.8f rank1 %.8f single %.8f float64 %.8f | rel err loss %.2e %.2e (bound %.1e) grad %.2e "
              "(bound %.1e) | vs single process: loss %.2e grad %.2e" %
              (float(losses[0]), float(losses[1]), float(single), float(ref["loss"]), e_loss[0], e_loss[1], bl, e_grad, bg,
               e_single[0], e_single[1]), flush=True)
        ok = float(losses[0]) == float(losses[1]) and max(e_loss) <= bl and e_grad <= bg and e_single[0] <= bl and e_single[1] <= bg
    flag = torch.tensor([1.0 if ok else 0.0])
    dist.all_reduce(flag, op=dist.ReduceOp.MIN)
    dist.barrier()
    dist.destroy_process_group()
    sys.exit(0 if float(flag) == 1.0 else 1)


if __name__ == "__main__":
    main()
