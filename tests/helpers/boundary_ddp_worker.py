"""Worker of tests/test_boundary_ddp_gpu.py: launched twice by torch.distributed.run (gloo rendezvous, BOTH ranks on cuda:0).
Each rank holds half of the batch of 4 of tests/boundary_ref.py's ddp_inputs and runs BoundaryLoss(group=WORLD) forward and
backward on it; the distance map is built per rank from its own labels (distances never cross an image).  Rank 0's half is all
ignored, so an N or a sum of weights formed per rank would be 0 there and the global batch's on the other.  Asserted: the loss on
both ranks equals the float64 restatement's on the whole batch, and the two ranks' gradients, concatenated, equal its gradient --
both within 4 x the recorded floor of these inputs -- and equal what one process computes on the whole batch to the same bound; N
is the global batch's on both ranks, exactly."""
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
    from iswm_amd.utils.loss import BoundaryLoss
    from tests import boundary_ref as R

    logits, labels, weight, sd2 = R.ddp_inputs()
    ref = R.ddp_reference()
    kw = dict(ce_weight=R.DDP_COMBO[1], boundary_weight=R.DDP_COMBO[2], clip=R.DDP_COMBO[3])
    per_rank = R.boundary_ref(logits[2:], labels[2:], sd2[2:], weight, R.IGNORE, R.DDP_COMBO[1], R.DDP_COMBO[2], R.DDP_COMBO[3],
                              "foreground")
    assert float((per_rank["grad"] - ref["grad"][2:]).abs().max()) == 0.0      # rank 1 alone IS the global batch: rank 0 adds nothing
    assert not bool(R.valid_mask(labels[:2], 2).any()) and int(ref["sums"][3]) > 1000 and ref["abs_bd"] > 1000

    sl = slice(2 * rank, 2 * rank + 2)
    z = logits[sl].to(dev).requires_grad_(True)
    crit = BoundaryLoss(weight=weight, group=dist.group.WORLD, **kw).to(dev)
    loss = crit(z, labels[sl].to(dev))
    loss.backward()
    torch.cuda.synchronize()
    count = crit.last_valid.cpu().double().reshape(1)                          # N as this rank sees it
    losses = [torch.zeros(1) for _ in range(world)]
    dist.all_gather(losses, loss.detach().cpu().reshape(1))
    grads = [torch.zeros(2, 2, 65, 65) for _ in range(world)]
    dist.all_gather(grads, z.grad.cpu())
    allcounts = [torch.zeros(1, dtype=torch.float64) for _ in range(world)]
    dist.all_gather(allcounts, count)
    grad = torch.cat(grads)

    ok = True
    if rank == 0:
        z1 = logits.to(dev).requires_grad_(True)
        single = BoundaryLoss(weight=weight, **kw).to(dev)(z1, labels.to(dev))
        single.backward()
        bl, bg = 4 * R.FLOOR["loss.ddp"], 4 * R.FLOOR["grad.ddp"]
        e_loss = [R.rel_err(l, ref["loss"]) for l in losses]
        e_grad = R.rel_err(grad, ref["grad"])
        e_single = (R.rel_err(losses[0], single.detach().cpu()), R.rel_err(grad, z1.grad.cpu()))
        want = [float(ref["sums"][3])]
        print("BOUNDARY_DDP loss rank0 %.8f rank1 %.8f single %.8f float64 %.8f | rel err loss %.2e %.2e (bound %.1e) grad %.2e "
              "(bound %.1e) | vs single process: loss %.2e grad %.2e | N rank0 %s rank1 %s expected %s" %
              (float(losses[0]), float(losses[1]), float(single), float(ref["loss"]), e_loss[0], e_loss[1], bl, e_grad, bg,
               e_single[0], e_single[1], allcounts[0].tolist(), allcounts[1].tolist(), want), flush=True)
        ok = (float(losses[0]) == float(losses[1]) and max(e_loss) <= bl and e_grad <= bg and e_single[0] <= bl and
              e_single[1] <= bg and allcounts[0].tolist() == want and allcounts[1].tolist() == want and
              not bool(grads[0].any()))                                          # the all-ignored half: a gradient of exactly 0
    flag = torch.tensor([1.0 if ok else 0.0])
    dist.all_reduce(flag, op=dist.ReduceOp.MIN)
    dist.barrier()
    dist.destroy_process_group()
    sys.exit(0 if float(flag) == 1.0 else 1)


if __name__ == "__main__":
    main()
