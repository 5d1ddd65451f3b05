"""Worker of tests/test_lovasz_ddp_gpu.py: launched twice by torch.distributed.run (gloo rendezvous, BOTH ranks on cuda:0).  Each
rank holds two images of a batch of 4 and runs LovaszSoftmaxLoss(ce_weight=1, group=WORLD) forward and backward on them.  One
image of rank 1 has no foreground, so N = 3 over the whole batch against 2 and 1 on the ranks alone: a normaliser taken per rank
gives another loss and other gradients.  Asserted: loss and N are identical on both ranks; N = 3; the loss and the two ranks'
gradients, concatenated, equal the float64 restatement on the four-image batch (evaluated on the order the kernels chose, which
each rank reports) within 4 x the floor of these inputs (tests/lovasz_ref.py's rule, measured here: the same formula in fp32
torch ops against float64, at least 2^-24)."""
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
    from iswm_amd import ops
    from iswm_amd.utils.loss import LovaszSoftmaxLoss
    from tests import lovasz_ref as R

    g = R.gen(29)
    b, h, w = 4, 37, 41
    labels = (torch.rand(b, h, w, generator=g) < 0.2).long()
    labels[3] = 0                                                    # rank 1's second image: no foreground
    logits = torch.randn(b, 2, h, w, generator=g)
    logits[:, 1] += 2.0 * labels.float() - 1.0
    labels[torch.rand(b, h, w, generator=g) < 0.05] = R.IGNORE
    labels = labels.to(torch.uint8)
    weight = torch.tensor([1.0, 3.0])
    lce, llv, up = 1.0, 0.8, R.UPSTREAM
    ref = R.lovasz_ref(logits, labels, weight, R.IGNORE, "foreground", lce, llv, upstream=up)
    assert ref["N"] == 3
    halves = [R.lovasz_ref(logits[s], labels[s], weight, R.IGNORE, "foreground", lce, llv) for s in (slice(0, 2), slice(2, 4))]
    assert [r["N"] for r in halves] == [2, 1]

    sl = slice(2 * rank, 2 * rank + 2)
    crit = LovaszSoftmaxLoss(ce_weight=lce, lovasz_weight=llv, weight=weight, group=dist.group.WORLD).to(dev)
    z = logits[sl].to(dev).requires_grad_(True)
    loss = crit(z, labels[sl].to(dev))
    (loss * up).backward()
    keys, _, _ = ops.lovasz_keys(logits[sl].to(dev), labels[sl].to(dev), None, R.IGNORE, "foreground")
    perm = ops.lovasz_sort(keys)[1].cpu().long().reshape(2, 1, h * w)
    torch.cuda.synchronize()
    mine = torch.tensor([float(loss.detach()), float(crit.last_present)], dtype=torch.float64)
    both = [torch.zeros(2, dtype=torch.float64) for _ in range(world)]
    dist.all_gather(both, mine)
    grads = [torch.zeros(2, 2, h, w) for _ in range(world)]
    dist.all_gather(grads, z.grad.cpu())
    perms = [torch.zeros(2, 1, h * w, dtype=torch.int64) for _ in range(world)]
    dist.all_gather(perms, perm)
    grad = torch.cat(grads)

    ok = True
    if rank == 0:
        pin = R.lovasz_ref(logits, labels, weight, R.IGNORE, "foreground", lce, llv, upstream=up, perm=torch.cat(perms))
        low = R.lovasz_ref(logits, labels, weight, R.IGNORE, "foreground", lce, llv, dtype=torch.float32, upstream=up,
                           perm=ref["perm"])
        bl = 4 * max(R.rel_err(low["loss"], ref["loss"]), R.FLOOR_MIN)
        bg = 4 * max(R.rel_err(low["grad"], ref["grad"]), R.FLOOR_MIN)
        e_loss = [R.rel_err(v[0], ref["loss"]) for v in both]
        e_grad = R.rel_err(grad, pin["grad"])
        alone = [float(r["loss"]) for r in halves]
        off = grad.permute(0, 2, 3, 1)[~ref["valid"].reshape(b, h, w)]
        print("LOVASZ_DDP loss rank0 %.8f rank1 %.8f float64 %.8f (the ranks alone: %.8f %.8f) | N rank0 %d rank1 %d | rel err loss "
              "%.2e %.2e (bound %.1e) grad %.2e (bound %.1e)" %
              (float(both[0][0]), float(both[1][0]), float(ref["loss"]), alone[0], alone[1], int(both[0][1]), int(both[1][1]),
               e_loss[0], e_loss[1], bl, e_grad, bg), flush=True)
        ok = (torch.equal(both[0], both[1]) and int(both[0][1]) == 3 and max(e_loss) <= bl and e_grad <= bg
              and not bool(off.any()))
    flag = torch.tensor([1.0 if ok else 0.0])
    dist.all_reduce(flag, op=dist.ReduceOp.MIN)
    dist.barrier()
    dist.destroy_process_group()
    sys.exit(0 if float(flag) == 1.0 else 1)


if __name__ == "__main__":
    main()
