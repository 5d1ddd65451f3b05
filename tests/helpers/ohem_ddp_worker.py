"""Worker of tests/test_ohem_ddp_gpu.py: launched twice by torch.distributed.run (gloo rendezvous, BOTH ranks on cuda:0).  Each
rank holds half of a batch of 4 and runs OhemCrossEntropyLoss(group=WORLD) forward and backward on it.  The first half holds easy
pixels only (nll <= 0.1), the second a hard third (nll in [1, 3]); min_kept is the number of hard pixels of the WHOLE batch, so a
selection made per rank would keep the hardest easy pixels on rank 0 -- a different set.  Asserted: loss, nu and |K| are identical
on both ranks; |K| is the hard population's size; nu, the loss and the two ranks' gradients, concatenated, equal the float64
restatement on the whole batch within 4 x the floor of these inputs (tests/ohem_ref.py's rule, measured here: the same formula in
fp32 torch ops against float64, at least 2^-24)."""
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
    from iswm_amd.utils.loss import OhemCrossEntropyLoss
    from tests import ohem_ref as R

    g = R.gen(23)
    b, h, w = 4, 37, 41
    labels = torch.randint(0, 2, (b, h, w), generator=g)
    hard = torch.rand(b, h, w, generator=g) < 1.0 / 3
    hard[:2] = False                                                 # ranks' halves: [0:2] easy only, [2:4] a third hard
    u = torch.rand(b, h, w, generator=g)
    lead = torch.where(hard, -2.9 + 2.3 * u, 3.0 + 3.0 * u)
    logits = torch.zeros(b, 2, h, w).scatter_(1, labels[:, None], lead[:, None])
    labels[torch.rand(b, h, w, generator=g) < 0.05] = R.IGNORE
    labels = labels.to(torch.uint8)
    nhard = int((hard & (labels != R.IGNORE)).sum())
    weight = torch.tensor([1.0, 3.0])
    thresh = R.GAP_NUK_THRESH                                        # nu_0 = 5: the k-th largest loss of the global batch decides
    ref = R.ohem_ref(logits, labels, weight, R.IGNORE, thresh, nhard)
    assert int(ref["sums"][2]) == nhard > 500 and torch.equal(ref["kept"], hard & ref["valid"])
    alone = R.ohem_ref(logits[:2], labels[:2], weight, R.IGNORE, thresh, nhard // 2)
    assert int(alone["sums"][2]) >= nhard // 2 and not bool(ref["kept"][:2].any())     # a per-rank selection keeps another set

    sl = slice(2 * rank, 2 * rank + 2)
    crit = OhemCrossEntropyLoss(thresh=thresh, min_kept=nhard, weight=weight, group=dist.group.WORLD).to(dev)
    z = logits[sl].to(dev).requires_grad_(True)
    loss = crit(z, labels[sl].to(dev))
    loss.backward()
    torch.cuda.synchronize()
    mine = torch.tensor([float(loss), float(crit.last_kept), float(crit.last_nu)], dtype=torch.float64)
    both = [torch.zeros(3, dtype=torch.float64) for _ in range(world)]
    dist.all_gather(both, mine)
    grads = [torch.zeros(2, 2, h, w) for _ in range(world)]
    dist.all_gather(grads, z.grad.cpu())
    grad = torch.cat(grads)

    ok = True
    if rank == 0:
        low = R.ohem_ref(logits, labels, weight, R.IGNORE, thresh, nhard, dtype=torch.float32, kept=ref["kept"])
        bl = 4 * max(R.rel_err(low["loss"], ref["loss"]), R.FLOOR_MIN)
        bg = 4 * max(R.rel_err(low["grad"], ref["grad"]), R.FLOOR_MIN)
        e_loss = [R.rel_err(v[0], ref["loss"]) for v in both]
        e_grad = R.rel_err(grad, ref["grad"])
        off = grad.permute(0, 2, 3, 1)[~ref["kept"]]
        bn = 4 * max(R.rel_err(torch.tensor(low["nu"], dtype=torch.float64), torch.tensor(ref["nu"], dtype=torch.float64)), R.FLOOR_MIN)
        e_nu = R.rel_err(both[0][2], torch.tensor(ref["nu"], dtype=torch.float64))
        print("OHEM_DDP loss rank0 %.8f rank1 %.8f float64 %.8f | nu rank0 %.8f rank1 %.8f float64 %.8f | kept rank0 %d rank1 %d hard "
              "pixels %d | rel err loss %.2e %.2e (bound %.1e) nu %.2e (bound %.1e) grad %.2e (bound %.1e)" %
              (float(both[0][0]), float(both[1][0]), float(ref["loss"]), float(both[0][2]), float(both[1][2]), ref["nu"],
               int(both[0][1]), int(both[1][1]), nhard, e_loss[0], e_loss[1], bl, e_nu, bn, e_grad, bg), flush=True)
        ok = (torch.equal(both[0], both[1]) and int(both[0][1]) == nhard and max(e_loss) <= bl and e_nu <= bn and e_grad <= bg
              and not bool(off.any()))
    flag = torch.tensor([1.0 if ok else 0.0])
    dist.all_reduce(flag, op=dist.ReduceOp.MIN)
    dist.barrier()
    dist.destroy_process_group()
    sys.exit(0 if float(flag) == 1.0 else 1)


if __name__ == "__main__":
    main()
