"""Worker of tests/test_optim_ext_ddp_gpu.py: launched twice by torch.distributed.run (gloo rendezvous, both ranks on cuda:0, as
tests/helpers/ddp_parity_worker.py).  Each rank trains three steps on its half of a global batch through
DistributedDataParallelHIP, the globally normalised criterion and FusedSGD with gradient clipping and EMA weights.  It prints
three result lines and exits 0 unless something raised; the tests read the lines.

OPTIM_EXT_DDP_RANKS   after the three steps the weight arena, the EMA arena and every step's last_grad_norm are BIT-IDENTICAL on
                      both ranks (each replica computes the clip factor from the same all-reduced gradients, with a reduction
                      whose result does not depend on timing or placement), and every step really clipped.
Rank 0 then replays the steps in one process by ddp_parity_worker's method -- both halves, local BatchNorm per half, the
per-half gradients of the GLOBAL weighted-mean loss summed -- and compares per parameter tensor, max |a - b| / max |b|, with that
worker's figure, 1e-5:
OPTIM_EXT_DDP_STEP    every step on its own: the replay of step t starts from the DDP run's state after step t - 1 (weights,
                      momentum, EMA copied bit for bit), exactly the situation ddp_parity_worker compares; gradient arena,
                      weights, EMA and the norm after the step.
OPTIM_EXT_DDP_FREE    the three steps free-running from the broadcast state; weights, EMA and the norms after step 3."""
import os
import sys

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

STEPS, MAX_NORM, DECAY, TOL = 3, 0.1, 0.9, 1e-5


def main():
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    from iswm_amd import ops
    from iswm_amd.network import modeling
    from iswm_amd.optim import FusedSGD
    from iswm_amd.parallel import DistributedDataParallelHIP
    from iswm_amd.utils.loss import CrossEntropyLoss

    def build():
        m = modeling.deeplabv3plus_resnet50(num_classes=2, output_stride=16).to(dev).train()
        m.classifier.aspp.project[3].p = 0.0           # dropout off: its counter-based masks depend on the call index
        return m

    def optimizer(m):
        opt = FusedSGD(m.parameters(), momentum=0.9, weight_decay=1e-4, nesterov=True)
        opt.set_grad_clip(MAX_NORM)
        opt.enable_ema(DECAY)
        return opt

    def state(opt):
        return dict(norm=float(opt.last_grad_norm), grad=opt.arena.grad.clone(), data=opt.arena.data.clone(),
                    buf=opt._buf.clone(), ema=opt._ema.clone())

    # The state, batch and tile size of tests/test_hip_modules.py::test_train_steps_match_oracle, the project's three-step
    # comparison, and for its reasons: the synthetic state with the residual branches damped (bn3.weight x 0.3) and 6 images
    # of 81 x 81 per BatchNorm batch (the ASPP image-pooling BatchNorm normalises over `batch` values per channel).  A randomly
    # initialised network at 4 x 65 x 65 per rank turns the few-ulp weight differences two fp32 runs have after one step
    # into gradient differences of 0.2 of a tensor's scale at the next (measured), and no two runs agree there.
    from oracle.synth import ArchCfg, synth_images, synth_labels, synth_state_dict
    torch.manual_seed(100 + rank)                      # different init per rank: the broadcast must fix it
    model = build()
    if rank == 0:
        sd = synth_state_dict(ArchCfg("deeplabv3plus", "resnet50", 2, 16))
        model.load_state_dict({k: (v * 0.3 if k.endswith(".bn3.weight") else v) for k, v in sd.items()}, strict=True)
    H = 6                                              # images per rank
    xs = [synth_images(2 * H, 81, 81, seed=100 + t) for t in range(STEPS)]
    labs = []
    for t in range(STEPS):
        lab = synth_labels(2 * H, 81, 81, seed=100 + t, p_fg=0.2, p_ignore=0.05).to(torch.int64)
        lab[:H, :40] = 0                               # unequal class mix per half -> different local normalisers
        labs.append(lab)
    w = torch.tensor([1.0, 3.0])

    net = DistributedDataParallelHIP(model, process_group=dist.group.WORLD, bucket_mb=8.0)
    init = {k: v.detach().clone() for k, v in model.state_dict().items()}          # after the rank-0 broadcast
    opt = optimizer(model)                             # the EMA starts from the broadcast weights
    net.attach(opt)
    crit = CrossEntropyLoss(weight=w, ignore_index=255, group=dist.group.WORLD).to(dev)
    sl = slice(H * rank, H * rank + H)
    rec = []
    for x, lab in zip(xs, labs):
        loss = crit(net(x[sl].to(dev)), lab[sl].to(dev))
        opt.zero_grad()
        loss.backward()
        opt.step()                                     # the attached pre-hook finishes the all-reduce first
        rec.append(state(opt) if rank == 0 else dict(norm=float(opt.last_grad_norm)))
    torch.cuda.synchronize()
    norms = torch.tensor([r["norm"] for r in rec], dtype=torch.float32, device=dev)
    clipped = all(r["norm"] > MAX_NORM for r in rec)                                # every step must really clip
    mine = torch.cat([opt.arena.data, opt._ema, norms]).cpu()
    gathered = [torch.empty_like(mine) for _ in range(world)]
    dist.all_gather(gathered, mine)
    equal = bool(torch.equal(gathered[0].view(torch.int32), gathered[1].view(torch.int32)))

    if rank == 0:
        print("OPTIM_EXT_DDP_RANKS ok=%d replicas_equal %s clipped %s norms %s" %
              (equal and clipped, equal, clipped, ["%.4f" % r["norm"] for r in rec]), flush=True)
        local = CrossEntropyLoss(weight=w, ignore_index=255).to(dev)
        halves = (slice(0, H), slice(H, 2 * H))
        names = [k for k, _ in model.named_parameters()]

        def worst(opt_a, flat_a, flat_b):
            """largest per-tensor max |a - b| / max |b| over the parameters' ranges of two flat buffers"""
            out = (0.0, "")
            for i, k in enumerate(names):
                a, b = opt_a.arena.view_of(flat_a, i), opt_a.arena.view_of(flat_b, i)
                out = max(out, (float((a - b).abs().max()) / max(float(b.abs().max()), 1e-30), k))
            return out

        for forced in (True, False):
            ref = build()
            ref.load_state_dict(init, strict=True)
            ropt = optimizer(ref)
            figs = []
            for t, (x, lab) in enumerate(zip(xs, labs)):
                if forced and t > 0:                   # start this step from the DDP run's state after the previous one
                    ropt.arena.data.copy_(rec[t - 1]["data"])
                    ropt._buf.copy_(rec[t - 1]["buf"])
                    ropt._ema.copy_(rec[t - 1]["ema"])
                    ops.weights_changed()
                valid = lab != 255
                den = [float(w[lab[h][valid[h]]].sum()) for h in halves]
                acc = None
                for h, dh in zip(halves, den):
                    ropt.zero_grad()
                    lh = local(ref(x[h].to(dev)), lab[h].to(dev))            # weighted mean over THIS half
                    (lh * (dh / sum(den))).backward()                        # its share of the global weighted mean
                    gs = [p.grad.detach().clone() for p in ref.parameters()]
                    acc = gs if acc is None else [a + b for a, b in zip(acc, gs)]
                ropt.zero_grad()
                for p, a in zip(ref.parameters(), acc):
                    p.grad = a
                ropt.step()
                r = rec[t]
                figs.append(dict(grad=worst(ropt, ropt.arena.grad, r["grad"]), data=worst(ropt, ropt.arena.data, r["data"]),
                                 ema=worst(ropt, ropt._ema, r["ema"]),
                                 norm=abs(float(ropt.last_grad_norm) - r["norm"]) / r["norm"]))
            if forced:
                ok = all(f["grad"][0] <= TOL and f["data"][0] <= TOL and f["ema"][0] <= TOL and f["norm"] <= TOL for f in figs)
                print("OPTIM_EXT_DDP_STEP ok=%d " % ok + "; ".join(
                    "step %d grad %.2e (%s) weights %.2e ema %.2e norm %.2e" %
                    (t + 1, f["grad"][0], f["grad"][1], f["data"][0], f["ema"][0], f["norm"]) for t, f in enumerate(figs)), flush=True)
            else:
                f = figs[-1]
                n_err = max(q["norm"] for q in figs)
                ok = f["data"][0] <= TOL and f["ema"][0] <= TOL and n_err <= TOL
                print("OPTIM_EXT_DDP_FREE ok=%d after step %d: weights %.3e (%s) ema %.3e (%s) norm %.3e; gradient arena per step %s" %
                      (ok, STEPS, f["data"][0], f["data"][1], f["ema"][0], f["ema"][1], n_err,
                       ["%.2e" % q["grad"][0] for q in figs]), flush=True)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
