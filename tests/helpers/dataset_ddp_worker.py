"""Worker of tests/test_dataset_gpu.py::test_two_ranks_share_weights_and_split_the_epoch: launched twice by
torch.distributed.run (gloo rendezvous, BOTH ranks on cuda:0 -- the only GPU a test box has).  Each rank builds the
resident train store, counts its own batches of epoch 0 with calculate_class_weights_resident over the group, and
prints the weights and the tile indices it was given."""
import argparse
import os
import random
import sys

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main():
    root, batch, seed = sys.argv[1], int(sys.argv[2]), int(sys.argv[3])
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    from iswm_amd import train
    from iswm_amd.datasets import BinarySegmentation, DeviceTileStore
    from iswm_amd.utils import ext_transforms as et
    from iswm_amd.utils.loss import calculate_class_weights_resident
    store = DeviceTileStore(BinarySegmentation(root, "train"), dev, workers=2)
    comp = train._train_transform(argparse.Namespace(crop_size=65), et)
    random.seed(seed)
    mine = train.epoch_batches(len(store), batch, seed, 0, rank, world)
    w = calculate_class_weights_resident((comp.batch_resident(store, idx) for idx in mine), dist.group.WORLD)
    sys.stdout.write("DSDDP rank=%d n=%d weights=%r idx=%r\n" % (rank, len(store), [float(v) for v in w], mine))
    sys.stdout.flush()                 # one write per rank: the two ranks share a pipe
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
