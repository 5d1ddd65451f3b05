#!/usr/bin/env python
"""One SHA-256 per output of the loss kernels (csrc/loss.hip) on seeded inputs: do two commits compute the same bits?

    python tools/loss_bits.py [-o out.txt]

Run it on both trees on the same GPU and compare the files line by line (profiles/loss_refactor_bits.txt).  It imports `ops`
and tests/streaming_ref.loss_inputs only -- what every commit since the hard-pixel loss has -- so the same file runs on both.
Inputs: loss_inputs (ignored, negative and out-of-range labels planted), labels as uint8 and int64, with and without class
weights, at (1, 3, 5) = one thread group with a ragged unroll tail, (2, 33, 37) = 3 blocks and (2, 129, 131) = 34 blocks with a
ragged tail.
    ce       C in {2, 3, 8, 9, 21} (registers, the register limit, the streamed class axis) x modes 0, 1, 2 x (alpha, gamma) in
             {(1, 0), (0.25, 2), (1, 0.5)}: loss, sums, and the gradient after loss_bwd_scale with upstream 0.37
    overlap  C in {2, 3, 8}, (ce_weight 1, overlap_weight 1, alpha 0.3, beta 0.7, gamma 0.75, smooth 1) x both class sets:
             sums, loss, coef, gradient (upstream 0.37)
    ohem     C in {2, 3, 8}, thresh 0.7 with min_kept = npix // 4 and thresh 1.0 with min_kept 0: keys, nvalid, nu, sums, the
             ohem_loss output, gradient (upstream 0.37)"""
import argparse
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402
from iswm_amd import ops  # noqa: E402
from streaming_ref import IGNORE, loss_inputs  # noqa: E402

SHAPES = [(1, 3, 5), (2, 33, 37), (2, 129, 131)]
UPSTREAM = 0.37


def sha(t):
    t = t.detach().contiguous().cpu()
    return hashlib.sha256(t.numpy().tobytes()).hexdigest()


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("-o", "--out", default=None)
    o = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("loss_bits.py hashes what the kernels compute; there is nothing to hash without a GPU")
    dev = torch.device("cuda:0")
    lines = []

    def emit(case, **outs):
        for k, v in outs.items():
            lines.append("%-44s %-8s %s" % (case, k, sha(v)))

    up = torch.tensor([UPSTREAM], dtype=torch.float32, device=dev)
    for shape in SHAPES:
        npix = shape[0] * shape[1] * shape[2]
        for kind in ("u8", "i64"):
            for wt in (False, True):
                tag = "%dx%dx%d %s %s" % (shape + (kind, "w" if wt else "now"))
                for c in (2, 3, 8, 9, 21):
                    z, y, w = (t.to(dev) for t in loss_inputs(c, kind, shape))
                    w = w if wt else None
                    for mode in (0, 1, 2):
                        for alpha, gamma in ((1.0, 0.0), (0.25, 2.0), (1.0, 0.5)):
                            loss, sums, grad = ops.loss_fwd(z, y, w, IGNORE, alpha, gamma, mode)
                            loss, sums = loss.clone(), sums.clone()
                            ops.loss_bwd_scale(grad, sums, up, mode, npix)
                            emit("ce c%d %s m%d a%g g%g" % (c, tag, mode, alpha, gamma), loss=loss, sums=sums, grad=grad)
                    if c > 8:
                        continue
                    osums = ops.overlap_loss_fwd(z, y, w, IGNORE)
                    for classes in ("foreground", "all"):
                        loss, coef = ops.overlap_loss_coeffs(osums, c, 1.0, 1.0, 0.3, 0.7, 0.75, 1.0, classes)
                        grad = ops.overlap_loss_bwd(z, y, w, IGNORE, coef, up)
                        emit("overlap c%d %s %s" % (c, tag, classes), sums=osums, loss=loss, coef=coef, grad=grad)
                    for thresh, min_kept in ((0.7, npix // 4), (1.0, 0)):
                        keys, nvalid = ops.ohem_keys(z, y, IGNORE)
                        nu = ops.ohem_select(keys, nvalid, min_kept, thresh)
                        hsums = ops.ohem_sums(keys, y, w, nu)
                        out = ops.ohem_loss(hsums)
                        grad = ops.ohem_bwd(z, y, w, keys, nu, out, up)
                        emit("ohem c%d %s t%g k%d" % (c, tag, thresh, min_kept), keys=keys, nvalid=nvalid, nu=nu, sums=hsums,
                             out=out, grad=grad)
    torch.cuda.synchronize()
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    sys.stdout.write("# %d hashes, all of them together: %s\n" % (len(lines), hashlib.sha256(text.encode()).hexdigest()))
    if o.out:
        if os.path.dirname(o.out):
            os.makedirs(os.path.dirname(o.out), exist_ok=True)
        with open(o.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
