"""Isolated time and output hashes of the round-1 conv kernels (conv_tile32.h) at geometries where the planner names them.

    python tools/tile32_ab.py [rounds] > pass.txt                   one pass on the library of this tree (one process per build)
    python tools/tile32_ab.py --compare A.txt A2.txt B.txt [B2.txt]  the table of profiles/tile32_refactor_ab.txt from such passes

A pass prints, per row: conv math, geometry, direction, the kernel the planner names, the median of `rounds` launches (HIP
events on the launch stream, after 3 warm-up launches) and a SHA-256 of the output, so two builds are compared bit for bit at
every timed shape.  fp32 operands throughout (no planes), as the MobileNetV2 1x1s with a gathered channel count off 64 and conv
math 0 run.  The weight is packed / transposed once, outside the timed calls.  --compare: margin = the largest relative gap
between the two parent passes (A, A2) over the rows; a row is SLOWER when mean(B) > mean(A) x (1 + margin); any differing hash
between the passes is reported."""
import hashlib
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1] != "--compare" else 20
ROWS = [  # conv_ref mode, geometry (n, h, w, cin, cout, k, stride, pad, dil)
    ("f32", (16, 33, 33, 1024, 256, 1, 1, 0, 1)), ("f32", (16, 33, 33, 256, 256, 3, 1, 1, 1)), ("f32", (16, 33, 33, 2048, 256, 3, 1, 12, 12)),
    ("f32", (16, 129, 129, 64, 256, 1, 1, 0, 1)), ("f32", (16, 129, 129, 256, 64, 1, 1, 0, 1)), ("f32", (16, 65, 65, 128, 512, 1, 1, 0, 1)),
    ("f32", (16, 65, 65, 512, 128, 1, 1, 0, 1)), ("f32", (16, 129, 129, 48, 256, 1, 1, 0, 1)), ("f32", (16, 129, 129, 256, 48, 1, 1, 0, 1)),
    ("f32", (16, 33, 33, 304, 48, 1, 1, 0, 1)), ("f32", (16, 33, 33, 48, 304, 1, 1, 0, 1)),
    ("x6", (16, 129, 129, 32, 192, 1, 1, 0, 1)), ("x6", (16, 129, 129, 16, 96, 1, 1, 0, 1)), ("x6", (16, 65, 65, 96, 576, 1, 1, 0, 1)),
    ("x6", (16, 65, 65, 576, 160, 1, 1, 0, 1)), ("x6", (16, 33, 33, 160, 960, 1, 1, 0, 1)), ("x6", (16, 33, 33, 384, 96, 1, 1, 0, 1)),
    ("x6", (16, 257, 257, 16, 96, 1, 1, 0, 1)), ("x6", (16, 65, 65, 144, 32, 1, 1, 0, 1)), ("x6", (16, 65, 65, 128, 256, 3, 2, 1, 1)),
    ("bf16", (16, 129, 129, 32, 192, 1, 1, 0, 1)), ("bf16", (16, 33, 33, 160, 960, 1, 1, 0, 1)), ("bf16", (16, 257, 257, 16, 96, 1, 1, 0, 1)),
    ("bf16", (16, 33, 33, 384, 96, 1, 1, 0, 1)),
    # plain-weight arm of k_conv_x6 (ops._USE_PACKED off): 64 x 64, 128 x 64 both directions, 128 x 128 forward
    ("plain", (16, 33, 33, 384, 96, 1, 1, 0, 1)), ("plain", (1, 79, 79, 64, 512, 1, 1, 0, 1)), ("plain", (1, 221, 222, 16, 96, 1, 1, 0, 1)),
    ("plain", (1, 362, 363, 128, 128, 3, 1, 1, 1)),
]


def med(fn):
    import torch
    for _ in range(3):
        fn()
    a = [torch.cuda.Event(enable_timing=True) for _ in range(ROUNDS)]
    b = [torch.cuda.Event(enable_timing=True) for _ in range(ROUNDS)]
    for i in range(ROUNDS):
        a[i].record()
        fn()
        b[i].record()
    torch.cuda.synchronize()
    ts = sorted(x.elapsed_time(y) * 1e3 for x, y in zip(a, b))
    return ts[len(ts) // 2]


def sha(t):
    return hashlib.sha256(t.detach().float().contiguous().cpu().numpy().tobytes()).hexdigest()[:16]


def one_pass():
    import torch
    from iswm_amd import _lib, ops
    dev = torch.device("cuda:0")
    lib = _lib.load()
    old = lib.iswm_get_conv_math()
    for mode, geom in ROWS:
        n, h, w, cin, cout, k, s, p, d = geom
        ops._USE_PACKED = mode != "plain"
        lib.iswm_set_conv_math({"f32": 0, "x6": 1, "plain": 1, "bf16": 2}[mode])
        gen = torch.Generator().manual_seed(5)
        x = torch.randn(n, h, w, cin, generator=gen).to(dev)
        wt = (torch.randn(cout, k, k, cin, generator=gen) * 0.05).to(dev)
        g = ops.ConvGeom(x, cout, k, k, s, p, d)
        dy = torch.randn(n, g.ho, g.wo, cout, generator=gen).to(dev)
        desc = g.desc(cin, cout)
        plans = [ops.conv_plan(desc, op, False) for op in ("fwd", "dgrad")]       # the plan the wrappers take, and its kernel
        wh = [ops.ConvWeight(wt, {pl.wform: ops.conv_weight(wt, pl, desc, dirn)}) for dirn, pl in enumerate(plans)]
        y = torch.empty(n, g.ho, g.wo, cout, device=dev)
        dx = torch.zeros(n, h, w, cin, device=dev)
        tf = med(lambda: ops.conv2d_fwd(x, wh[0], g, out=y, want_stats=True))
        st = ops.conv2d_fwd(x, wh[0], g, out=y, want_stats=True)[1]
        td = med(lambda: ops.conv2d_dgrad(dy, wh[1], g, (n, h, w, cin), dx=dx))
        tag = "%-5s n%d %dx%d c%d->%d k%d s%d d%d" % (mode, n, h, w, cin, cout, k, s, d)
        print("%-40s fwd   %-38s %8.1f us  y %s stats %s" % (tag, plans[0].name, tf, sha(y), sha(st) if st is not None else "-"), flush=True)
        print("%-40s dgrad %-38s %8.1f us  dx %s" % (tag, plans[1].name, td, sha(dx)), flush=True)
    ops._USE_PACKED = True
    lib.iswm_set_conv_math(old)


def load(path):
    rows = []
    for ln in open(path):
        m = re.match(r"(.{40}) (fwd  |dgrad) (.{38})\s+([\d.]+) us\s+(.*)$", ln.rstrip())
        if m:
            rows.append((m.group(1).strip() + " " + m.group(2).strip(), m.group(3).strip(), float(m.group(4)), m.group(5)))
    return rows


def compare(paths):
    a, a2, bs = load(paths[0]), load(paths[1]), [load(p) for p in paths[2:]]
    assert a and all(len(t) == len(a) for t in [a2] + bs), "the passes differ in their rows"
    margin = max(abs(x[2] - y[2]) / min(x[2], y[2]) for x, y in zip(a, a2))
    slower = differ = 0
    for i, (x, y) in enumerate(zip(a, a2)):
        par, new = (x[2] + y[2]) / 2, sum(t[i][2] for t in bs) / len(bs)
        ok, same = new <= par * (1 + margin), all(t[i][3] == x[3] and t[i][1] == x[1] for t in [a2] + bs)
        slower, differ = slower + (not ok), differ + (not same)
        print("%-46s %-38s %8.1f %8.1f " % (x[0], x[1], x[2], y[2]) + " ".join("%8.1f" % t[i][2] for t in bs) +
              "  %+6.2f%%  %s  %s" % (100 * (new / par - 1), "ok" if ok else "SLOWER", "bits equal" if same else "BITS DIFFER"))
    print("margin (largest |A - A'| / min over the rows) %.2f%%; rows with mean(B) above mean(A, A') x (1 + margin): %d; rows whose "
          "hashes or kernel names differ between the passes: %d" % (100 * margin, slower, differ))
    print("sum of the rows (us): A %.1f  A' %.1f  " % (sum(x[2] for x in a), sum(x[2] for x in a2)) +
          "  ".join("B%s %.1f" % ("'" * i, sum(x[2] for x in t)) for i, t in enumerate(bs)))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--compare":
        compare(sys.argv[2:])
    else:
        one_pass()
