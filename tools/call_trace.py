#!/usr/bin/env python
"""The library calls of a few small training / inference runs, in order, and hashes of what they computed.

    python tools/call_trace.py [-o out.json] [--size H W] [--cases a,b] [--dump-traces]

Wraps `_lib.call` (and the name `ops.call` is bound to) and records, per call, the entry point with every scalar argument,
every descriptor's fields and every ctypes int array; pointers only as null / non-null.  Per case and conv math 0 / 1 / 2 it
runs one training step (forward, weighted CE, backward), one eval-mode forward and one no_grad training-mode forward at
batch 2 (seeded) and writes the number of calls, a SHA-256 of the trace and a SHA-256 each of the loss, the logits (train /
eval / no_grad) and all parameter gradients.  Two commits whose files agree make the same launches and compute the same bits
in these runs (profiles/host_plan_trace.txt).  One name is left out: iswm_conv2d_fwd_packed_stat_layout, a pure host query that
happens to go through `call` -- how often the wrappers ask it is not a launch.  Imports only what every commit since the route
planner has."""
import argparse
import ctypes
import hashlib
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from iswm_amd import _lib, ops  # noqa: E402
from iswm_amd.network import _deeplab, modeling  # noqa: E402
from iswm_amd.utils.loss import CrossEntropyLoss  # noqa: E402


def _separable():
    m = modeling.deeplabv3plus_resnet50(num_classes=2, output_stride=16)
    m.classifier = _deeplab.convert_to_separable_conv(m.classifier)
    return m


CASES = {
    "deeplabv3plus_resnet50_os16": lambda: modeling.deeplabv3plus_resnet50(num_classes=2, output_stride=16),
    "deeplabv3_resnet50_os8": lambda: modeling.deeplabv3_resnet50(num_classes=2, output_stride=8),
    "deeplabv3plus_mobilenet_os16": lambda: modeling.deeplabv3plus_mobilenet(num_classes=2, output_stride=16),
    "deeplabv3plus_resnet50_os16_separable": _separable,
}


def _arg(a):
    """one argument in its recorded form"""
    if a is None:
        return "null"
    if isinstance(a, (bool, int, float)):
        return a
    if isinstance(a, ctypes.c_void_p):
        return "ptr" if a.value else "null"
    if isinstance(a, ctypes.Array):
        if a._type_ is ctypes.c_void_p:
            return ["ptr" if v else "null" for v in a]
        return [v for v in a]
    obj = getattr(a, "_obj", a)                       # byref(struct)
    if isinstance(obj, ctypes.Structure):
        return {n: getattr(obj, n) for n, _ in obj._fields_}
    if isinstance(obj, ctypes._SimpleCData):
        return "out"                                  # byref(c_int): an output of a host query
    raise TypeError("call_trace: unrecorded argument type %r" % (type(a),))


HOST_QUERIES = ("iswm_conv2d_fwd_packed_stat_layout",)


class Trace(object):
    def __init__(self):
        self.calls, self.real = [], _lib.call

    def __enter__(self):
        def spy(name, *args):
            if name not in HOST_QUERIES:
                self.calls.append([name] + [_arg(a) for a in args])
            return self.real(name, *args)
        _lib.call = ops.call = spy
        return self

    def __exit__(self, *exc):
        _lib.call = ops.call = self.real
        return False


def sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().float().contiguous().cpu().numpy().tobytes())
    return h.hexdigest()


def run_case(make, math, size, dev):
    lib = _lib.load()
    lib.iswm_set_conv_math(math)
    torch.manual_seed(7)
    m = make().to(dev).train()
    g = torch.Generator(device="cpu").manual_seed(11)
    x = torch.randn(2, 3, size[0], size[1], generator=g).to(dev)
    lab = (torch.rand(2, size[0], size[1], generator=g) < 0.2).to(torch.int64).to(dev)
    crit = CrossEntropyLoss(weight=torch.tensor([1.0, 3.0]), ignore_index=255).to(dev)
    with Trace() as tr:
        logits = m(x)
        loss = crit(logits, lab)
        loss.backward()
        m.eval()
        with torch.no_grad():
            ev = m(x)
        m.train()
        with torch.no_grad():
            ng = m(x)
        torch.cuda.synchronize()
    text = json.dumps(tr.calls, sort_keys=True)
    return dict(calls=len(tr.calls), trace=hashlib.sha256(text.encode()).hexdigest(),
                aspp_fwd=sum(c[0] == "iswm_aspp_fwd" for c in tr.calls), loss=sha(loss), logits=sha(logits), eval=sha(ev),
                no_grad=sha(ng), grads=sha(*[p.grad for _, p in sorted(m.named_parameters()) if p.grad is not None])), tr.calls


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("-o", "--output")
    ap.add_argument("--size", type=int, nargs=2, default=(97, 129))
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--dump-traces", action="store_true", help="keep the full call lists in the output (large)")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    old = _lib.load().iswm_get_conv_math()
    out = {}
    for name in a.cases.split(","):
        for math in (0, 1, 2):
            res, calls = run_case(CASES[name], math, a.size, dev)
            if a.dump_traces:
                res["calls_list"] = calls
            out["%s.math%d" % (name, math)] = res
            print("%-46s calls %5d aspp_fwd %d trace %s loss %s grads %s" % ("%s.math%d" % (name, math), res["calls"],
                  res["aspp_fwd"], res["trace"][:12], res["loss"][:12], res["grads"][:12]), flush=True)
    _lib.load().iswm_set_conv_math(old)
    if a.output:
        with open(a.output, "w") as f:
            json.dump({"size": list(a.size), "cases": out}, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
