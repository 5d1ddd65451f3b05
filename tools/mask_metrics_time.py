"""Time the sequence-validation evaluators: the device path (StreamMetrics with sliding windows, and the batched per-frame
kernels) against the CPU restatement of the reference's host path (tests/mask_metrics_ref.py) on N frames at 513².

    python tools/mask_metrics_time.py [--frames 32] [--size 513] [--seq 7] [--cpu-frames 8]

Prints one JSON line.  Device times: host clock around work that ends in torch.cuda.synchronize(), after a warm-up run of
the same shapes.  The CPU restatement is timed on --cpu-frames windows (it is slow) and reported per window; it runs the
reference's call graph literally, recomputing per-frame work for every window a frame belongs to.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from iswm_amd import ops  # noqa: E402
from iswm_amd.metrics import StreamMetrics  # noqa: E402
from tests import mask_metrics_ref as R  # noqa: E402


def wave_frames(n, s, seed):
    """a wave front moving right, with blob noise, in every frame"""
    rng = np.random.default_rng(seed)
    out = np.zeros((n, s, s), np.uint8)
    for t in range(n):
        x0 = s // 8 + 3 * t
        out[t, s // 10:s - s // 10, x0:x0 + s // 3] = 1
        coarse = rng.random((s // 16 + 1, s // 16 + 1)) < 0.03
        out[t] |= np.kron(coarse, np.ones((16, 16), np.uint8))[:s, :s].astype(np.uint8)
    return out


def run_device(G, P, L):
    m = StreamMetrics(2, sequence_length=L)
    for i in range(G.shape[0] - L + 1):
        m.update(G[i:i + L], P[i:i + L], sequence_data=True)
    return m.get_results()


def run_batched(G, P):
    """every per-frame / per-pair quantity of N frames in batched launches"""
    pv, pw, _ = ops.mask_preprocess(ops.mask_preprocess(P)[0])
    gv, gw, _ = ops.mask_preprocess(ops.mask_preprocess(G)[0])
    pf, ps = ops.mask_fronts(pv, pw)
    gf, gs = ops.mask_fronts(gv, gw)
    ops.front_error(pf, gf, P.shape[-1] * 0.1)
    ops.mask_pair_scores(pf, ps, gv, gw, gs)
    ops.mask_pair_scores(pf[1:], ps[1:], pv[:-1], pw[:-1], ps[:-1])
    ops.region_score(P, G)


def timed(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--size", type=int, default=513)
    ap.add_argument("--seq", type=int, default=7)
    ap.add_argument("--cpu-frames", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU")
    n, s, L = a.frames, a.size, a.seq
    gt = wave_frames(n, s, 1)
    pr = wave_frames(n, s, 2)
    G, P = torch.as_tensor(gt).cuda(), torch.as_tensor(pr).cuda().to(torch.int64)
    windows = n - L + 1
    res = run_device(G, P, L)
    run_batched(G, P)
    t_stream = timed(lambda: run_device(G, P, L), a.reps)
    t_batched = timed(lambda: run_batched(G, P), a.reps)

    nc = min(a.cpu_frames + L - 1, n)
    ref = R.StreamMetrics(2, sequence_length=L)
    t0 = time.perf_counter()
    for i in range(nc - L + 1):
        ref.update(gt[i:i + L], pr[i:i + L])
    t_cpu = (time.perf_counter() - t0) / (nc - L + 1)
    dev_small = run_device(G[:nc], P[:nc], L)
    want = ref.get_results()
    worst = max(abs(float(dev_small[k]) - float(want[k])) / max(1.0, abs(float(want[k]))) for k in want)
    print(json.dumps({
        "frames": n, "size": s, "sequence_length": L, "windows": windows,
        "device_stream_ms_per_window": round(1e3 * t_stream / windows, 4),
        "device_batched_ms_per_frame": round(1e3 * t_batched / n, 4),
        "cpu_restatement_ms_per_window": round(1e3 * t_cpu, 2),
        "cpu_windows_timed": nc - L + 1,
        "worst_rel_diff_vs_restatement": worst,
        "temporal_consistency": float(res["Temporal Consistency"]),
    }))


if __name__ == "__main__":
    main()
