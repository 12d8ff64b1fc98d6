"""Times lie_vae.s2.synthesis / analysis on a 64 x 128 latitude-longitude grid against the
plain-torch equivalent, a matmul with a basis matrix precomputed on the device (DESIGN.md
§4.11).  Device events around runs of `calls` back-to-back calls, the two arms alternating,
`reps` runs each after a warm-up; prints the median and the spread per call.

    python tools/s2_bench.py [--out profiles/s2_transform_times.txt]
"""
import argparse
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "lie-vae_amd"))

from lie_vae import s2  # noqa: E402

SIZES = ((64, 6, 10), (1, 20, 64))  # (B, L, C)
HEIGHT, WIDTH = 64, 128


def timed(fn, calls):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(calls):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e3 / calls  # us per call


def compare(name, ours, theirs, calls, reps, warmup, lines):
    for _ in range(warmup):
        ours()
        theirs()
    torch.cuda.synchronize()
    a, b = [], []
    for _ in range(reps):
        a.append(timed(ours, calls))
        b.append(timed(theirs, calls))
    fmt = lambda t: f"median {statistics.median(t):8.2f} us  (min {min(t):8.2f}, max {max(t):8.2f})"
    lines.append(f"{name:<34} kernels {fmt(a)}")
    lines.append(f"{'':<34} matmul  {fmt(b)}   ratio kernels/matmul "
                 f"{statistics.median(a) / statistics.median(b):.2f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("s2_bench needs a HIP device: timings are taken on the GPU only")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    x = s2.equirect_points(HEIGHT, WIDTH, dev)
    P = x.shape[0]
    w = torch.rand(P, device=dev) + 0.5
    lines = [f"# {torch.cuda.get_device_name(0)}; P = {HEIGHT} x {WIDTH} = {P} points; "
             f"{args.reps} runs of {args.calls} calls per arm, alternating, after {args.warmup} "
             f"warm-up calls; device events"]
    for B, L, C in SIZES:
        M = (L + 1) ** 2
        F = torch.randn(B, M, C, device=dev)
        V = torch.randn(B, P, C, device=dev)
        Y = s2.real_spherical_harmonics(x, L)           # (P, M), precomputed for the torch arm
        YwT = (Y * w[:, None]).t().contiguous()         # (M, P)
        syn, ana = s2.synthesis(F, x), s2.analysis(V, x, w, L)
        dsyn = ((syn - torch.matmul(Y, F)).abs().max() / syn.abs().max()).item()
        dana = ((ana - torch.matmul(YwT, V)).abs().max() / ana.abs().max()).item()
        flop = 2.0 * B * P * M * C
        lines.append(f"B={B} L={L} C={C}: {flop / 1e6:.0f} MFLOP per call; kernels vs matmul, max "
                     f"abs difference / max abs: synthesis {dsyn:.1e}, analysis {dana:.1e}")
        compare(f"synthesis B={B} L={L} C={C}", lambda: s2.synthesis(F, x),
                lambda: torch.matmul(Y, F), args.calls, args.reps, args.warmup, lines)
        compare(f"analysis  B={B} L={L} C={C}", lambda: s2.analysis(V, x, w, L),
                lambda: torch.matmul(YwT, V), args.calls, args.reps, args.warmup, lines)
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
