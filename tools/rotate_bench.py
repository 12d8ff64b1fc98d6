#!/usr/bin/env python3
"""Same-box A/B of the image rotation (csrc/image.hip): the staged (LDS) path, the direct
path and the torch composition F.affine_grid + F.grid_sample the reference runs, plus the
equivariance loss kernel against bmm / sub / pow / sum.

Each variant is captured as K back-to-back calls in one hipGraph and replayed; the rounds
alternate the variants, and the figure is the median round's time per call (device events
around each replay).  The roofline is the N·C·H·W·8 bytes a rotation must move (each plane
read once and written once) over the HBM peak.

  python tools/rotate_bench.py [--out FILE]
"""
import argparse
import json
import math
import os
import statistics
import sys

import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "lie-vae_amd"))

HBM_PEAK = 8.0e12  # bytes/s, HBM3E spec (MI355X); ~6.3e12 is what a float4 copy reaches
SHAPES = [(512, 1, 64, 64), (4096, 1, 64, 64), (512, 3, 64, 64), (4096, 3, 64, 64)]


def graph_of(fn, calls, dev):
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
    torch.cuda.current_stream(dev).wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(calls):
            fn()
    return g


def time_variants(variants, calls, rounds, dev):
    """variants: name -> callable.  Returns name -> (median, min, max) microseconds per call."""
    graphs = {k: graph_of(f, calls, dev) for k, f in variants.items()}
    for g in graphs.values():  # warm replays
        g.replay()
    torch.cuda.synchronize(dev)
    times = {k: [] for k in variants}
    for _ in range(rounds):
        for k, g in graphs.items():  # alternate the variants inside every round
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            g.replay()
            b.record()
            b.synchronize()
            times[k].append(a.elapsed_time(b) * 1e3 / calls)
    return {k: (statistics.median(v), min(v), max(v)) for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50, help="calls per captured graph")
    ap.add_argument("--rounds", type=int, default=21)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    import lie_vae._ops as ops
    from lie_vae import _lib
    dev = torch.device("cuda:0")
    lines = []
    for shape in SHAPES:
        N, C, H, W = shape
        g = torch.Generator().manual_seed(N + C)
        img = torch.rand(*shape, generator=g).to(dev)
        theta = torch.rand(N, generator=g) * 2 * math.pi
        cs = torch.stack((torch.cos(theta), torch.sin(theta)), 1).to(dev)
        zero = torch.zeros(N, device=dev)
        affine = torch.stack([cs[:, 0], -cs[:, 1], zero, cs[:, 1], cs[:, 0], zero], 1).view(-1, 2, 3)

        def torch_rot():
            return F.grid_sample(img, F.affine_grid(affine, list(shape), align_corners=False),
                                 align_corners=False)

        variants = {"staged": lambda: ops.rotate_images(img, cs),
                    "direct": lambda: ops.rotate_images(img, cs, flags=_lib.LV_ROTATE_DIRECT),
                    "torch affine_grid+grid_sample": torch_rot}
        # faster and different is not faster: same inputs, same outputs to rounding
        ref = torch_rot()
        for k in ("staged", "direct"):
            y = variants[k]()
            err = float((y - ref).norm() / ref.norm())
            assert err < 1e-5, (k, err)
        assert torch.equal(variants["staged"](), variants["direct"]())
        res = time_variants(variants, args.calls, args.rounds, dev)
        floor_us = N * C * H * W * 8 / HBM_PEAK * 1e6
        lines.append({"op": "rotate", "shape": list(shape), "bytes_min": N * C * H * W * 8,
                      "roofline_us_at_8TBps": floor_us,
                      "us_per_call": {k: {"median": v[0], "min": v[1], "max": v[2],
                                          "roofline_frac": floor_us / v[0]}
                                      for k, v in res.items()},
                      "calls_per_graph": args.calls, "rounds": args.rounds})
        print(json.dumps(lines[-1]), flush=True)
    for N in (512, 4096):
        g = torch.Generator().manual_seed(N)
        theta = torch.rand(N, generator=g) * 2 * math.pi
        cs = torch.stack((torch.cos(theta), torch.sin(theta)), 1).to(dev)
        enc = torch.randn(N, 3, 3, generator=g).to(dev)
        enc_rot = torch.randn(N, 3, 3, generator=g).to(dev)
        gmat = torch.zeros(N, 3, 3, device=dev)
        gmat[:, 0, 0] = 1
        gmat[:, 1, 1] = gmat[:, 2, 2] = cs[:, 0]
        gmat[:, 2, 1] = cs[:, 1]
        gmat[:, 1, 2] = -cs[:, 1]

        def torch_diff():
            return (gmat.bmm(enc) - enc_rot).pow(2).view(N, -1).sum(-1)

        variants = {"lv_equivariance_diff_fwd": lambda: ops.equivariance_diff(cs, enc, enc_rot),
                    "torch bmm+sub+pow+sum": torch_diff}
        err = float((variants["lv_equivariance_diff_fwd"]() - torch_diff()).norm() / torch_diff().norm())
        assert err < 1e-5, err
        res = time_variants(variants, args.calls, args.rounds, dev)
        lines.append({"op": "equivariance_diff_fwd", "n": N,
                      "us_per_call": {k: {"median": v[0], "min": v[1], "max": v[2]}
                                      for k, v in res.items()},
                      "calls_per_graph": args.calls, "rounds": args.rounds})
        print(json.dumps(lines[-1]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
