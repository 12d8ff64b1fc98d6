"""Phase timeline of the group-action tile kernels from in-kernel timestamps (A/B build,
LV_STAMPS=1: lane 0 of every wave writes the 100 MHz real-time counter at each phase
boundary; action_common.h phase_stamp).  For the last of R back-to-back launches of the
fused forward and of lv_group_action_bwd at one shape, prints per degree segment (wave
index) the median / 90th-percentile phase durations and, over the whole grid, when blocks
start / finish relative to the earliest block start (10 ns ticks shown as us); for the
forward also when the output drain starts and ends chip-wide against the launch time, the
per-class chain ends under LV_TILE_NCLASS, each wave's SIMD and the blocks per CU.

  LIEVAE_HIP_LIB=lie-vae_amd/lie_vae/liblievae_hip_ab.so LV_STAMPS=1 \
      python tools/timeline.py [B] [L] [f32|bf16] [fwd|bwd|both]
"""
import ctypes
import os
import sys

import numpy as np
import torch

sys.path[:0] = [os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lie-vae_amd")]
from lie_vae import _lib  # noqa: E402

KB = 16384  # kStampBlocks
TICK_US = 0.01  # s_memrealtime: 100 MHz


DEG_BASE, DEG_BLOCKS = KB * 16 * 8 + 2 * 4096, 2048


def stamps(lib, with_deg=False):
    n = DEG_BASE + DEG_BLOCKS * 16 * 24
    buf = np.zeros(n, dtype=np.uint64)
    fn = lib.lv_ab_stamps_copy
    fn.restype, fn.argtypes = ctypes.c_size_t, [ctypes.c_void_p, ctypes.c_size_t]
    got = fn(buf.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(buf.nbytes))
    assert got == buf.nbytes, "LV_STAMPS=1 and the A/B library (LIEVAE_HIP_LIB) are required"
    out = (buf[: KB * 16 * 8].reshape(KB, 16, 8).astype(np.int64),
           buf[KB * 16 * 8: DEG_BASE].reshape(4096, 2).astype(np.int64))
    if with_deg:
        out = out + (buf[DEG_BASE:].reshape(DEG_BLOCKS, 16, 24).astype(np.int64),)
    return out


def degree_costs(name, st, deg, nblk, masks):
    """Median time per degree (us): stamp at the end of degree l minus the end of the
    wave's previous degree (phase-1 stamp for its first), in the order the wave ran them
    (the backward walks its degrees largest first, the forward smallest first)."""
    nb = min(nblk, DEG_BLOCKS)
    res = {}
    for w, m in enumerate(masks):
        prev = st[:nb, w, 1]
        ls = [b for b in range(24) if (m >> b) & 1]
        ls.sort(key=lambda b: float(np.median(deg[:nb, w, b])))  # execution order
        for l in ls:
            d = (deg[:nb, w, l] - prev) * TICK_US
            res[l] = (w, float(np.median(d)))
            prev = deg[:nb, w, l]
    print(f"  {name} per-degree median us: " + " ".join(f"l{l}(w{w}):{t:.3f}" for l, (w, t) in sorted(res.items())))
    return res


def drain(st, s, t0, nblk, launch_us):
    """Forward tile kernel, chip-wide: when the output drain starts and ends (a block's flush
    starts when its last wave leaves the second barrier, stamp 3, and ends at its last stamp 4)
    against the launch time, the streamed-store time of the bytes, and -- with block priority
    classes (slot [block][15][0] = class + 1) -- per class when the chains end."""
    us = lambda x: x * TICK_US  # noqa: E731
    chain_end = us(s[:, :, 2].max(axis=1) - t0)
    fl0 = us(s[:, :, 3].max(axis=1) - t0)
    fl1 = us(s[:, :, 4].max(axis=1) - t0)
    print(f"  flush start  min/p10/50/90/max {fl0.min():6.2f} {np.percentile(fl0, 10):6.2f} {np.median(fl0):6.2f} "
          f"{np.percentile(fl0, 90):6.2f} {fl0.max():6.2f} us")
    print(f"  flush end    p10/50/90/max     {np.percentile(fl1, 10):6.2f} {np.median(fl1):6.2f} "
          f"{np.percentile(fl1, 90):6.2f} {fl1.max():6.2f} us")
    if launch_us:
        print(f"  launch {launch_us:6.2f} us (events over the back-to-back launches, stamps on): "
              f"last flush end -> launch end {launch_us - fl1.max():5.2f} us; "
              f"first flush -> launch end {launch_us - fl0.min():5.2f} us")
    cls = st[:nblk, 15, 0] - 1
    if (cls >= 0).any():
        for k in sorted(set(cls[cls >= 0].tolist())):
            m = cls == k
            print(f"  class {k} (s_setprio rank, 0 first): {int(m.sum()):4d} blocks  start {np.median(us(s[m, 0, 0] - t0)):5.2f}  "
                  f"chain end p50/p90 {np.median(chain_end[m]):5.2f} {np.percentile(chain_end[m], 90):5.2f}  "
                  f"flush start p50 {np.median(fl0[m]):5.2f}  flush end p50/max {np.median(fl1[m]):5.2f} {fl1[m].max():5.2f} us")
    else:
        print("  block classes off")
    nwave = s.shape[1]
    hw = st[:nblk, 8:8 + nwave, 1]
    if (hw >> 32).all():  # each wave's hardware-ID register (class_stamp)
        simd = (hw >> 4) & 3
        print("  SIMD of wave k (blocks on SIMD 0/1/2/3): " +
              "  ".join(f"w{w} " + "/".join(str(int((simd[:, w] == q).sum())) for q in range(4)) for w in range(nwave)))
        # blocks b and b + 8 share an XCD; within it SE / SH / CU id name the CU
        cu = (np.arange(nblk) % 8) * 4096 + ((hw[:, 0] >> 8) & 0xff)
        _, inv, cnt = np.unique(cu, return_inverse=True, return_counts=True)
        print("  CUs holding 1/2/3/4+ blocks: " + " ".join(str(int((cnt == k).sum())) for k in (1, 2, 3)) +
              f" {int((cnt >= 4).sum())}")
        for k in (1, 2, 3):
            m = cnt[inv] == k
            if m.any():
                print(f"    blocks on a CU with {k}: chain end p50/max {np.median(chain_end[m]):5.2f} {chain_end[m].max():5.2f}  "
                      f"flush end p50/max {np.median(fl1[m]):5.2f} {fl1[m].max():5.2f} us")
        # the first-arrived block of each CU wins VALU issue by age: its chain is the path to
        # the CU's first flush
        first = np.zeros(nblk, dtype=bool)
        for k in range(len(cnt)):
            idx = np.nonzero(inv == k)[0]
            first[idx[np.argmin(s[idx, 0, 0])]] = True
        ch = us(s[first][:, :, 2] - s[first][:, :, 1])
        print(f"  first-arrived block of each CU ({int(first.sum())}): prologue barrier -> chain end per wave, p50/p90: " +
              "  ".join(f"w{w} {np.median(ch[:, w]):4.2f}/{np.percentile(ch[:, w], 90):4.2f}" for w in range(nwave)))
        b2f = us(s[first][:, :, 3].max(axis=1) - s[first][:, :, 1].max(axis=1))
        print(f"    its barrier -> flush start p10/50/90 {np.percentile(b2f, 10):5.2f} {np.median(b2f):5.2f} "
              f"{np.percentile(b2f, 90):5.2f} us; its flush start from grid start p10/50/90 "
              f"{np.percentile(fl0[first], 10):5.2f} {np.median(fl0[first]):5.2f} {np.percentile(fl0[first], 90):5.2f} us")


def report(name, st, nblk, nwave, phases, red=None, nred=0, extra=None, launch_us=None):
    s = st[:nblk, :nwave, :]
    t0 = s[:, :, 0][s[:, :, 0] > 0].min()
    print(f"== {name}: {nblk} blocks x {nwave} waves")
    us = lambda x: x * TICK_US  # noqa: E731
    for w in range(nwave):
        cols = []
        for k in range(1, len(phases)):
            d = us(s[:, w, k] - s[:, w, k - 1])
            cols.append(f"{phases[k]} {np.median(d):6.2f}/{np.percentile(d, 90):6.2f}")
        print(f"  wave {w}: " + "  ".join(cols))
    start = us(s[:, 0, 0] - t0)
    end = us(s[:, :, len(phases) - 1].max(axis=1) - t0)
    print(f"  block start  p10/50/90/max {np.percentile(start, 10):6.2f} {np.median(start):6.2f} "
          f"{np.percentile(start, 90):6.2f} {start.max():6.2f} us")
    print(f"  block finish p10/50/90/max {np.percentile(end, 10):6.2f} {np.median(end):6.2f} "
          f"{np.percentile(end, 90):6.2f} {end.max():6.2f} us")
    if extra:
        for k, nm in extra:
            d = us(s[:, :, k] - s[:, :, 0])
            ok = s[:, :, k] > 0
            print(f"  {nm}: median " + " ".join(f"{np.median(d[:, w][ok[:, w]]):5.2f}" if ok[:, w].any() else "  -  "
                                            for w in range(nwave)) + " us after wave start")
    first = [us(np.median(s[:, w, 1] - t0)) for w in range(nwave)]
    print("  median time of phase 1 end per wave (from grid start): " + " ".join(f"{x:5.2f}" for x in first))
    if phases[-1] == "flush":
        drain(st, s, t0, nblk, launch_us)
    if red is not None and nred:
        r = red[:nred]
        print(f"  reduce kernel: start p50 {us(np.median(r[:, 0] - t0)):6.2f}  end max {us(r[:, 1].max() - t0):6.2f} us"
              f"  (tile grid finished at {end.max():6.2f})")


def main():
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
    L = int(sys.argv[2]) if len(sys.argv) > 2 else 10
    dt = sys.argv[3] if len(sys.argv) > 3 else "f32"
    which = sys.argv[4] if len(sys.argv) > 4 else "both"
    C, R = 10, 30
    dev = torch.device("cuda:0")
    lib = _lib.load()
    P = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    g = torch.Generator().manual_seed(0)
    v = torch.randn(B, 3, generator=g).to(dev)
    M = (L + 1) ** 2
    F = torch.randn(M, C, generator=g).to(dev)
    odt = torch.bfloat16 if dt == "bf16" else torch.float32
    out = torch.empty(B, M, C, device=dev, dtype=odt)
    ang = torch.empty(B, 3, device=dev)
    plan = (ctypes.c_int64 * 40)()
    code = _lib.LV_DTYPE_BF16 if dt == "bf16" else _lib.LV_DTYPE_F32
    assert lib.lv_action_fwd_plan(1, 0, code, B, L, C, plan) == 0
    if which in ("fwd", "both"):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        for r in range(2 * R):
            if r == R:  # the first R warm up; the second R are timed
                ev[0].record()
            assert lib.lv_fused_exp_action_fwd(None, P(v), P(F), 0, P(out), code, P(ang), B, L, C, 0, None) == 0
        ev[1].record()
        torch.cuda.synchronize()
        launch_us = ev[0].elapsed_time(ev[1]) * 1e3 / R
        st, _, deg = stamps(lib, True)
        print(f"plan: blocks {plan[1]} segments {plan[2]} lds {plan[4]} degree sets "
              f"{[bin(plan[24 + k]) for k in range(plan[2])]}")
        report(f"fused forward B={B} l={L} {dt}", st, min(plan[1], KB), plan[2],
               ["start", "prologue", "chain", "barrier", "flush"],
               extra=[(5, "loads landed"), (6, "exp->ZYZ done (wave 0)"), (7, "multiples done (wave 0)")],
               launch_us=launch_us)
        degree_costs("forward", st, deg, plan[1], [plan[24 + k] for k in range(plan[2])])
    if which in ("bwd", "both"):
        lib.lv_fused_exp_action_fwd(None, P(v), P(F), 0, P(out), _lib.LV_DTYPE_F32, P(ang), B, L, C, 0, None)
        gout = torch.randn(B, M, C, generator=g).to(dev)
        gang, gF = torch.empty(B, 3, device=dev), torch.empty(M, C, device=dev)
        wsb = lib.lv_group_action_bwd_workspace(B, L, C, 1)
        ws = torch.zeros(max(wsb, 1), device=dev, dtype=torch.uint8)
        bp = (ctypes.c_int64 * 40)()
        assert lib.lv_group_action_bwd_plan(B, L, C, 1, bp) == 0
        for _ in range(R):
            assert lib.lv_group_action_bwd(P(ang), P(F), 0, P(gout), P(gang), P(gF), B, L, C, 0, P(ws), wsb,
                                           None) == 0
        st, red, deg = stamps(lib, True)
        print(f"bwd plan: blocks {bp[1]} segments {bp[2]} lds {bp[4]} degree sets {[bin(bp[24 + k]) for k in range(bp[2])]}")
        report(f"group-action backward B={B} l={L}", st, min(bp[1], KB), bp[2],
               ["start", "load+prologue", "chain", "slab", "angle-sync", "end"], red, (M * C + 15) // 16)
        degree_costs("backward", st, deg, bp[1], [bp[24 + k] for k in range(bp[2])])


if __name__ == "__main__":
    main()
