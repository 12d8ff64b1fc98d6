"""LDS waits on the chain of a forward tile kernel, from its ISA listing.

Between the first and the second s_barrier of one kernel (the chain: prologue barrier ->
flush barrier) every `s_waitcnt lgkmcnt(N)` guards the LDS reads issued before it.  For each
wait this prints how many ds_read instructions are outstanding when it is reached, how many
of them it lets stay in flight (N), and how many VALU instructions were issued between the
last of the reads it waits for and the wait itself: the cover.  A wait with a cover of ~100
VALU (a J product) is hidden; one with a handful is an exposed LDS round trip on the wave's
serial path.

  hipcc <the Makefile's CXXFLAGS and ACTION_FLAGS> -DLV_INST_L=10 --cuda-device-only -S \
      lie-vae_amd/csrc/action_inst.hip -o l10.s
  python tools/chain_waits.py l10.s 'action_fwd_tile_kernelILi10ELi10ELb1EfLb0E' [--list]

Also prints the kernel's .vgpr_count / .sgpr_count / scratch size from its metadata.
"""
import re
import sys

EXPOSED_BELOW = 24  # VALU instructions: less than one LDS round trip (~64-128 cycles) of issue


def kernel_body(lines, key):
    start = next(i for i, s in enumerate(lines) if re.match(r"^_Z\w*" + re.escape(key) + r"\w*:", s))
    end = next(i for i in range(start, len(lines)) if lines[i].strip().startswith("s_endpgm"))
    return lines[start:end + 1]


def metadata(lines, key):
    out = {}
    for i, s in enumerate(lines):
        if s.strip().startswith(".name:") and key in s and not s.strip().endswith(".kd"):
            j = i
            while j > 0 and not lines[j].strip().startswith("- .agpr_count"):
                j -= 1
            for t in lines[j:j + 400]:
                m = re.match(r"\s*-?\s*\.(vgpr_count|sgpr_count|private_segment_fixed_size|vgpr_spill_count):\s*(\d+)", t)
                if m:
                    out[m.group(1)] = int(m.group(2))
                if t.strip().startswith(".wavefront_size") and out:
                    break
            break
    return out


def analyse(body):
    ins = [s.split(";")[0].strip() for s in body]
    ins = [s for s in ins if s and not s.endswith(":") and not s.startswith(".")]
    bars = [i for i, s in enumerate(ins) if s.startswith("s_barrier")]
    assert len(bars) >= 2, "two s_barrier expected"
    chain = ins[bars[0] + 1:bars[1]]
    waits = []
    pending = []  # VALU count at issue of each outstanding LDS op ("r" read / "w" write)
    valu = 0
    for s in chain:
        op = s.split()[0]
        if op.startswith("ds_read"):
            pending.append(("r", valu))
        elif op.startswith("ds_write"):
            pending.append(("w", valu))
        elif op.startswith("v_"):
            valu += 1
        elif op.startswith("s_cbranch") or op.startswith("s_branch"):
            pending = []  # a degree's block ends: what follows is another path
        elif op == "s_waitcnt":
            m = re.search(r"lgkmcnt\((\d+)\)", s)
            if not m:
                continue
            keep = int(m.group(1))
            done = pending[:len(pending) - keep] if keep else pending
            reads = [v for k, v in done if k == "r"]
            if reads:
                waits.append((len(reads), keep, valu - reads[-1]))
            pending = pending[len(pending) - keep:] if keep else []
    nvalu = sum(1 for s in chain if s.startswith("v_"))
    return chain, waits, nvalu


def main():
    path, key = sys.argv[1], sys.argv[2]
    lines = open(path).read().splitlines()
    chain, waits, nvalu = analyse(kernel_body(lines, key))
    exposed = [w for w in waits if w[2] < EXPOSED_BELOW]
    print(f"{key}: chain {len(chain)} instructions, {nvalu} VALU, "
          f"{sum(1 for s in chain if s.startswith('ds_read'))} ds_read, "
          f"{sum(1 for s in chain if s.startswith('ds_write'))} ds_write")
    print(f"  s_waitcnt lgkmcnt that guard LDS reads: {len(waits)}; cover < {EXPOSED_BELOW} VALU (exposed): {len(exposed)}")
    cov = sorted(w[2] for w in waits)
    if cov:
        print(f"  cover (VALU between the last awaited read and the wait): min {cov[0]} median {cov[len(cov) // 2]} max {cov[-1]}")
    print(f"  metadata: {metadata(lines, key)}")
    if "--list" in sys.argv:
        for n, keep, c in waits:
            print(f"    reads awaited {n:3d}  left in flight {keep:2d}  cover {c:4d} VALU")


if __name__ == "__main__":
    main()
