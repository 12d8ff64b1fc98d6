"""Case table of tests/test_gpu_action_matrix.py: which (l_max, C, n) the group-action
kernels are run at, which entry points ("runs") each case takes, and which dispatch branch
of the planner (action.hip plan_fwd / plan_bwd) a run reaches.  Plain module, no GPU call:
the GPU tests execute the table, the CPU guard in tests/test_plan.py classifies it with the
host-only plan queries, so a planner change that moves the cases off a branch fails there
instead of silently emptying the GPU tests."""
import collections
import math

from lie_vae import _lib

F32, BF16 = _lib.LV_DTYPE_F32, _lib.LV_DTYPE_BF16
CUS = _lib.load().lv_compute_units()   # the planner's CU count (256 on MI355X / no device)
FAST_C = 10                            # action_common.h kTileFastC: the compile-time-C kernels
F_GLOBAL_MIN_L = 13                    # kTileFGlobalMinL / kTrigLdsMinL
BWD_MAX_BLOCKS = 4096                  # action.hip kBwdMaxBlocks
BWD_MAX_BLOCKS_FALLBACK = 1024         # action.hip kBwdMaxBlocksFallback
PERSIST_BLOCKS = 3 * CUS               # action_bwd_persist.h kBwdPersistBlocksPerCU

# section: which test runs the case; shared: spectrum (M, C) for the whole batch (else
# (n, M, C)) in the runs that do not say otherwise
Case = collections.namedtuple("Case", "section L C n shared")
# path: "angles" (ops.group_action), "fused_mu" / "fused_nomu" (ops.fused_exp_action with /
# without a mean rotation); fwd / bwd: whether the run's output / gradients are checked
Run = collections.namedtuple("Run", "path shared bf16 transpose fwd bwd")


def _fused(L):
    return "fused_mu" if L % 2 else "fused_nomu"


def sweep_runs(L):
    """Sections 1 and 3: angle path with a shared and a per-sample spectrum, the fused path,
    forward and backward; bf16 forward from angles and fused.  Plain for even l,
    transposed for odd l; a mean rotation for odd l, none for even l."""
    t = bool(L % 2)
    return [Run("angles", True, False, t, True, True),
            Run("angles", False, False, t, True, True),
            Run(_fused(L), True, False, t, True, True),
            Run("angles", True, True, t, True, False),
            Run(_fused(L), True, True, t, True, False)]


# 1. every degree at the product's channel count: six full 6-sample groups and a ragged one
DEGREE_SWEEP = [Case("degree", L, 10, 37, True) for L in range(21)]

# 2. the persistent backward (plan mode 3) at every degree it serves, just past its
#    threshold of CUs + 1 groups; l = 0, 1, 2 at the same size stay on the one-group kernel
PERSIST_N = 6 * (CUS + 1) + 5
PERSIST = [Case("persist", L, 10, PERSIST_N, True) for L in range(10)]

# 3. channel classes of the run-time-C kernels: 64, 32, 21, 9, 5, 4, 3, 2 (twice), 1 and 1
#    samples per group; two full groups and a ragged one
CHANNEL_CS = (1, 2, 3, 7, 11, 16, 21, 32, 33, 64)
CHANNEL_LS = (1, 5, 12, 13, 16)
CHANNELS = [Case("channels", L, C, max(5, 2 * (64 // C) + 1), True)
            for C in CHANNEL_CS for L in CHANNEL_LS]
# l = 20 fp32: the forward is the grid-stride kernel, the C = 11 backward one sample per block
L20_FUSED = [Case("l20", 20, 10, 37, True), Case("l20", 20, 11, 37, True)]
# one channel at the ends of the degree range: at l = 0 (C = 1, 2) and l = 1 (C = 1, above) a
# block has too few waves for 64 // C samples, so the forward takes the grid-stride kernel and
# the backward a reduced group; at l = 19, 20 the bf16 forward is grid-stride too
EDGES = [Case("edges", 0, 1, 129, True), Case("edges", 0, 2, 65, True),
         Case("edges", 19, 1, 129, True), Case("edges", 20, 1, 129, True)]

# 4. grids whose blocks loop over several sample groups
LOOPED = [Case("looped", 2, 10, 6 * 4096 + 7, True),     # compile-time C, below the persistent range
          Case("looped", 11, 10, 6 * 4096 + 7, True),    # the same kernel above it
          Case("looped", 20, 10, 3 * 4096 + 7, True),    # reduced group of 3
          Case("looped", 5, 33, 4101, True),             # run-time C, one sample per block
          Case("looped", 12, 64, 1030, True),            # mode 2 fallback, 1,024 blocks
          Case("looped", 3, 64, 4100, False),            # per-sample spectrum
          Case("looped", 7, 10, 6 * PERSIST_BLOCKS + 7, True),  # persistent kernel walking groups
          Case("looped", 1, 1, 42 * 4096 + 1, True),     # reduced group (42 of 64), run-time C
          Case("looped", 1, 1, 42 * 4096 + 1, False)]    # the same, per-sample spectrum

# 5. hand-made boundary angles
def boundary_angles():
    """ZYZ triples on the edges of the reference extraction's ranges (alpha, gamma in
    [-pi, pi], beta in [0, pi]): every combination of alpha, gamma in {-pi, -pi/2, 0, pi/2,
    pi} and beta in {0, pi/2, pi}, then beta within 1e-6 of 0 and of pi at two generic
    (alpha, gamma) pairs."""
    pi = math.pi
    edge = (-pi, -pi / 2, 0.0, pi / 2, pi)
    out = [(a, b, c) for a in edge for b in (0.0, pi / 2, pi) for c in edge]
    for a, c in ((0.3, -1.1), (-2.5, 3.0)):
        out += [(a, b, c) for b in (1e-7, 5e-7, 1e-6, pi - 1e-6, pi - 5e-7, pi - 1e-7)]
    return out


BOUNDARY_N = len(boundary_angles())
BOUNDARY = [Case("boundary", L, 10, BOUNDARY_N, True) for L in (10, 20)]

ALL_CASES = DEGREE_SWEEP + PERSIST + CHANNELS + L20_FUSED + EDGES + LOOPED + BOUNDARY


def runs(case):
    """The runs the GPU test of case.section executes."""
    L = case.L
    if case.section in ("degree", "channels", "edges"):
        return sweep_runs(L)
    if case.section == "persist":  # transposed for even l; backward only
        t = L % 2 == 0
        return [Run("angles", True, False, t, False, True), Run(_fused(L), True, False, t, False, True)]
    if case.section == "l20":
        return [Run("fused_mu", True, False, False, True, True)]
    if case.section == "looped":
        return [Run("angles", case.shared, False, False, False, True)]
    if case.section == "boundary":
        return [Run("angles", True, False, False, True, True)]
    raise ValueError(case.section)


def seed(case):
    """One seed per case from (L, C, n)."""
    return (case.L * 1_000_003 + case.C * 10_007 + case.n) % (2 ** 31)


def fwd_plan(case, run):
    M = (case.L + 1) ** 2
    return _lib.plan("fwd", int(run.path != "angles"), 0 if run.shared else M * case.C,
                     BF16 if run.bf16 else F32, case.n, case.L, case.C)


def bwd_plan(case, run):
    return _lib.plan("bwd", case.n, case.L, case.C, int(run.shared))


def bwd_groups(case, plan):
    return -(-case.n // plan["samples_per_group"])


def fwd_branch(case, run):
    """(tile | grid-stride, C = 10 | run-time C, spectrum and trig tables below | from l = 13,
    fp32 | bf16 output, input path).  The C class is the kernel's: the grid-stride kernel has
    no compile-time-C twin (action_fwd.h FwdLauncher)."""
    p = fwd_plan(case, run)
    return ("tile" if p["tile"] else "grid",
            "c10" if case.C == FAST_C and p["tile"] else "crt",
            "l<13" if case.L < F_GLOBAL_MIN_L else "l>=13",
            "bf16" if run.bf16 else "f32",
            run.path)


def bwd_branch(case, run):
    """(plan mode 0 per-sample / 1 LDS spectrum / 2 global-spectrum fallback / 3 persistent,
    C = 10 | run-time C, one group per block | looped, full | reduced samples per group).
    The C class is the kernel's: compile-time C = 10 exists for modes 1 and 3 only
    (action_bwd.h BwdLauncher)."""
    p = bwd_plan(case, run)
    return (p["tile"],
            "c10" if case.C == FAST_C and p["tile"] in (1, 3) else "crt",
            "looped" if p["blocks"] < bwd_groups(case, p) else "one",
            "reduced" if p["samples_per_group"] < 64 // case.C else "full")


def table_branches():
    """Branch -> cases of the table that reach it, forward and backward; and the degrees
    with a checked forward / backward run."""
    fwd, bwd = collections.defaultdict(list), collections.defaultdict(list)
    for case in ALL_CASES:
        for run in runs(case):
            if run.fwd:
                fwd[fwd_branch(case, run)].append(case)
            if run.bwd:
                bwd[bwd_branch(case, run)].append(case)
    return fwd, bwd


def reachable_branches():
    """Every branch the planner reaches anywhere in its domain: all l and C, batch sizes on
    both sides of each grid cap and of the persistent threshold, every entry point."""
    ns = (5, 37, PERSIST_N, BWD_MAX_BLOCKS_FALLBACK + 6, BWD_MAX_BLOCKS + 5,
          6 * BWD_MAX_BLOCKS + 7, 64 * BWD_MAX_BLOCKS + 1)
    fwd, bwd = set(), set()
    for L in range(21):
        for C in range(1, 65):
            for n in ns:
                for shared in (True, False):
                    case = Case("any", L, C, n, shared)
                    bwd.add(bwd_branch(case, Run("angles", shared, False, False, False, True)))
                    fwd.add(fwd_branch(case, Run("angles", shared, False, False, True, False)))
                    if shared:  # bf16 output and the fused path take a shared spectrum only
                        fwd.add(fwd_branch(case, Run("angles", True, True, False, True, False)))
                        for path in ("fused_mu", "fused_nomu"):
                            for bf16 in (False, True):
                                fwd.add(fwd_branch(case, Run(path, True, bf16, False, True, False)))
    return fwd, bwd
