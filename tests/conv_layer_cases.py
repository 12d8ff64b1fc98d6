"""Case table of tests/test_gpu_conv_layers.py: the shapes at which the conv-layer kernels
(csrc/deconv.hip, csrc/bn.hip) are run, each with the launch-code branch it is there for.
Plain module, no GPU call: the GPU tests execute the table, tests/test_abi.py checks the
host-side size queries against the closed forms below (bn_geom is a transcription of
bn.hip's), so a change of a tile size or a block cap that moves a case off its branch fails
there instead of silently emptying the GPU tests."""
import collections
import math

from lie_vae import _lib

CUS = _lib.load().lv_compute_units()   # 256 on MI355X (and with no device)
RELU_OUT, MASK_GX = _lib.LV_DECONV_RELU_OUT, _lib.LV_DECONV_MASK_GX

# deconv.hip constants the cases are built around
MFMA_BM = 128            # pixel rows per block tile of the default bf16 / fp32 variants
MFMA_MAX_COUT = 208      # kBN
BW_TA, BW_TB = 2, 32     # kBwTA x kBwTB input pixels per tile of the small-Cout backward
WG_MAX_BLOCKS = 512      # kWgMaxBlocks
CS_MAX_BLOCKS = 1024     # kCsMaxBlocks
# bn.hip constants
BN_THREADS, BN_MAX_BLOCKS, BN_APPLY_MAX_BLOCKS = 256, 512, 2048

# ------------------------------------------------------------------ A. bf16 MFMA forward
# y (N, 2H, 2W, Cout) = conv_transpose2d(x (N, H, W, Cin), w (Cin, Cout, 4, 4), 2, 1) + bias.
# M = N·H·W rows in tiles of MFMA_BM; the grid is padded to whole groups of 8 tiles x 4
# phases, the padding blocks return at once.  K = 4·Cin in steps of 32.
Mfma = collections.namedtuple("Mfma", "N H W Cin Cout bias flags")
MFMA_BF16 = [
    # M = 1: a 1x1 image (every tap but one outside), 127 idle rows, 7 of 8 tiles returning;
    # Cin = 8: one K step (prologue only); Cout = 8: one live channel tile
    Mfma(1, 1, 1, 8, 8, True, 0),
    # M = 127: one ragged tile; Cin = 16: two K steps; Cout = 12: Cout % 8 == 4 (8-byte stores)
    Mfma(127, 1, 1, 16, 12, True, 0),
    # M = 128: exactly one tile; Cin = 24: the tap changes inside a K step; workload Cout
    Mfma(16, 2, 4, 24, 200, True, 0),
    # M = 129: a full tile and a one-row tile; Cin = 40; Cout = 204 (% 8 == 4, last tile ragged)
    Mfma(43, 1, 3, 40, 204, True, 0),
    # 8 tiles: the XCD-grouped grid with no padding block; workload Cin, maximum Cout
    Mfma(16, 8, 8, 200, 208, True, 0),
    # 9 tiles (M = 1025): a second group of 8 with 7 returning tiles; 41x1 image
    Mfma(25, 41, 1, 16, 8, True, 0),
    # 1x9 image: every tap row partly outside; null bias
    Mfma(3, 1, 9, 8, 16, False, 0),
    # 9x1 image: every tap column partly outside; the fused ReLU
    Mfma(2, 9, 1, 24, 12, True, RELU_OUT),
    # 5x3 image (odd sizes, borders on all sides), ReLU with a null bias
    Mfma(2, 5, 3, 40, 200, False, RELU_OUT),
    # the workload's layer (200 -> 200) at its smallest image
    Mfma(4, 4, 4, 200, 200, True, 0),
]
# the encoder dgrad (_Conv4s2: gx of Conv2d(Cout, Cin, 4, 2, 1) by the same kernel, no bias):
# a Cout % 8 == 4 case and a bordered odd image
MFMA_BF16_DGRAD = [MFMA_BF16[3], MFMA_BF16[8]]

# ------------------------------------------------------------------ B. fp32 MFMA forward
# x (N, H, W, Cin) fp32, y NCHW (+ channels-last twin when Cout % 4 == 0); K steps of 16.
MFMA_F32 = [
    Mfma(1, 1, 1, 4, 1, True, 0),             # M = 1; Cin = 4: one K step; one output channel
    Mfma(127, 1, 1, 8, 5, True, RELU_OUT),    # M = 127; two K steps; odd Cout; ReLU
    Mfma(16, 2, 4, 12, 16, True, 0),          # M = 128; Cin = 12: taps change inside a step; twin
    Mfma(43, 1, 3, 4, 17, False, 0),          # M = 129; one channel past a 16-wide tile; null bias
    Mfma(16, 8, 8, 200, 208, True, 0),        # 8 tiles; workload Cin, maximum Cout; twin
    Mfma(25, 41, 1, 8, 207, True, 0),         # 9 tiles (M = 1025); Cout one short of the maximum
    Mfma(2, 5, 3, 12, 208, False, RELU_OUT),  # bordered odd image; ReLU, null bias; twin
]

# ------------------------------------------------------------------ C. small-Cout forward
# blocks of 8 x 16 output quads, K padded to 32 channels per neighbour
Small = collections.namedtuple("Small", "N H W Cin Cout bias")
SMALL_FWD = [
    Small(1, 8, 16, 8, 1, True),      # exactly one block; Cin = 8: 24 zero-padded channels
    Small(3, 9, 17, 40, 2, True),     # four blocks per image, three ragged; Cin = 40: second chunk padded
    Small(1, 1, 1, 200, 3, False),    # 1x1 image; workload channels; null bias
    Small(3, 3, 40, 248, 4, True),    # three column blocks, the last ragged; the backward's Cin limit
    Small(1, 9, 17, 200, 3, True),    # the RGB layer's channels on ragged blocks
]

# ------------------------------------------------------------------ D. small-Cout backward
# tiles of BW_TA x BW_TB input pixels; nct = ceil((Cin + 1) / 16) channel tiles (the + 1 is
# the bias "ones" column); dgrad: 4 waves own tiles w, w + 4, ...; wgrad: 8 waves own tiles
# w and w + 8 (the second accumulator set).
SmallBwd = collections.namedtuple("SmallBwd", "N H W Cin Cout flags")
SMALL_BWD = [
    SmallBwd(2, 1, 1, 8, 1, 0),       # one channel tile (three dgrad waves idle); 1x1 image
    SmallBwd(1, 2, 31, 40, 2, 0),     # three channel tiles; a full-height tile one column short
    SmallBwd(2, 5, 32, 120, 4, 0),    # eight tiles: wgrad's second accumulator set unused; W = one tile
    SmallBwd(1, 2, 33, 136, 3, 0),    # nine tiles: second set just used; a one-column tile
    SmallBwd(3, 1, 32, 248, 1, 0),    # sixteen tiles: the "ones" column in the last; half-height tile
]
# Looped grids.  H = 5, W = 33 -> 3 x 2 = 6 tiles per image, four of them ragged.  A
# 256-thread block is 4 waves and a CU has 32 wave slots, so at most 8 blocks of the dgrad
# are resident per CU (the 512-thread wgrad: at most 4, and it is capped at WG_MAX_BLOCKS);
# both launch min(ntiles, resident) blocks and block b walks tiles b, b + grid, ...  With
# ntiles > 2·8·CUs >= 2·grid every block of both kernels runs at least two tiles, on any part.
LOOP_H, LOOP_W = 5, 33
LOOP_TILES_IMG = -(-LOOP_H // BW_TA) * -(-LOOP_W // BW_TB)
LOOP_N = -(-(16 * CUS + 3) // LOOP_TILES_IMG)   # 684 at 256 CUs
assert LOOP_TILES_IMG == 6 and LOOP_N * LOOP_TILES_IMG > 2 * 8 * CUS
assert LOOP_N * LOOP_TILES_IMG > 2 * WG_MAX_BLOCKS
SMALL_BWD_LOOP = [
    SmallBwd(LOOP_N, LOOP_H, LOOP_W, 8, 3, 0),
    SmallBwd(LOOP_N, LOOP_H, LOOP_W, 40, 3, 0),
    SmallBwd(LOOP_N, LOOP_H, LOOP_W, 8, 3, MASK_GX),   # x = relu(x), gx masked by x > 0
]
# partial calls (gx only / gw only / gw without gb) and N = 0 run at this shape
SMALL_BWD_PARTIAL = SmallBwd(2, 5, 33, 40, 3, 0)

# ------------------------------------------------------------------ E. per-channel sum
# (P, C): min(CS_MAX_BLOCKS, ceil(P / 256)) blocks of ceil(P / nblk) rows, thread = 8 channels
# x every R-th row, R = 256 / (C / 8), rows 4-way unrolled
CHANNEL_SUM = [
    (1, 8),          # one row: 31 of 32 row slots idle
    (255, 200),      # one block, one row short; C = 200: R = 10, six idle threads
    (256, 2048),     # R = 1: every thread walks all rows; exactly one block
    (257, 8),        # two blocks (129 + 128 rows)
    (8191, 200),     # 32 blocks, the last one row short
    (257, 2048),
    (262145, 8),     # ceil(P / 256) = 1025 > the cap: 1024 blocks of 257 rows, the last 3 empty
]
assert -(-262145 // CS_MAX_BLOCKS) * (CS_MAX_BLOCKS - 3) >= 262145


# ------------------------------------------------------------------ F. BatchNorm + LeakyReLU
def bn_geom(P, C):
    """bn.hip bn_geom: None when unsupported, else (T, R, groups, per_blk, nblk)."""
    if C < 8 or P <= 0:
        return None
    T = C // math.gcd(C, 8)
    if T > BN_THREADS:
        return None
    pix_per_group = 8 * T // C
    if P % pix_per_group:
        return None
    R = BN_THREADS // T
    groups = P // pix_per_group
    nblk = min(BN_MAX_BLOCKS, -(-groups // (4 * R)))
    per_blk = -(-groups // nblk)
    nblk = -(-groups // per_blk)
    return T, R, groups, per_blk, nblk


def bn_workspace_elems(P, C):
    g = bn_geom(P, C)
    return 0 if g is None else g[4] * 2 * C + 7 * C


def bn_nblk_from_workspace(ws_elems, C):
    return (ws_elems - 7 * C) // (2 * C)


def _bn_min_p(C):
    """Smallest supported P with at least 2 pixels."""
    m = 8 // math.gcd(C, 8)
    return m * -(-2 // m)


# (C, P, why).  T = C / gcd(C, 8) vectors per channel period, R = 256 / T periods per pass.
BN_GEOMETRY = [
    (8, _bn_min_p(8), "T = 1, R = 256: one vector per period"),
    (9, _bn_min_p(9), "odd C: 8 pixels per period, reps = 8, R = 28 (4 idle threads)"),
    (12, _bn_min_p(12), "gcd 4: T = 3, R = 85 (one idle thread)"),
    (16, _bn_min_p(16), "T = 2, R = 128"),
    (25, _bn_min_p(25), "odd C: T = 25, R = 10 (6 idle threads)"),
    (1000, _bn_min_p(1000), "T = 125, R = 2: a partly idle block, 4 finalize blocks of C / 64"),
    (2040, _bn_min_p(2040), "T = 255, R = 1, one idle thread"),
    (2048, _bn_min_p(2048), "T = 256, R = 1: the largest C"),
]
# the 4-way unrolled loop of bn_reduce_part_kernel: 4R - 1, 4R and 4R + 1 period groups
# (the last makes two blocks).  C = 9: R = 28, 8 pixels per group; C = 50: R = 10, 4 pixels.
BN_UNROLL = [(9, 8 * 111), (9, 8 * 112), (9, 8 * 113), (50, 4 * 39), (50, 4 * 40), (50, 4 * 41)]
for _C, _P in BN_UNROLL:
    _T, _R, _groups = bn_geom(_P, _C)[:3]
    assert _groups - 4 * _R in (-1, 0, 1), (_C, _P)
# reduction blocks: bn_finalize_kernel adds them in 16 slices, 4-way unrolled (boundaries at
# 16 and 64 blocks).  C = 50: 40 groups of 4 pixels per block, so P = 160·nblk.
BN_NBLK = [(50, 160 * n, n) for n in (1, 15, 16, 17, 63, 64, 65)]
for _C, _P, _n in BN_NBLK:
    assert bn_geom(_P, _C)[4] == _n, (_C, _P, _n)
# grid-stride apply: above 2048 x 256 vectors a thread takes a second vector and the running
# channel offset (c0 += step) is used, forward and backward
BN_GRID_STRIDE = [
    (50, 196608),    # 1,228,800 vectors: two or three per thread, step = 4
    (9, 466040),     # 524,295 vectors: only seven threads take a second one
]
for _C, _P in BN_GRID_STRIDE:
    assert _P * _C // 8 > BN_APPLY_MAX_BLOCKS * BN_THREADS and bn_geom(_P, _C)
BN_EVAL = [(9, 8 * 113), (50, 160 * 17)]
BN_NULL_PARAMS = (50, 160 * 17)
BN_STATS = [(50, 65536), (9, 8 * 113), (16, 4096)]   # save_mean / save_invstd against float64
BN_STRESS = (16, 65536)                              # 128 blocks
BN_DETERMINISM = (50, 160 * 65)
