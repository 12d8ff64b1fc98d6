#pragma once
#include <array>
#include <type_traits>
#include <utility>
// Forward group-action kernels for gfx950 (MI355X) + their launchers.
// Instantiated once per l_max in action_inst.hip (-DLV_INST_L=k) so the 21 degree
// variants compile in parallel; host planning lives in action.hip.
//
//   lv_group_action_fwd      block_wigner_matrix_multiply, lie_tools.py:226-253
//   lv_fused_exp_action_fwd  mu@rodrigues(v) -> ZYZ -> block D·F in one pass
//                            (reparameterize.py:269-273, vae.py:182, decoders.py:47-56)
//   lv_wigner_d_fwd          packed D_l blocks 0..L; lv_wigner_d_block_fwd: D_l alone
//                            (their VJPs: wigner_bwd.h)
//
// Two forward kernels:
//   * action_fwd_tile_kernel (shared spectrum, LDS tile fits): one block per sample
//     group, one wave per degree segment; the per-sample prologue runs once per
//     (sample, Euler slot) into an LDS table of multiples, the group's whole output is
//     staged in LDS and written as one contiguous run of 16-byte stores;
//   * action_fwd_kernel (per-sample spectrum, or a tile too large for LDS): blocks of
//     4 waves on one degree segment (gridDim.y), row-pair stores straight from registers.
#include "action_common.h"

namespace lv {

// Forward, no LDS tile.  Per degree each lane runs the factored chain on its column and
// stores its (2l+1) outputs straight from registers.  There is no global load after the
// first store (vmcnt retires in order, so a later load would wait for every older store):
// a shared spectrum is staged into LDS up front and a per-sample spectrum is prefetched
// one degree ahead.
template <int LT, bool FUSED, bool SHARED, typename OutT>
__global__ __launch_bounds__(kThreads) void action_fwd_kernel(ActionArgs a) {
  extern __shared__ float lds[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // wave-uniform: scalar branches
  const int C = a.C, Sw = a.Sw;
  const int j = lane / C;
  const int c = lane - j * C;
  const int lo = a.seg_lo[blockIdx.y], hi = a.seg_lo[blockIdx.y + 1];
  const int rows_lo = lo * lo;
  const int frows = SHARED ? fseg_rows(lo, hi) : 0;
  const int64_t s0 = ((int64_t)blockIdx.x * kWavesPerBlock + wave) * Sw;
  const int Sv = (int)max((int64_t)0, min((int64_t)Sw, a.n - s0));
  const bool active = j < Sv;
  const int64_t s = active ? s0 + j : (Sv > 0 ? s0 : 0);  // idle lanes mirror a valid sample
  LaneIn in;
  if (Sv > 0) lane_load<FUSED>(a, s, in);
  // Shared spectrum slice: loads issued now, LDS writes and the barrier after the
  // prologue maths so that both memory latencies overlap the per-lane arithmetic.
  constexpr int kFPer = 8;  // staged values per thread (bounded; a loop covers larger slices)
  float fv[kFPer];
  const int fcnt = SHARED ? (hi * hi - rows_lo) * C : 0;
  const float* fsrc = a.F + rows_lo * C;
  if constexpr (SHARED) {
#pragma unroll
    for (int k = 0; k < kFPer; ++k) {
      const int e = threadIdx.x + k * kThreads;
      fv[k] = e < fcnt ? fsrc[e] : 0.f;
    }
  }
  // l >= kTrigLdsMinL: the per-sample (cos, sin) multiples live in a wave-private LDS table
  // (one row per sample, written by the sample's first three lanes) instead of 6(l+1)
  // VGPRs per lane -- 202 -> ~120 VGPRs at l = 20, i.e. 4 instead of 2 waves per SIMD.
  constexpr bool TL = LT >= kTrigLdsMinL;
  constexpr int kRow = TrigLds<LT>::kRow;
  float* trow = lds + a.fpitch + wave * Sw * kRow;
  float c1[3], s1[3];
  TrigTab<TL ? 0 : LT> t;
  if (Sv > 0) {
    lane_angles<FUSED>(a, in, s, active, c, FUSED && a.ang_out && blockIdx.y == 0, c1, s1);
    if constexpr (TL) {
      if (j < Sw)
        for (int q = c; q < 3; q += C) trig_row_fill<LT>(trow + j * kRow, c1, s1, q, hi - 1);
      if constexpr (!SHARED) wave_lds_sync();
    } else {
      trig_fill<LT>(t, c1, s1, hi - 1);
    }
  }
  const float* tj = trow + min(j, Sw - 1) * kRow;
  if constexpr (SHARED) {
#pragma unroll
    for (int k = 0; k < kFPer; ++k) {
      const int e = threadIdx.x + k * kThreads;
      if (e < fcnt) {
        const int r = e / C, cc = e - r * C;
        lds[cc * frows + r] = fv[k];
      }
    }
    for (int e = threadIdx.x + kFPer * kThreads; e < fcnt; e += kThreads) {
      const int r = e / C, cc = e - r * C;
      lds[cc * frows + r] = fsrc[e];
    }
    __syncthreads();
  }
  if (Sv == 0) return;  // whole wave idle (no block barriers below)

  OutT* out = reinterpret_cast<OutT*>(a.out);
  const float* Fl = lds + c * frows - rows_lo;                  // shared: LDS column
  const float* Fs = a.F + s * a.Fstride + c;                    // per-sample: global
  float fpre[SHARED ? 1 : 2 * LT + 1];

  sfor<LT + 1>([&](auto Lc) {
    constexpr int l = LV_CV(Lc);
    if (l >= lo && l < hi) {
      constexpr int nn = 2 * l + 1;
      constexpr int r0 = l * l;
      float x[nn], y[nn];
      if constexpr (SHARED) {
        sfor<nn>([&](auto K) { x[LV_CV(K)] = Fl[r0 + LV_CV(K)]; });
      } else {
        if (l == lo) {
          sfor<nn>([&](auto K) { x[LV_CV(K)] = Fs[(r0 + LV_CV(K)) * C]; });
        } else {
          sfor<nn>([&](auto K) { x[LV_CV(K)] = fpre[LV_CV(K)]; });
        }
        if constexpr (l < LT) {
          if (l + 1 < hi) {
            constexpr int r1 = (l + 1) * (l + 1);
            sfor<nn + 2>([&](auto K) { fpre[LV_CV(K)] = Fs[(r1 + LV_CV(K)) * C]; });
          }
        }
      }
      if constexpr (TL) {
        xrot_lds<l, 2, LT>(tj, x, y);
        jmul<l>(y, x);
        xrot_lds<l, 1, LT>(tj, x, y);
        jmul<l>(y, x);
        xrot_lds<l, 0, LT>(tj, x, y);
      } else {
        xrot<l, 2>(t, x, y);
        jmul<l>(y, x);
        xrot<l, 1>(t, x, y);
        jmul<l>(y, x);
        xrot<l, 0>(t, x, y);
      }
      if ((C & 1) == 0) {
        // Row pairs: adjacent lanes (c even, c+1) swap one value (DPP quad_perm, no LDS)
        // so that even lanes store (row i, cols c..c+1) and odd lanes (row i+1, cols
        // c-1..c): one 8-byte store per lane writes two whole rows of every sample
        // (80-B runs at C = 10).  A pair never straddles samples since C is even.
        const bool odd = (c & 1) != 0;
        OutT* d = out + s * a.MC + r0 * C + (odd ? C + c - 1 : c);
        sfor<nn / 2>([&](auto P) {
          constexpr int i = 2 * LV_CV(P);
          const float send = odd ? y[i] : y[i + 1];
          const float recv = dpp_swap_adjacent(send);
          const float v0 = odd ? recv : y[i];
          const float v1 = odd ? y[i + 1] : recv;
          if (active) store_out2(d, v0, v1);
          d += 2 * C;
        });
        if (active) store_out(out + s * a.MC + (r0 + nn - 1) * C + c, y[nn - 1]);
      } else if (active) {
        // one store per output row: Sw contiguous C-value pieces per instruction; a
        // sample's rows are adjacent, so L2 merges them into whole lines
        OutT* d = out + s * a.MC + r0 * C + c;
        sfor<nn>([&](auto I) {
          store_out(d, y[LV_CV(I)]);
          d += C;
        });
      }
    }
  });
}

// ------------------------------------------------------------- tile forward
// Output staging: every wave parks its outputs in the block's LDS tile [j][row][c] --
// exactly the global layout of the group's Sw consecutive samples -- so after one block
// barrier the tile leaves as ONE contiguous run of Sw * M * C values: 16-byte stores,
// 1 KiB per wave instruction, whole 128-B lines.  POL selects the store cache policy
// (buffer-store aux bits on gfx950): 1 nt, 16 sc1 (write-through: the bytes leave the
// XCD's L2 during the kernel instead of as dirty lines written back at the kernel
// boundary; measured best while the output is small, nt beyond).
typedef float lv_f4 __attribute__((ext_vector_type(4)));

template <int POL>
__device__ __forceinline__ void tile_store16(__amdgpu_buffer_rsrc_t r, int off, lv_f4 v) {
  __builtin_amdgcn_raw_buffer_store_b128(v, r, off, 0, POL);
}
template <int POL>
__device__ __forceinline__ void tile_store_elem(__amdgpu_buffer_rsrc_t r, int off, float v) {
  __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned int, v), r, off, 0, POL);
}
template <int POL>
__device__ __forceinline__ void tile_store_elem(__amdgpu_buffer_rsrc_t r, int off,
                                                __hip_bfloat16 v) {
  __builtin_amdgcn_raw_buffer_store_b16(__builtin_bit_cast(short, v), r, off, 0, POL);
}
__device__ __forceinline__ float tile_cvt(float v, float*) { return v; }
__device__ __forceinline__ __hip_bfloat16 tile_cvt(float v, __hip_bfloat16*) {
  return __float2bfloat16(v);
}

// Buffer descriptor word 3 for raw (untyped) buffer access on gfx9-family parts.
constexpr int kRawBufferFlags = 0x00020000;

// LDS bytes of the output tile (+16 for the alignment shift).
__host__ __device__ inline int tile_stage_bytes(int Sw, int64_t MC, int out_bytes) {
  return (int)((((int64_t)Sw * MC * out_bytes + 16) + 15) & ~(int64_t)15);
}

// Write a staged tile back: head elements up to the first 16-B boundary, the 16-B
// body (ds_read_b128 -> buffer_store_dwordx4, 1 KiB per wave instruction), tail elements.
// The LDS tile starts `mis` bytes past a 16-B boundary, mis = gout mod 16, so LDS and
// global addresses agree mod 16.
template <typename OutT, int POL>
__device__ __forceinline__ void tile_flush(OutT* gout, const char* stage_b, int mis, int nbytes,
                                           int tid, int nthr) {
  const int head = min((16 - mis) & 15, nbytes);
  const int nvec = (nbytes - head) >> 4;
  const int tail0 = head + nvec * 16;
  const __amdgpu_buffer_rsrc_t rs =
      __builtin_amdgcn_make_buffer_rsrc(gout, 0, nbytes, kRawBufferFlags);
  for (int k = tid; k < nvec; k += nthr) {
    const lv_f4 v = *reinterpret_cast<const lv_f4*>(stage_b + head + 16 * k);
    tile_store16<POL>(rs, head + 16 * k, v);
  }
  constexpr int E = (int)sizeof(OutT);
  const int nedge = head / E + (nbytes - tail0) / E;
  if (tid < nedge) {
    const int b = tid < head / E ? tid * E : tail0 + (tid - head / E) * E;
    tile_store_elem<POL>(rs, b, *reinterpret_cast<const OutT*>(stage_b + b));
  }
}

// Block barrier for LDS hand-offs only: waits for this wave's LDS operations, never for
// its global stores (a __syncthreads() release fence may emit s_waitcnt vmcnt(0) and
// stall on stores still in flight).
__device__ __forceinline__ void block_sync_lds() {
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

// The store policy picked at run time (uniform branch; aux bits must be immediates).
template <typename OutT>
__device__ __forceinline__ void tile_flush_rt(OutT* gout, const char* stage_b, int mis, int nbytes,
                                              int write_through) {
  if (write_through == 1)
    tile_flush<OutT, 16>(gout, stage_b, mis, nbytes, (int)threadIdx.x, (int)blockDim.x);
  else if (kAbKnobs && write_through == 2)
    tile_flush<OutT, 0>(gout, stage_b, mis, nbytes, (int)threadIdx.x, (int)blockDim.x);
  else
    tile_flush<OutT, 1>(gout, stage_b, mis, nbytes, (int)threadIdx.x, (int)blockDim.x);
}

// s_setprio takes an immediate: p is wave-uniform (SGPR), so these are scalar branches around
// one s_setprio each (a divergent guard would run the instruction in every wave).
__device__ __forceinline__ void set_wave_prio(int p) {
  if (p <= 0) __builtin_amdgcn_s_setprio(0);
  else if (p == 1) __builtin_amdgcn_s_setprio(1);
  else if (p == 2) __builtin_amdgcn_s_setprio(2);
  else __builtin_amdgcn_s_setprio(3);
}

// Priority class of this block, 0 (favoured) .. nclass - 1, nclass 2 or 3; scalar arithmetic
// on blockIdx.x or on the hardware-ID register, so wave-uniform.  Blocks are dealt round-
// robin over the 8 XCDs and, within one, over its CUs: blockIdx.x >> 3 is the dealing round
// and blockIdx.x >> log2(total CUs) counts the blocks a CU already holds when every block is
// resident (the plan's condition for classes).  kClassMapSlot reads the workgroup's slot on
// its CU instead: HW_ID (hardware register 4) bits 19:16, TG_ID, on GCN / CDNA parts.
__device__ __forceinline__ int tile_block_class(int nclass, int class_map) {
  constexpr int kHwIdTgId = 4 | (16 << 6) | ((4 - 1) << 11);  // hwreg(HW_REG_HW_ID, 16, 4)
  unsigned x;
  if (class_map & kClassMapSlot) x = __builtin_amdgcn_s_getreg(kHwIdTgId);
  else x = blockIdx.x >> (class_map & kClassMapShift);
  x = __builtin_amdgcn_readfirstlane(x);
  return (int)(nclass == 2 ? (x & 1u) : x % 3u);
}

// Operand prefetch of the tile kernel's chain (fwd_tile_body `degree`): how many of the next
// rotation's multiples a lane holds in registers across the J product in front of it.  A
// fixed choice per kernel and degree, like kTilePrio, against the kernel's VGPR ceiling:
//   * up to l_max = 10 the ceiling is 64, 8 waves per SIMD: the 8-wave plan (batch 16,384)
//     runs 4 blocks per CU there and 3 from 65 VGPRs (16.8 -> 17.9 us measured with a build
//     that held the reads' unused lanes, 65 VGPRs).  Every degree holds all 2l multiples:
//     the compiler finishes one parity block of J_l before the other, so the held values
//     fit beside the product -- the l_max = 10, C = 10, fp32 kernel compiles to 61 VGPRs
//     against 62 at depth 0;
//   * beyond, 104: the l = 20 bf16 kernel of config 5 needs every one of its 4 wave slots per
//     SIMD and stood at 96-97.  There a degree's product has its 2(2l + 1) input and output
//     values live and kChainRegsOther more (addresses, lane indices, temporaries: 82 + 14 at
//     l = 20); full depth may add 2(l + 1), half depth the first (l + 4) / 8 quads of cos and
//     sin.  Low degrees get the full depth for free: the top degree sets the register count.
constexpr int kChainDepthOff = 0, kChainDepthHalf = 1, kChainDepthFull = 2;
constexpr int kChainRegsOther = 16;
constexpr int kChainFullMaxL = 10;
constexpr int tile_vgpr_ceiling(int LT) { return LT <= kChainFullMaxL ? 64 : 104; }
// depth of degree l in the kernel of l_max LT (compile-time in the kernel; the plan query
// reports it)
constexpr int chain_depth(int LT, int l) {
  if (LT <= kChainFullMaxL) return kChainDepthFull;
  const int ceiling = tile_vgpr_ceiling(LT);
  const int live = 2 * (2 * l + 1) + kChainRegsOther;
  if (live + 2 * (l + 1) <= ceiling) return kChainDepthFull;
  if ((l + 4) / 8 > 0 && live + 8 * ((l + 4) / 8) <= ceiling) return kChainDepthHalf;
  return kChainDepthOff;
}
static_assert(chain_depth(10, 10) == kChainDepthFull && chain_depth(20, 20) == kChainDepthOff,
              "chain depth: config 2 prefetches its top degree, config 5's top degree has no room");

// The planner's per-wave chain cost targets (plan_tile, action.hip, which documents the
// measurements behind them) and the wave count they give -- here, next to the kernel, because
// the kernel compiles out what no plan of its l_max can reach (tile_min_waves).
constexpr double kTileSegCostFew = 300.0;    // -> 7 waves at l = 10
constexpr double kTileSegCostMid = 260.0;    // -> 8
constexpr double kTileSegCostLarge = 560.0;  // -> 4
constexpr int kTileMaxWaves = 8;
template <int... Ls>
constexpr std::array<int, sizeof...(Ls)> nnz_table(std::integer_sequence<int, Ls...>) {
  return {j_nnz<Ls>()...};
}
constexpr auto kNnz = nnz_table(std::make_integer_sequence<int, LV_MAX_DEGREE + 1>{});
// Lane-instruction cost of one degree of the forward chain (FMA-pairs + loads + staging).
constexpr double chain_degree_cost(int l) { return 2.0 * kNnz[l] + 6.0 * (2 * l + 1) + 3.0 * (2 * l + 1); }
constexpr double chain_total_cost(int L) {
  double total = 0.0;
  for (int l = 0; l <= L; ++l) total += chain_degree_cost(l);
  return total;
}
// waves per block for a per-wave cost target: ceil(total / target) within [1, min(8, L + 1)]
constexpr int tile_waves(int L, double target) {
  const double total = chain_total_cost(L);
  int k = (int)(total / target);
  if (k * target < total) ++k;
  const int cap = kTileMaxWaves < L + 1 ? kTileMaxWaves : L + 1;
  return k < 1 ? 1 : (k > cap ? cap : k);
}
// The fewest waves any product plan gives a block of the l_max = L kernel, whatever the batch
// and the channel count: the wave count of the largest cost target.  (The prologue's thread
// count only raises a plan's count, and the product does not read the A/B knobs.)
constexpr int tile_min_waves(int L) {
  const double t = kTileSegCostFew > kTileSegCostMid ? kTileSegCostFew : kTileSegCostMid;
  return tile_waves(L, t > kTileSegCostLarge ? t : kTileSegCostLarge);
}
static_assert(tile_min_waves(5) == 1 && tile_min_waves(6) == 2 && tile_min_waves(8) == 3 &&
                  tile_min_waves(10) == 4 && tile_waves(10, kTileSegCostFew) == 7,
              "tile plan: one-wave blocks up to l_max = 5; config 2 runs 7 waves, l = 10 never fewer than 4");

// Tile kernel.  One block = one sample group (Sw = 64 / C samples, one wave's lanes) x
// nseg degree segments, one wave per segment.
//   1. Prologue ONCE per (sample j, Euler slot q): the block's first 3*Sw threads each
//      load one sample's v (and mu), run exp -> ZYZ (cos, sin) and the multiples of
//      slot q (trig_row_fill: the same recurrence as trig_fill, bitwise) into the
//      block's LDS table.  Every segment wave used to repeat the whole prologue on all
//      its lanes: 5x the work at batch 4096 and ~40% of the kernel's VALU stream.
//   2. Meanwhile each wave stages its spectrum slice; one barrier publishes both.
//   3. Chain per degree with the multiples read from LDS one rotation ahead, across the J
//      product in front of their use (chain_depth above; 61 VGPRs at l = 10, C = 10).
//   4. Outputs parked in the LDS tile; barrier; one contiguous flush.
// CT: compile-time C (0 = run-time a.C).  With CT the spectrum slice is staged row-major
// ([row][c], no index division, immediate-offset reads); without it column-major.
// With CT the waves' row-major slices are contiguous: the block holds the whole spectrum
// once (M*C floats, 17.6 KB at l = 20) and each wave stages and reads its own rows.  With
// run-time C from l_max >= kTileFGlobalMinL the spectrum is read from global memory
// instead (no global store precedes the flush, so these loads never wait behind stores);
// that costs ~10 cycles of address processing per wave load instruction, which is why
// the C = 10 path keeps it in LDS (l = 20 bf16: 18.5 -> 5 us of skeleton, tools/c5bench).
// MAYMU = false: compiled without the mean-rotation (mu) prologue (a.mu must be null).
template <int LT, int CT, bool FUSED, typename OutT, bool MAYMU = true>
__device__ __forceinline__ void fwd_tile_body(const ActionArgs& a, int64_t grp) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int kRow = TrigLds<LT>::kRow;
  constexpr bool FG = CT == 0 && LT >= kTileFGlobalMinL;  // spectrum from global, no LDS
  // fp32 tile with compile-time C: the spectrum lives in the tile's LAST sample slot
  // (same [row][c] layout, M*C floats).  A wave reads degree l's spectrum rows into
  // registers before it writes that degree's tile rows, and no other wave touches those
  // rows, so the slot is free to be overwritten; the block saves M*C*4 bytes of LDS
  // (l = 10: 35.7 -> 30.9 KB, 4 -> 5 blocks per CU).
  constexpr bool FT = CT > 0 && std::is_same_v<OutT, float>;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // wave-uniform: scalar branches
  const int tid = (int)threadIdx.x;
  // Start-up: every launch argument the prologue reads ahead of its first global load, as
  // ONE batch of scalar loads behind one wait (the empty asm needs them all in registers
  // here).  The scalar cache is cold at every launch; fetched where they were first used
  // the fields took four serial round trips before the task lanes' v load was issued.
  const float* const vin = FUSED ? a.v : a.ang;
  const float* const aF = a.F;
  void* const aout = a.out;
  float* const aang = a.ang_out;
  const int64_t an = a.n;
  const int Sw = a.Sw;  // 64 / C, or fewer (plan: LDS per block vs blocks per CU)
  // (the product's kernels hold the A/B-only fields as constants: action_common.h kAbKnobs)
  const int prio = kAbKnobs ? a.prio : kTilePrio, spread = kAbKnobs ? a.task_spread : 0;
  const int transp = a.transpose, wthrough = a.write_through;
  const int ang_order = kAbKnobs ? a.ang_order : 0;
  const int nclass = kAbKnobs ? a.nclass : 0, class_map = kAbKnobs ? a.class_map : 0;
  const int cfetch = kAbKnobs ? a.chain_fetch : 1;
  // this wave's degrees: a bit set (compile-time C: any set the planner balanced by cost);
  // run-time C keeps contiguous ranges [lo, hi) for its column-major spectrum slices
  const unsigned dmask = a.seg_mask[wave];
  const int nthr = (int)blockDim.x;
  if constexpr (kAbKnobs)
    asm volatile("" ::"s"(vin), "s"(aF), "s"(aout), "s"(aang), "s"(an), "s"(Sw), "s"(prio), "s"(spread),
                 "s"(transp), "s"(ang_order), "s"(wthrough), "s"(nclass), "s"(class_map), "s"(dmask),
                 "s"(nthr), "s"(cfetch));
  else
    asm volatile("" ::"s"(vin), "s"(aF), "s"(aout), "s"(aang), "s"(an), "s"(Sw), "s"(transp),
                 "s"(wthrough), "s"(dmask), "s"(nthr));
  // Wave priority (a.prio, the plan's default 2): the prologue (v / mu loads, exp -> ZYZ,
  // multiples, spectrum staging) issues at s_setprio 3 and the chain at 0, so on a CU that
  // holds blocks in different phases a new block's loads start ahead of the other blocks'
  // FMA streams (tools/gpu_fwd_knobs.sh, profiles/r03_fwd_prio_ab.txt: batch 16,384
  // 20.96 -> 18.27 us, 65,536 63.6 -> 61.1, 262,144 256 -> 252; 4,096, where every block
  // starts at once, unchanged).  1 / 3: A/B variants with the flush raised.
  phase_stamp(a.stamps, wave, 0);
  if (prio >= 2) __builtin_amdgcn_s_setprio(3);
  const int nw = nthr >> 6;
  const int64_t s0 = grp * Sw;
  const int Sv = (int)min((int64_t)Sw, an - s0);  // >= 1: grp < ceil(n / Sw)
  // v (angles) and ang_out of the group through buffer resources based at its first sample:
  // per-lane 32-bit byte offsets, no 64-bit address arithmetic on the lanes (as tile_flush
  // addresses out)
  const __amdgpu_buffer_rsrc_t vrs = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float*>(vin) + s0 * 3, 0, Sv * 12, kRawBufferFlags);
  auto load3 = [&](int js, float x[3]) {
    // (three 4-byte loads, which the compiler merges into one buffer_load_dwordx3)
#pragma unroll
    for (int i = 0; i < 3; ++i)
      x[i] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(vrs, js * 12 + 4 * i, 0, 0));
  };
  // 1. prologue task (sample jt, slot q); the host guarantees 3*Sw <= blockDim.x
  // task_spread: task t on lane t / nw of wave t % nw, so the prologue's serial chains run on
  // every SIMD of the CU instead of all in wave 0
  const int t_task = spread ? lane * nw + wave : tid;
  const bool task = t_task < 3 * Sw;
  const int jt = (t_task * 683) >> 11, q = t_task - 3 * jt;  // t / 3, exact below 2,045
  const int64_t st = s0 + min(jt, Sv - 1);  // idle slots mirror a valid sample
  LaneIn in;
  if (task) {
    load3(min(jt, Sv - 1), in.v);
    if constexpr (FUSED && MAYMU) {
      if (a.mu) {
#pragma unroll
        for (int i = 0; i < 9; ++i) in.mu[i] = a.mu[st * 9 + i];
      }
    }
  }
  const int C = CT > 0 ? CT : a.C;
  const int64_t MC = CT > 0 ? (int64_t)(LT + 1) * (LT + 1) * CT : a.MC;
  const int j = lane / C;
  const int c = lane - j * C;
  const int lo = a.seg_lo[wave], hi = a.seg_lo[wave + 1];
  const int rows_lo = lo * lo;
  const int frows = fseg_rows(lo, hi);
  const bool active = j < Sv;
  const int stage_bytes = tile_stage_bytes(Sw, MC, (int)sizeof(OutT));
  float* trig = lds + (stage_bytes >> 2);
  OutT* gout = reinterpret_cast<OutT*>(aout) + s0 * MC;
  const int mis = (int)(reinterpret_cast<uintptr_t>(gout) & 15);
  char* stage_b = reinterpret_cast<char*>(lds) + mis;  // LDS addr = global addr (mod 16)
  // spectrum in LDS: CT > 0 the whole (M, C) row-major, staged by all threads of the block
  // (FT: in the tile's last sample slot), else per-wave column-major slices of a.fpitch
  float* const Fall = FT ? reinterpret_cast<float*>(stage_b) + (Sw - 1) * MC : trig + Sw * kRow;
  float* Fw = Fall + (CT > 0 ? 0 : wave * a.fpitch);
  // The mu-free fused kernel writes ang_out (the product operator's saved angles) from
  // waves 1 and 2, lanes j < Sv -- waves that only stage spectrum rows in the prologue, on
  // other SIMDs than the task lanes of wave 0 -- instead of on the q = 0 task lanes, where
  // quat_to_eazyz_fwd's atan2 / acos held wave 0's multiples by ~0.5 us per launch.  Same
  // quaternion (exp_quat), so the same angles bit for bit.  Wave 1 writes alpha and gamma,
  // wave 2 beta = saved_beta of the forward's own (cos, sin) pair (a longer chain than the
  // acos it replaces: all three on wave 1 cost 0.11 us per launch at config 2, split
  // 0.06 us); a two-wave block writes all three from wave 1, a one-wave block from wave 0.
  // a.ang_order 0 (the product): they run that maths (~350 VALU: exp_quat, two generic
  // atan2) before they issue their spectrum loads.  1 (A/B): their v load goes out with the
  // spectrum loads and the maths runs AFTER the prologue barrier, ahead of their chain (the
  // planner then charges them for it, balance_masks); that takes them off the path to the
  // barrier but puts ~550 wave-instructions on the VALU-bound chain: 6.74-6.77 us against
  // 6.65-6.68 at config 2 (profiles/r07_ab_startup_c2.txt), so 0 stays.  A one-wave block
  // always writes behind the barrier.
  // The product's kernel holds that second copy -- ~300 instructions at the chain's first
  // address, which every wave branches over -- only where a product plan of this l_max can
  // have a one-wave block (kMinWaves, tile_min_waves: up to l_max = 5); beyond, the angle
  // waves' indices are constants too wherever every plan has them (wave 1 from two waves,
  // l_max >= 6; wave 2 from three, l_max >= 8).  The A/B library, whose knobs force wave
  // counts and placement 1, keeps all of it.  Measured at config 2: DESIGN.md section 9, "The
  // one-wave code out of the kernels that never run one wave".
  constexpr int kMinWaves = kAbKnobs ? 1 : tile_min_waves(LT);
  constexpr bool kAngLate = FUSED && !MAYMU;
  constexpr bool kAngBehind = kAngLate && kMinWaves == 1;
  const int ang_wave = (kMinWaves > 1 || nw > 1) ? 1 : 0;
  const int beta_wave = (kMinWaves > 2 || nw > 2) ? 2 : ang_wave;
  const bool ang_on = kAngLate && aang != nullptr && lane < Sv;
  const bool dirs_lane = ang_on && wave == ang_wave, beta_lane = ang_on && wave == beta_wave;
  const bool ang_early = !kAngBehind || (ang_order == 0 && nw > 1);
  float vang[3] = {0.f, 0.f, 0.f};
  if (dirs_lane || beta_lane) load3(lane, vang);
  auto write_ang = [&]() {
    const __amdgpu_buffer_rsrc_t ars =
        __builtin_amdgcn_make_buffer_rsrc(aang + s0 * 3, 0, Sv * 12, kRawBufferFlags);
    const ExpQuat e = exp_quat(vang);
    if (dirs_lane) {
      float ang[3];
      quat_to_eazyz_fwd(e.qr, ang);
      __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned int, ang[0]), ars, lane * 12, 0, 0);
      __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned int, ang[2]), ars, lane * 12 + 8, 0, 0);
    }
    if (beta_lane) {
      float cb, sb;
      exp_beta(e, cb, sb);
      __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned int, saved_beta(cb, sb)), ars,
                                            lane * 12 + 4, 0, 0);
    }
  };
  if constexpr (kAngLate) {
    if ((dirs_lane || beta_lane) && ang_early) write_ang();
  }
  // 2. spectrum staging: every load issued now (before the prologue maths), the LDS writes
  //    after it.  CT > 0: element e = tid + k * nthr of the whole (M, C) spectrum, in as
  //    many slots as the block's thread count needs (three tiers: from 7, from 4, fewer
  //    waves; a batched loop beyond kFPerCap slots).  A lane past the end re-stages the
  //    last element (clamped index: the same value to the same LDS word), so no slot is
  //    guarded -- sized for the 2-wave block and guarded twice, the 10 slots at l = 10
  //    cost the 7-wave block 20 exec-mask regions of which 3 + 3 did work.
  //    Run-time C: this wave's column-major slice.
  constexpr int kFPer = FG ? 1 : (CT > 0 ? ((LT + 1) * (LT + 1) * (CT > 0 ? CT : 1) + 127) / 128 : 6);
  constexpr int kFPerCap = kFPer < 18 ? kFPer : 18;
  constexpr int kMCT = (LT + 1) * (LT + 1) * (CT > 0 ? CT : 1);
  constexpr int kSlots7 = (kMCT + 447) / 448 < kFPerCap ? (kMCT + 447) / 448 : kFPerCap;
  constexpr int kSlots4 = (kMCT + 255) / 256 < kFPerCap ? (kMCT + 255) / 256 : kFPerCap;
  static_assert(CT == 0 || kSlots4 * 256 >= kMCT, "tile staging: the 4-wave tier covers the spectrum");
  float fv[kFPerCap];
  const int fcnt = FG ? 0 : (CT > 0 ? (int)MC : (hi * hi - rows_lo) * C);
  const int fstr = CT > 0 ? nthr : 64;
  const int fbase = CT > 0 ? tid : lane;
  const float* fsrc = aF + (CT > 0 ? 0 : rows_lo * C);
  if constexpr (CT > 0) {
    auto ld = [&](auto K) { fv[LV_CV(K)] = fsrc[min(tid + nthr * LV_CV(K), kMCT - 1)]; };
    if (nw >= 7) sfor<kSlots7>(ld);
    else if (nw >= 4) sfor<kSlots4>(ld);
    else sfor<kFPerCap>(ld);
  } else {
#pragma unroll
    for (int k = 0; k < kFPerCap; ++k) {
      const int e = fbase + fstr * k;
      fv[k] = e < fcnt ? fsrc[e] : 0.f;
    }
  }
  if constexpr (kStamps) {
    if (a.stamps) {  // A/B timeline: when this wave's loads (v; spectrum) have landed
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      phase_stamp(a.stamps, wave, 5);
    }
  }
  if (task) {
    float cq, sq;
    if constexpr (FUSED && !MAYMU) {
      // z = exp(v): this thread's slot only (transpose: slot q takes angle 2 - q, sine negated)
      // ang_out is not written here (see above)
      float qr[4];
      exp_to_zyz_slot(in.v, transp ? 2 - q : q, cq, sq, qr);
      if (transp) sq = -sq;
    } else {
      float c1[3], s1[3];
      lane_angles<FUSED, MAYMU>(a, in, st, jt < Sv, q, FUSED && aang != nullptr, c1, s1);
      cq = q == 0 ? c1[0] : (q == 1 ? c1[1] : c1[2]);
      sq = q == 0 ? s1[0] : (q == 1 ? s1[1] : s1[2]);
    }
    phase_stamp(a.stamps, wave, 6);
    trig_row_fill1<LT>(trig + jt * kRow, cq, sq, q, LT);
    phase_stamp(a.stamps, wave, 7);
  }
  if constexpr (FG) {
  } else if constexpr (CT > 0) {
    auto wr = [&](auto K) { Fw[min(tid + nthr * LV_CV(K), kMCT - 1)] = fv[LV_CV(K)]; };
    if (nw >= 7) sfor<kSlots7>(wr);
    else if (nw >= 4) sfor<kSlots4>(wr);
    else {
      sfor<kFPerCap>(wr);
      for (int e0 = fbase + fstr * kFPerCap; e0 < fcnt; e0 += 8 * fstr) {
        float t8[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) t8[u] = e0 + fstr * u < fcnt ? fsrc[e0 + fstr * u] : 0.f;
#pragma unroll
        for (int u = 0; u < 8; ++u)
          if (e0 + fstr * u < fcnt) Fw[e0 + fstr * u] = t8[u];
      }
    }
  } else {
#pragma unroll
    for (int k = 0; k < kFPerCap; ++k) {
      const int e = lane + 64 * k;
      if (e < fcnt) {
        const int r = e / C, cc = e - r * C;
        Fw[cc * frows + r] = fv[k];
      }
    }
    for (int e = lane + 64 * kFPerCap; e < fcnt; e += 64) {
      const int r = e / C, cc = e - r * C;
      Fw[cc * frows + r] = fsrc[e];
    }
  }
  block_sync_lds();
  phase_stamp(a.stamps, wave, 1);

  // Chain priority: 0 after the prologue's 3.  A/B (LV_TILE_NCLASS, plan_tile): with block
  // classes the blocks that share a CU run their chains -- and flushes -- at priorities 2, 1,
  // 0 by class.  Scheduling only; measured at config 2 it changes nothing, because VALU
  // issue goes by priority and THEN AGE: at equal priority the block a CU received first
  // already ends its chain ~0.9 us ahead of the second and that ~0.9 us ahead of the third
  // (profiles/r08_timeline_block_classes.txt), the order the classes impose.  Not in the
  // product's code.
  int cprio = 0, cls = -1;
  if (nclass > 1) {
    cls = tile_block_class(nclass, class_map);
    cprio = nclass - 1 - cls;
  }
  class_stamp(a.stamps, wave, cls);
  if (cprio == 2) __builtin_amdgcn_s_setprio(2);
  else if (cprio == 1) __builtin_amdgcn_s_setprio(1);
  else if (prio >= 2) __builtin_amdgcn_s_setprio(0);
  if constexpr (kAngBehind) {
    if ((dirs_lane || beta_lane) && !ang_early) write_ang();
  }
  OutT* st_lane = reinterpret_cast<OutT*>(stage_b) + j * MC + c;
  const float* tj = trig + min(j, Sw - 1) * kRow;
  // spectrum column: LDS slice, or global (FG)
  const float* Fl = FG ? aF + c : (CT > 0 ? Fall + c : Fw + c * frows - rows_lo);
  const int fstep = (FG || CT > 0) ? C : 1;  // stride between consecutive rows of a column

  // One degree of the chain at operand-prefetch depth D (chain_depth).  Depth 0 reads every
  // operand right before its use (xrot_lds): four exposed LDS round trips per degree on the
  // wave's serial path.  From depth 1 the spectrum column and slot c's multiples leave as one
  // batch behind one wait, and the multiples of the next rotation are issued BEFORE the J
  // product that precedes it and consumed after it -- all of them (full) or their first
  // (l + 4) / 8 quads (half, the rest at the point of use) -- so the product's ~2 nnz(J_l)
  // FMAs cover the round trip.  The addresses are known at the prologue barrier and nothing
  // the chain produces feeds them; the FMAs and their order are those of depth 0, so the
  // outputs are bitwise the same.  chain_pin holds each J product between the issue of the
  // reads and their use (left alone the compiler gathers a degree's reads at its top, at 96
  // VGPRs, or sinks them to their use).
  auto degree = [&](auto Lc, auto Dc) {
    constexpr int l = LV_CV(Lc), D = LV_CV(Dc);
    constexpr int nn = 2 * l + 1;
    constexpr int r0 = l * l;
    float x[nn], y[nn];
    if constexpr (D == kChainDepthOff) {
      sfor<nn>([&](auto K) { x[LV_CV(K)] = Fl[(r0 + LV_CV(K)) * fstep]; });
      xrot_lds<l, 2, LT>(tj, x, y);
      jmul<l>(y, x);
      xrot_lds<l, 1, LT>(tj, x, y);
      jmul<l>(y, x);
      xrot_lds<l, 0, LT>(tj, x, y);
    } else {
      constexpr int NQ = xrot_quads<l>();
      constexpr int QH = D == kChainDepthFull ? NQ : (l + 4) / 8;  // quads fetched a stage ahead
      XrotOps<l> ta, tb;
      xrot_fetch<l, 2, LT, 0, NQ>(tj, ta);
      sfor<nn>([&](auto K) { x[LV_CV(K)] = Fl[(r0 + LV_CV(K)) * fstep]; });
      xrot_apply<l>(ta, x, y);
      xrot_fetch<l, 1, LT, 0, QH>(tj, tb);  // in flight over the J product
      chain_pin(y);
      jmul<l>(y, x);
      chain_pin(x);
      xrot_fetch<l, 1, LT, QH, NQ>(tj, tb);
      xrot_apply<l>(tb, x, y);
      xrot_fetch<l, 0, LT, 0, QH>(tj, ta);
      chain_pin(y);
      jmul<l>(y, x);
      chain_pin(x);
      xrot_fetch<l, 0, LT, QH, NQ>(tj, ta);
      xrot_apply<l>(ta, x, y);
    }
    if (active) {
      OutT* d = st_lane + r0 * C;
      sfor<nn>([&](auto I) {
        d[0] = tile_cvt(y[LV_CV(I)], (OutT*)nullptr);
        d += C;
      });
    }
    degree_stamp(a.stamps, wave, l);
  };
  // The product runs each degree at its compile-time depth; the A/B library also holds the
  // chain at depth 0 (ActionArgs::chain_fetch 0, LV_TILE_PREFETCH=0), the order to compare with.
  auto chain = [&](auto On) {
    sfor<LT + 1>([&](auto Lc) {
      constexpr int l = LV_CV(Lc);
      constexpr int D = LV_CV(On) ? chain_depth(LT, l) : kChainDepthOff;
      if ((dmask >> l) & 1u) degree(Lc, std::integral_constant<int, D>{});
    });
  };
  if (kAbKnobs && !cfetch) chain(std::false_type{});
  else chain(std::true_type{});
  phase_stamp(a.stamps, wave, 2);
  block_sync_lds();
  phase_stamp(a.stamps, wave, 3);
  if (prio == 1) __builtin_amdgcn_s_setprio(3);  // A/B: the flush ahead of other waves' chains
  else if (prio == 3) __builtin_amdgcn_s_setprio(2);
  else if (class_map & kClassFlushUp) set_wave_prio(cprio + 1);  // A/B: flush above the class's chain
  tile_flush_rt<OutT>(gout, stage_b, mis, Sv * (int)MC * (int)sizeof(OutT), wthrough);
  phase_stamp(a.stamps, wave, 4);
}

template <int LT, int CT, bool FUSED, typename OutT, bool MAYMU = true>
__global__ __launch_bounds__(512) void action_fwd_tile_kernel(ActionArgs a) {
  fwd_tile_body<LT, CT, FUSED, OutT, MAYMU>(a, blockIdx.x);
}


// ------------------------------------------------------------ Wigner-D blocks
// Column q of D_l = chain applied to e_q; one thread per (sample, q), one kernel per
// degree.  Sample s's block goes to D + s * pitch + off, row-major: the packed layout
// (pitch = sum_k (2k+1)^2, off = sum_{k<l} (2k+1)^2) or the block alone (pitch =
// (2l+1)^2, off = 0) -- the same values either way, only the destination differs.
template <int l>
__global__ void wigner_d_kernel(const float* ang, float* D, int64_t n, int64_t pitch, int off) {
  constexpr int nn = 2 * l + 1;
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (tid >= n * nn) return;
  const int64_t s = tid / nn;
  const int q = (int)(tid - s * nn);
  float c1[3], s1[3];
  for (int i = 0; i < 3; ++i) sincosf(ang[s * 3 + i], &s1[i], &c1[i]);
  TrigTab<l> t;
  trig_fill<l>(t, c1, s1, l);
  float x[nn], y[nn];
  sfor<nn>([&](auto K) { x[LV_CV(K)] = (LV_CV(K) == q) ? 1.f : 0.f; });
  xrot<l, 2>(t, x, y);
  jmul<l>(y, x);
  xrot<l, 1>(t, x, y);
  jmul<l>(y, x);
  xrot<l, 0>(t, x, y);
  sfor<nn>([&](auto I) { D[s * pitch + off + LV_CV(I) * nn + q] = y[LV_CV(I)]; });
}

// ------------------------------------------------------------------ host side

// Compile-time channel count of the specialised tile kernel (ActionNet's default
// rep_copies, decoders.py:11, and every BASELINE config).
constexpr int kTileFastC = 10;

struct FwdLaunch {
  ActionArgs a;
  int gx, gy;
  bool fused;
  bool tile;     // tile kernel (shared spectrum; gy = waves per block)
  size_t lds;    // tile kernel dynamic LDS bytes
  int dtype;
  hipStream_t stream;
};

// Launchers: run() is defined out of class (not implicitly inline), so that the
// `extern template` declarations in action.hip keep the host TU from instantiating --
// and the device compiler from compiling -- every kernel a second time.
template <int LT>
struct FwdLauncher {
  using Args = FwdLaunch;
  template <int CT>
  static void launch_tile(FwdLaunch& p, bool bf16);
  static int run(FwdLaunch& p);
};

template <int LT>
template <int CT>
void FwdLauncher<LT>::launch_tile(FwdLaunch& p, bool bf16) {
  const dim3 grid(p.gx), block(64 * p.gy);
  if (p.fused && CT > 0 && !p.a.mu) {
    // no mean rotation (the metric path, z = exp(v)): the instantiation without the fp64
    // mu prologue -- 1,660 -> ~700 instructions ahead of the first barrier at l = 10, so
    // fewer cold instruction-cache lines on every block's critical path
    if (bf16)
      hipLaunchKernelGGL((action_fwd_tile_kernel<LT, CT, true, __hip_bfloat16, false>), grid, block, p.lds, p.stream, p.a);
    else
      hipLaunchKernelGGL((action_fwd_tile_kernel<LT, CT, true, float, false>), grid, block, p.lds, p.stream, p.a);
  } else if (p.fused) {
    if (bf16)
      hipLaunchKernelGGL((action_fwd_tile_kernel<LT, CT, true, __hip_bfloat16>), grid, block, p.lds, p.stream, p.a);
    else
      hipLaunchKernelGGL((action_fwd_tile_kernel<LT, CT, true, float>), grid, block, p.lds, p.stream, p.a);
  } else {
    if (bf16)
      hipLaunchKernelGGL((action_fwd_tile_kernel<LT, CT, false, __hip_bfloat16>), grid, block, p.lds, p.stream, p.a);
    else
      hipLaunchKernelGGL((action_fwd_tile_kernel<LT, CT, false, float>), grid, block, p.lds, p.stream, p.a);
  }
}

template <int LT>
int FwdLauncher<LT>::run(FwdLaunch& p) {
  const bool bf16 = p.dtype == LV_DTYPE_BF16;
  if (p.tile) {
    if (!kAbKnobs && p.gy < tile_min_waves(LT)) {  // the kernel holds no code for such a block
      set_error("tile plan of %d waves below the kernel's minimum %d at l_max %d", p.gy, tile_min_waves(LT), LT);
      return LV_ERR_ARG;
    }
    if (p.a.C == kTileFastC)
      launch_tile<kTileFastC>(p, bf16);
    else
      launch_tile<0>(p, bf16);
    LV_RETURN_LAUNCH("action_fwd_tile_kernel");
  }
  const bool shared = p.a.Fstride == 0;
  const size_t lds = p.lds;  // spectrum slice + trig tables (plan_fwd in action.hip)
  const dim3 grid(p.gx, p.gy), block(kThreads);
  if (p.fused) {  // the fused path takes a shared spectrum (ActionNet's item_rep)
    if (bf16)
      hipLaunchKernelGGL((action_fwd_kernel<LT, true, true, __hip_bfloat16>), grid, block, lds, p.stream, p.a);
    else
      hipLaunchKernelGGL((action_fwd_kernel<LT, true, true, float>), grid, block, lds, p.stream, p.a);
  } else if (shared) {
    if (bf16)
      hipLaunchKernelGGL((action_fwd_kernel<LT, false, true, __hip_bfloat16>), grid, block, lds, p.stream, p.a);
    else
      hipLaunchKernelGGL((action_fwd_kernel<LT, false, true, float>), grid, block, lds, p.stream, p.a);
  } else {
    if (bf16) {
      set_error("bf16 output needs a shared spectrum");
      return LV_ERR_ARG;
    }
    hipLaunchKernelGGL((action_fwd_kernel<LT, false, false, float>), grid, block, lds, p.stream, p.a);
  }
  LV_RETURN_LAUNCH("action_fwd_kernel");
}

// Offset of block l in the packed row: sum_{k<l} (2k+1)^2.
__host__ __device__ constexpr int wigner_block_off(int l) { return l * (2 * l - 1) * (2 * l + 1) / 3; }
constexpr int kWigThreads = 256;

struct WigLaunch {
  const float* ang;
  float* D;
  int64_t n;
  int64_t pitch;  // floats per sample of D
  bool packed;    // block l at wigner_block_off(l) of the row, else at 0
  hipStream_t stream;
};

template <int l>
struct WigLauncher {
  static int run(WigLaunch& p);
};
template <int l>
int WigLauncher<l>::run(WigLaunch& p) {
  const int64_t total = p.n * (2 * l + 1);
  hipLaunchKernelGGL((wigner_d_kernel<l>), dim3(ceil_div(total, kWigThreads)), dim3(kWigThreads), 0,
                     p.stream, p.ang, p.D, p.n, p.pitch, p.packed ? wigner_block_off(l) : 0);
  LV_RETURN_LAUNCH("wigner_d_kernel");
}

#define LV_EXTERN_LAUNCHERS(L)            \
  extern template struct FwdLauncher<L>;  \
  extern template struct WigLauncher<L>;

}  // namespace lv
