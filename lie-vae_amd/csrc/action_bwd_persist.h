#pragma once
// Persistent group-action backward for large batches (compile-time C = 10, shared spectrum,
// kBwdPersistWaves - 1 <= l_max <= kBwdPersistMaxL): the reference's autograd through
// lie_tools.py:211-253 (wigner_d_matrix, block_wigner_matrix_multiply) for the training
// direction.
//
// The one-group tile kernel (action_bwd.h) runs one 6-sample group per block, so every
// block pays its whole phase chain -- gradient-tile load, prologue, chain, per-group dF slab
// pass, angle barrier -- back to back, and writes one 4.8 KB dF slab per 6 samples (a
// third of the gradient tile's bytes again at l = 10, read back by the reduce).  Beyond
// 4,096 groups the grid was capped and blocks looped over groups in a 256-VGPR build.
//
// Here a grid of 3 blocks per CU (3 waves per SIMD) walks the groups (block b: groups b,
// b + P, b + 2P, ...):
//   * each wave adds its degrees' dF rows, summed over the group's samples, into the
//     block's LDS slab (its own rows only: no race); the slab leaves once per block;
//   * every lane leaves its three angle partials in LDS; a barrier publishes them and frees
//     the gradient tile, which then takes the next group by buffer loads to LDS (no VGPR
//     holds it in flight);
//   * under that DMA wave 0 sums the group's angle gradients and the last wave fills the
//     next group's multiples (sincos of the stored angle, one (sample, slot) per lane; the
//     angle loads issued at the top of the group) into the second of two tables; a second
//     barrier ends the group.
// The chain itself (P1..P4 forward recompute, Q4..dF transposed chain, angle gradients as
// <Q4, K P4>, <Q2, K P2>, <dF, K F>) is the one-group kernel's JIT chain, operation for
// operation.  Summation orders are fixed by the plan (degree set per wave, groups per
// block): reproducible bit for bit, and within fp32 rounding of the one-group kernel.
// The angle gradient goes to a.gang (the caller's, or a workspace region for the fused
// exp -> ZYZ VJP, which the host then runs beside the dF reduce, in
// action_bwd_reduce5_vjp_kernel).
// The variants measured against this one (double-buffered tile, padded tile, lane map,
// cross-lane angle tree, ...) are listed in DESIGN.md, "retired backward variants".
// Included by action_bwd.h after the one-group kernel and its helpers.

namespace lv {

constexpr int kBwdPersistMaxL = 10;
constexpr int kBwdPersistWaves = 4;        // degree-set waves per block
constexpr int kBwdPersistBlocksPerCU = 3;  // one gradient-tile buffer, 3 waves per SIMD

// LDS floats of the persistent kernel: the gradient tile, 2 multiples tables, 2
// angle-partial buffers, the dF slab and the spectrum.
// Samples of the gradient tile sit M*C floats apart in LDS, exactly as in global memory, so
// one DMA instruction moves 1 KiB of any sample(s) and the tile takes ~29 of them, spread
// evenly over the waves.
__host__ __device__ constexpr int persist_tile_floats(int L) {
  return (((64 / 10) * (L + 1) * (L + 1) * 10 * 4 + 16 + 15) & ~15) / 4;
}
__host__ __device__ constexpr int persist_lds_floats(int L, int NW) {
  return persist_tile_floats(L) + 2 * (64 / 10) * trig_row_floats(L) + 2 * 3 * (NW * 64 + 4) +
         2 * ((((L + 1) * (L + 1) * 10) + 3) & ~3);
}

template <int LT, int NW>
__global__ __launch_bounds__(64 * NW) __attribute__((amdgpu_waves_per_eu(3)))
void action_bwd_persist_kernel(ActionBwdArgs a) {
  constexpr int C = kTileFastC;
  constexpr int Sw = 64 / C;
  constexpr int MC = (LT + 1) * (LT + 1) * C;
  constexpr int MC4 = (MC + 3) & ~3;
  constexpr int kRow = TrigLds<LT>::kRow;
  constexpr int kTile = persist_tile_floats(LT);
  constexpr int kTrig = Sw * kRow;
  // angle partials per buffer: three planes [wave][lane] kPl floats apart -- 4 floats more
  // than a plane, so that the summing lanes' 8-byte reads of the three planes fall in
  // distinct banks
  constexpr int kPl = NW * 64 + 4;
  constexpr int kAp = 3 * kPl;
  constexpr int nthr = 64 * NW;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* const tile = lds;                  // [kTile]
  float* const trig = tile + kTile;         // [2][Sw][kRow]
  float* const apart = trig + 2 * kTrig;    // [2][3][kPl]
  float* const slab = apart + 2 * kAp;      // [MC4]
  float* const Fsp = slab + MC4;            // [MC4], row-major (M, C)

  const int tid = (int)threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int j = lane / C;
  const int c = lane - j * C;
  const unsigned dmask = a.seg_mask[wave];
  const int64_t P = gridDim.x;
  const int64_t groups = a.groups;
  const int64_t n = a.n;
  // prologue task of this thread: task t = (sample, slot) on lane t of the last wave
  const int t_fill = wave == NW - 1 ? lane : 64;
  const bool task = t_fill < 3 * Sw;
  const int jt = t_fill / 3, q = t_fill - 3 * (t_fill / 3);
  // A/B timeline (LV_STAMPS=1): phase stamps of the block's 5th group (steady state)
  auto st = [&](int kk, int ph) {
    if (kk == 4 && a.stamps) phase_stamp(a.stamps, wave, ph);
  };
  // all groups' tiles sit at the same offset mod 16 (Sw * MC * 4 = 29,040 B at l = 10)
  const int mis = (int)(reinterpret_cast<uintptr_t>(a.gout) & 15);
  char* const stage_b = reinterpret_cast<char*>(tile) + mis;

  // the group's gradient tile, global -> LDS by buffer loads to LDS (buffer_load_dwordx4 ...
  // lds): 16-byte pieces (1 KiB per wave instruction) spread over the waves, 4-byte head /
  // tail pieces.  The group's rows are a buffer resource, each lane's byte offset is fixed for
  // the whole walk and the round's offset sits in an SGPR, so a full round costs no VALU
  // (global_load_lds needs a 64-bit VGPR address per lane); only the last, partial round
  // keeps a per-lane bound.
  auto issue_tile = [&](int64_t g) {
    const int64_t s0 = g * Sw;
    const int Sv = (int)min((int64_t)Sw, n - s0);
    const int nbytes = Sv * MC * 4;
    const char* gb = reinterpret_cast<const char*>(a.gout + s0 * MC);
    const int head = min((16 - mis) & 15, nbytes);
    const int nvec = (nbytes - head) >> 4;
    const int tail0 = head + nvec * 16;
    const __amdgpu_buffer_rsrc_t rs =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(gb), 0, nbytes, kRawBufferFlags);
    const int vo = head + 16 * (wave * 64 + lane);  // this lane's piece in round 0
    char* const ldsw = stage_b + head + 16 * (wave * 64);
    const int nfull = nvec / nthr;  // rounds in which every lane of every wave has a piece
    for (int it = 0; it < nfull; ++it)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, as_lds(ldsw + it * nthr * 16), 16, vo, it * nthr * 16, 0, 0);
    if (nfull * nthr + wave * 64 + lane < nvec)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, as_lds(ldsw + nfull * nthr * 16), 16, vo, nfull * nthr * 16, 0, 0);
    if (wave == NW - 1) {
      if (4 * lane < head) __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, as_lds(stage_b), 4, 4 * lane, 0, 0, 0);
      if (tail0 + 4 * lane < nbytes)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, as_lds(stage_b + tail0), 4, 4 * lane, tail0, 0, 0);
    }
  };
  // the stored angle a task's slot uses (transpose: slot q takes angle 2 - q)
  auto task_angle = [&](int64_t g) -> float {
    const int64_t s0 = g * Sw;
    const int Sv = (int)min((int64_t)Sw, n - s0);
    return a.ang[(s0 + min(jt, Sv - 1)) * 3 + (a.transpose ? 2 - q : q)];
  };
  auto task_fill = [&](float ang, int buf) {
    // straight-line sincos (Cody-Waite + minimax, <= 1.6 ulp; action_common.h): the
    // library sincosf's range-reduction branches sat on every group's prologue path
    float cq, sq;
    lv_sincos(ang, sq, cq);
    if (a.transpose) sq = -sq;
    trig_row_fill1<LT>(trig + buf * kTrig + jt * kRow, cq, sq, q, LT);
  };

  int64_t g = blockIdx.x;
  // ---- first group: its tile, its multiples; the spectrum; the zeroed slab
  float ang_next = 0.f;
  if (task) ang_next = task_angle(g);
  issue_tile(g);
  {
    constexpr int kFPer = (MC + nthr - 1) / nthr;
    float fv[kFPer];
#pragma unroll
    for (int k = 0; k < kFPer; ++k) {
      const int e = tid + nthr * k;
      fv[k] = e < MC ? a.F[e] : 0.f;
    }
#pragma unroll
    for (int k = 0; k < kFPer; ++k) {
      const int e = tid + nthr * k;
      if (e < MC) {
        Fsp[e] = fv[k];
        slab[e] = 0.f;
      }
    }
  }
  if (task) task_fill(ang_next, 0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  block_sync_lds();

  const float* Fl = Fsp + c;
  // the flat slab pass (step 3): this wave's element pairs, the tile's 8-byte alignment
  constexpr int kPR = 3;
  int npairs = 0;
  for (unsigned m = dmask; m; m &= m - 1) npairs += 5 * (2 * __builtin_ctz(m) + 1);
  const bool pair_ok = (mis & 7) == 0 && npairs <= 64 * kPR;
  // this lane's pair offsets in the wave's rows (-1: none), fixed for the whole walk
  int poff[kPR];
#pragma unroll
  for (int uu = 0; uu < kPR; ++uu) {
    const int pp = lane + 64 * uu;
    int o = 0, acc = 0;
    for (unsigned m = dmask; m; m &= m - 1) {
      const int l = __builtin_ctz(m);
      const int np = 5 * (2 * l + 1);
      if (pp >= acc && pp < acc + np) o = l * l * C + 2 * (pp - acc);
      acc += np;
    }
    poff[uu] = pp < npairs ? o : -1;
  }
  for (int k = 0; g < groups; ++k, g += P) {
    const int cur = k & 1, nxt = cur ^ 1;
    const int64_t gn = g + P;
    const bool has_next = gn < groups;
    st(k, 0);
    // 1. next group's angle loads (task lanes); the tile is refilled after this group's
    //    barrier (step 5)
    if (task && has_next) ang_next = task_angle(gn);

    // 2. this group's chain over the wave's degrees, largest first
    const int64_t s0 = g * Sw;
    const int Sv = (int)min((int64_t)Sw, n - s0);
    const bool active = j < Sv;
    float* tile_lane = reinterpret_cast<float*>(stage_b) + j * MC + c;
    const float* t0 = reinterpret_cast<const float*>(stage_b);
    const float* tj = trig + cur * kTrig + min(j, Sw - 1) * kRow;
    float ga = 0.f, gb = 0.f, gc = 0.f;
    sfor<LT + 1>([&](auto Lc) {
      constexpr int l = LT - LV_CV(Lc);
      if ((dmask >> l) & 1u) {
        constexpr int nn = 2 * l + 1;
        constexpr int r0 = l * l;
        float p2[nn], p4[nn], u[nn];
        const float* fcol = Fl + r0 * C;
        xm_mem<l, false>(mult_lds<l, 2, LT>(tj), fcol, C, u);              // P1
        jmul<l>(u, p2);                                                    // P2
        xm<l>(mult_lds<l, 1, LT>(tj), p2, u);                              // P3
        jmul<l>(u, p4);                                                    // P4
        xm_mem<l, true>(mult_lds<l, 0, LT>(tj), tile_lane + r0 * C, C, u);  // Q4
        ga += kdot<l>(u, p4);
        jmul<l>(u, p4);                                                    // Q3
        xm_t<l>(mult_lds<l, 1, LT>(tj), p4, u);                            // Q2
        gb += kdot<l>(u, p2);
        jmul<l>(u, p2);                                                    // Q1
        xm_t<l>(mult_lds<l, 2, LT>(tj), p2, u);                            // dF column
        gc += kdot_mem<l>(u, fcol, C);
        if (active) sfor<nn>([&](auto I) { tile_lane[(r0 + LV_CV(I)) * C] = u[LV_CV(I)]; });
      }
    });
    st(k, 1);
    // 3. this wave's dF rows summed over the group's samples (sample order), added to the
    //    block's slab (groups in the block's order)
    wave_lds_sync();
    if (pair_ok && Sv == Sw) {
      // full group, 8-byte aligned tile: the wave's rows as ONE flat list of element pairs
      // (a degree's 10 (2l+1) elements are whole pairs), up to kPR rounds of 64 pairs with
      // every 8-byte load issued before any sum: one LDS round trip for the loads, one for
      // the slab's read-modify-write (the per-degree passes took 3-6)
      typedef float f2 __attribute__((ext_vector_type(2)));
      f2 v[kPR][Sw];
      const int* off = poff;
#pragma unroll
      for (int uu = 0; uu < kPR; ++uu) {
#pragma unroll
        for (int jj = 0; jj < Sw; ++jj)
          v[uu][jj] = *reinterpret_cast<const f2*>(t0 + jj * MC + (off[uu] < 0 ? 0 : off[uu]));
      }
#pragma unroll
      for (int uu = 0; uu < kPR; ++uu) {
        f2 sum = v[uu][0];
#pragma unroll
        for (int jj = 1; jj < Sw; ++jj) sum += v[uu][jj];
        if (off[uu] >= 0) *reinterpret_cast<f2*>(slab + off[uu]) += sum;
      }
    } else {
      for (unsigned m = dmask; m; m &= m - 1) {
        const int l = __builtin_ctz(m);
        const int base = l * l * C, cnt = (2 * l + 1) * C;
        if (Sv == Sw) {
          constexpr int kU = 4;
          for (int e0 = lane; e0 < cnt; e0 += kU * 64) {
            float v[kU][Sw];
#pragma unroll
            for (int uu = 0; uu < kU; ++uu) {
              const int e = base + min(e0 + 64 * uu, cnt - 1);
#pragma unroll
              for (int jj = 0; jj < Sw; ++jj) v[uu][jj] = t0[jj * MC + e];
            }
#pragma unroll
            for (int uu = 0; uu < kU; ++uu) {
              float sum = v[uu][0];
#pragma unroll
              for (int jj = 1; jj < Sw; ++jj) sum += v[uu][jj];
              if (e0 + 64 * uu < cnt) slab[base + e0 + 64 * uu] += sum;
            }
          }
        } else {
          for (int e = lane; e < cnt; e += 64) {
            float sum = t0[base + e];
            for (int jj = 1; jj < Sv; ++jj) sum += t0[jj * MC + base + e];
            slab[base + e] += sum;
          }
        }
      }
    }
    st(k, 2);
    // 4. angle partials: every lane's three straight to the buffer, [angle][wave][lane]
    {
      float* ap = apart + cur * kAp + wave * 64 + (j * C + c);  // [angle][wave][sample][column]
      ap[0] = ga;
      ap[kPl] = gb;
      ap[2 * kPl] = gc;
    }
    st(k, 3);
    block_sync_lds();
    st(k, 4);
    // 5. every wave is past this group's chain and slab pass: the tile takes the next group
    //    now, and the angle sums and the next multiples run under its DMA
    if (has_next) issue_tile(gn);
    // 6. the group's angle gradients: output t = (sample, angle) on lane t of wave 0, its 4
    //    waves x 10 columns of partials read as 8-byte pairs, summed column-pairwise then
    //    over the waves (waves in order)
    if (wave == 0 && lane < 3 * Sv) {
      const int js = lane / 3, i = lane - 3 * (lane / 3);
      // transpose: angle i is the negated sum of stored component 2 - i
      const int ci = a.transpose ? 2 - i : i;
      typedef float f2 __attribute__((ext_vector_type(2)));
      const float* apc = apart + cur * kAp + ci * kPl + js * C;
      f2 pv[NW][C / 2];
#pragma unroll
      for (int w = 0; w < NW; ++w)
#pragma unroll
        for (int k2 = 0; k2 < C / 2; ++k2) pv[w][k2] = *reinterpret_cast<const f2*>(apc + w * 64 + 2 * k2);
      float r = 0.f;
#pragma unroll
      for (int w = 0; w < NW; ++w) {
        f2 t = pv[w][0];
#pragma unroll
        for (int k2 = 1; k2 < C / 2; ++k2) t += pv[w][k2];
        r += t[0] + t[1];
      }
      a.gang[(s0 + js) * 3 + i] = a.transpose ? -r : r;
    }
    // 7. the next group's multiples (its angles have long landed), then its tile
    if (has_next) {
      if (task) task_fill(ang_next, nxt);
      st(k, 5);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      st(k, 6);
      block_sync_lds();
      st(k, 7);
    }
  }
  // ---- the block's slab to the workspace, chunk-major: whole 16-byte pieces with
  // write-through (sc1) buffer stores after one block barrier (4-byte stores left the lines
  // dirty in the XCD's L2 for the end-of-kernel write-back)
  block_sync_lds();  // every wave's slab rows are final
  typedef float f4 __attribute__((ext_vector_type(4)));
  const int nch = (MC + kSlabChunk - 1) / kSlabChunk;
  const __amdgpu_buffer_rsrc_t rw =
      __builtin_amdgcn_make_buffer_rsrc(a.ws_F, 0, nch * (int)gridDim.x * kSlabChunk * 4, kRawBufferFlags);
  // piece (chunk q, quarter k): slab[16 q + 4 k ..] -> ws_F[q * grid * 16 + block * 16 + 4 k ..]
  // (the last chunk's pad reads the next LDS floats: summed by reduce5, never stored to gF)
  for (int pc = tid; pc < 4 * nch; pc += nthr) {
    const int q4 = pc >> 2, k4 = pc & 3;
    const f4 v = *reinterpret_cast<const f4*>(slab + kSlabChunk * q4 + 4 * k4);
    __builtin_amdgcn_raw_buffer_store_b128(v, rw, ((q4 * (int)gridDim.x + (int)blockIdx.x) * kSlabChunk + 4 * k4) * 4,
                                           0, 16);
  }
}

}  // namespace lv
