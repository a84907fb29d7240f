// K1 on the bf16 matrix pipe: fp32 second moments from TWO bf16 planes ("bf16 split-accumulate ... only if
// it holds the 1e-3 bar").
//
//   d = fl32(x - p)            p: the launch's pilot, subtracted once, undone in fp64 (k_pilot_fixup).  Near the column mean and COARSE:
//                              for float32 columns that lie on a grid the mean of a row sample rounded to 2^(ilogb(sd) - 3)
//                              (gram.hip k_sample_grid, k_pilot_coarse; every other float32 column: the sample mean), for half
//                              rows a point of their own grid (k_pilot_on_grid) -- x - p then keeps the grid of grid-valued
//                              columns (0/1, one-hot, pixels, counts, integers), hi holds it exactly and mid = 0
//   d = hi + mid + lo          hi = bf16(d), mid = bf16(d - hi)  (d - hi is exact in fp32), |mid| <= 2^-8 |d|, |lo| <= 2^-16 |d|
//   d_i d_j = hi_i hi_j + hi_i mid_j + mid_i hi_j  [+ mid_i mid_j + hi_i lo_j + lo_i hi_j + ...]
//
// The three kept products run as THREE MFMAs into ONE fp32 accumulator per k-step (operand sequences (H, H, M) x (H, M, H)),
// so an output tile needs no symmetrisation pass and costs 3 bf16 MFMAs per fp32 one it replaces -- at 16x the fp32 MFMA
// rate.  Of the dropped terms only mid_i mid_i on the DIAGONAL is systematic (a sum of squares); it is added back exactly
// from sum_k mid_ik^2, which the split pass accumulates on the side.  The rest are zero-mean at 2^-16 per product and
// average out over the rows like the fp32 kernel's own accumulation error (measured in bench.py: k1_rel_err of both routes).
// Accumulation is unchanged from the fp32 kernel: fp32 inside a row chunk (<= 16384 rows), fp64 across chunks.
// A DELIBERATE DIFFERENCE from float64 moments: sum mid^2 is added where i == j in G only (k_split_reduce).  Two IDENTICAL columns
// at different positions -- a view passed twice, columns shared between views -- give an off-diagonal entry whose dropped
// sum_k mid_ki mid_kj is the same sum of squares, and that entry lacks it: about 3e-6 of the entry, flat in the row count (rCCA on
// [X, X]: canonical correlations of 1 - 2.5e-6).  Heavy-tailed rows (Student-t, one row at 1e4 sigma) and an input whose period
// matches the pilot sample's stride keep errors of that order too.  tests/split_emulation.py restates this arithmetic on the host;
// tests/test_gpu_k1_split_structured.py holds the kernels to it: bit for bit on grid-valued inputs, within the float32 accumulation
// allowance elsewhere, these pinned effects included.
//
// Data layout.  The MFMA operand of v_mfma_f32_32x32x16_bf16 is 8 consecutive k (= ROWS of a view) of one column per lane,
// which row-major views cannot deliver coalesced -- so the split pass also transposes, into the exact LDS image the Gram
// kernel wants:  planes[panel p][k-step s][plane H|M][column tile t: 8][k half h: 2][column c: 32][k: 8]  (bf16), i.e. one
// panel (256 columns) x one k-step (16 rows) = 16 KiB, and every 1 KiB run of it is one MFMA operand of one wave
// (lane l = (h, c) holds its 16 bytes).  The Gram kernel streams those runs with buffer_load ... lds (LDS-DMA: lane-linear
// image, no VGPRs, no ds_write) and reads them back with conflict-free ds_read_b128 -- no address arithmetic anywhere.
// Views are padded per view to whole panels and the rows to whole k-steps with zeros (d = 0, not x - p), so every tile is
// a full tile: ragged widths, unaligned rows and odd leading dimensions all take this one path.
//
// Gram kernel: 256 x 256 output tile per workgroup, 4 waves (2 x 2) of 128 x 128 = 4 x 4 MFMA tiles, one wave per SIMD
// (256 accumulator registers).  LDS: a 4-slot ring of k-steps (32 KiB each: A panel H|M, B panel H|M); each wave DMAs a
// quarter of every slot.  One barrier per k-step: wave-side `s_waitcnt vmcnt(16)` (its own DMAs of step s + 1 have landed)
// -> s_barrier (everybody's have; everybody has finished reading slot s) -> DMA of step s + 4 into slot s -> fragments of
// step s + 1 from LDS while the 48 MFMAs of step s run.  Three k-steps of loads are always in flight.
//
// Output: per (row chunk, tile) fp32 partial tiles with plain 16-byte stores (no atomics); k_split_reduce adds the chunks
// up in fp64 into G and applies the diagonal correction.  The loss fast path (gram_partials_split_f32) hands the partial
// tiles to loss.hip's preparation kernel instead.  The split pass also gathers the exact fp64 column sums of x (the means; s of
// the pilot fix-up), so the route reads the rows once.  Panel / tile tables hold no pointers and are cached with the handle.
//
// Roofline: executed flops = 3 x n Dp (Dp + 256) on the bf16 pipe (2.5 PF dense peak); algorithmic F = n D (D + 1).
#include <algorithm>
#include <vector>

#include "hip_common.h"
#include "half_cvt.h"
#include "gram_map.h"
#include "split_mma.h"

namespace ccz {

typedef unsigned int sp_v2u32 __attribute__((ext_vector_type(2)));   // four 2-byte elements of a half row

constexpr int SP_MAXV = 16;         // views per launch (their base pointers travel as a kernel argument, the tables hold no pointers)

struct SplitPanel {
  int32_t view;          // which view
  int32_t col0;          // first column of the panel in its view
  int32_t width;         // valid columns (<= 256); the rest of the panel is zero
  int32_t gcol0;         // column of G (and of pilot / msq) of the panel's first column
};

struct SplitViews {
  const void* data[SP_MAXV];       // rows of the launch's input type (float, or a 2-byte format widened on load)
  int64_t ld[SP_MAXV];
};

struct SplitTile {
  int32_t pa, pb;        // panels (pa <= pb)
  int32_t out_row, out_col;
  int32_t wa, wb;
  int32_t diag;
  int32_t pad_;
};

// ---------------------------------------------------------------------------
// split pass: rows [r0, r0 + nrows) of every view -> the two bf16 planes of this launch (k-steps [0, ksteps)),
// and msq[j] += sum_k mid_kj^2.  grid = (row blocks of rb <= SP_RB rows, panels).  A thread owns 4 consecutive columns and, per
// pass, the 8 rows of one k half: its 8 float4 loads are one 1 KiB-per-wave row segment each, its stores 64 contiguous
// bytes per plane.  HBM-bound: 4 bytes in, 4 bytes out per element.
// T = float, or bf16_t / f16_t (half_cvt.h): the same thread then loads 8 bytes per row and widens them exactly -- 2 bytes in,
// 4 out, no float32 copy of the view anywhere; everything after the load is the float32 code.  ALIGNED: every row of every view
// starts on a 4-element boundary (16 bytes of float, 8 bytes of a half type) and whole 4-column groups are in or out.
// ---------------------------------------------------------------------------
__device__ __forceinline__ void sp_wave_lds_sync() {    // lanes of ONE wave exchange data through LDS (see cholinv.hip::wave_lds_sync)
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// The piece exchange: the 64 bytes a thread produces per plane are FOUR 16-byte pieces of a 512-byte run, so storing them as they
// are makes every wave-level store 64 separate 16-byte writes at a stride of 64 bytes -- the PMC pass over that first form
// (profiles/r06_split_pass_pmc_raw.md) counts 6.05e8 L2 requests per 262144 rows, 5.4e8 of them these partial writes, i.e. 80
// requests per clock on 128 L2 channels.  So the eight lanes of a column tile swap pieces through a wave-private 4 KB of LDS
// (no workgroup barrier) until store e of lane j is piece 8 e + j: every wave-level store is eight whole 128-byte lines
// (2.03e8 L2 requests per 262144 rows; the pass at the metric shape 14.0 -> 12.4 ms).
template <typename T, bool ALIGNED>
__global__ __launch_bounds__(256) void k_split_bf16x2(const SplitPanel* __restrict__ panels, SplitViews vws, int64_t r0, int64_t nrows, int64_t ksteps,
                                                      const float* __restrict__ pilot, char* __restrict__ planes,
                                                      double* __restrict__ msq, double* __restrict__ csum, int rb, int panel_fast) {
  __shared__ float red[4][256];
  __shared__ double redc[4][256];
  __shared__ sp_v4u32 xch[4][256];                          // per wave: 8 column tiles x 32 pieces of 16 bytes (one plane, one k half)
  // panel_fast: consecutive workgroups take the panels of ONE row block (together they read whole rows) instead of the row blocks
  // of one panel (a 1 KiB stripe of every 16 KiB row: the same few HBM channels for everybody) -- CCZ_SPLIT_ORDER
  const unsigned pidx = panel_fast ? blockIdx.x : blockIdx.y, ridx = panel_fast ? blockIdx.y : blockIdx.x;
  const SplitPanel pn = panels[pidx];
  const int tid = threadIdx.x, cg = tid & 63, rg = tid >> 6;
  const int64_t rows_pad = ksteps * SP_K;
  const int64_t rb0 = int64_t(ridx) * rb;                   // rb rows per workgroup (a multiple of 32, <= SP_RB)
  const int c0 = 4 * cg;
  sp_v4f32 p = {0.f, 0.f, 0.f, 0.f};
  bool cok[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    cok[e] = c0 + e < pn.width;
    if (pilot && cok[e]) p[e] = pilot[pn.gcol0 + c0 + e];
  }
  const T* __restrict__ X = static_cast<const T*>(vws.data[pn.view]) + pn.col0 + c0;
  const int64_t pld = vws.ld[pn.view];
  char* out = planes + int64_t(pidx) * ksteps * SP_PSTEP + (cg >> 3) * 1024 + (cg & 7) * 64;
  sp_v4f32 q = {0.f, 0.f, 0.f, 0.f};
  double cs[4] = {0.0, 0.0, 0.0, 0.0};               // exact column sums of x (not of x - p): the means, and the pilot fix-up's s
  for (int pass = 0; pass < rb / 32; ++pass) {
    const int64_t row = rb0 + pass * 32 + rg * 8;          // first of this thread's 8 rows (within the launch)
    if (row >= rows_pad) break;
    sp_v4f32 v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const bool rok = row + k < nrows;
      const T* src = X + (r0 + (rok ? row + k : 0)) * pld;
      if (ALIGNED) {
        v[k] = p;                                          // (whole 4-column groups are inside or outside the panel's width)
        if constexpr (sizeof(T) == 4) {
          if (cok[0]) v[k] = __builtin_nontemporal_load(reinterpret_cast<const sp_v4f32*>(src));   // read once: keep L2 / MALL for the planes
        } else if (cok[0]) {
          const sp_v2u32 w = __builtin_nontemporal_load(reinterpret_cast<const sp_v2u32*>(src));   // 4 elements of 2 bytes
#pragma unroll
          for (int e = 0; e < 4; ++e) v[k][e] = widen(T{uint16_t(w[e >> 1] >> (16 * (e & 1)))});
        }
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[k][e] = cok[e] ? widen(src[e]) : 0.f;
      }
      if (!rok) v[k] = p;                                  // d = 0 exactly for the rows that pad the last k-step
      else if (csum) {
#pragma unroll
        for (int e = 0; e < 4; ++e) cs[e] += cok[e] ? double(v[k][e]) : 0.0;
      }
    }
    sp_v4u32 hw[4], mw[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float d[8], m[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) d[k] = cok[e] ? v[k][e] - p[e] : 0.f;
#pragma unroll
      for (int k = 0; k < 8; k += 2) {
        const unsigned hb = sp_pack2(d[k], d[k + 1]);
        hw[e][k >> 1] = hb;
        m[k] = d[k] - __builtin_bit_cast(float, hb << 16);            // exact: hi shares d's leading bits
        m[k + 1] = d[k + 1] - __builtin_bit_cast(float, hb & 0xffff0000u);
        const unsigned mb = sp_pack2(m[k], m[k + 1]);
        mw[e][k >> 1] = mb;
        const float m0 = __builtin_bit_cast(float, mb << 16), m1 = __builtin_bit_cast(float, mb & 0xffff0000u);
        q[e] += m0 * m0 + m1 * m1;
      }
    }
    char* dst = out + (row >> 4) * SP_PSTEP + ((row >> 3) & 1) * 512;
    // piece (tile t, column c) sits at xw[32 t + (c ^ ((c >> 3) & 3) ^ ((t & 1) << 3))]: the 8 lanes of a ds_write_b128 group
    // (c = 4 j + e) then cover all eight 16-byte bank quads, and the 16 lanes of a ds_read_b128 group (c = 8 e + j over four
    // tiles) all sixteen of a 256-byte row (MI355X_MICROARCH.md, LDS service groups) -- plain [32 t + c] is 4-way / 2-way
    sp_v4u32* xw = xch[rg];
    char* dst2 = dst - (cg & 7) * 48;                                // tile base + (cg & 7) * 16
    const int t8 = ((cg >> 3) & 1) << 3, j = cg & 7;
    const int wr = (cg >> 3) * 32 + ((4 * j) ^ t8), wx = j >> 1;     // + (e ^ wx)
    const int rd = (cg >> 3) * 32;                                   // + ((8 e) ^ t8) + (j ^ e)
    sp_wave_lds_sync();                                              // the previous pass's reads are done
#pragma unroll
    for (int e = 0; e < 4; ++e) xw[wr + (e ^ wx)] = hw[e];
    sp_wave_lds_sync();
#pragma unroll
    for (int e = 0; e < 4; ++e) hw[e] = xw[rd + ((8 * e) ^ t8) + (j ^ e)];
    sp_wave_lds_sync();
#pragma unroll
    for (int e = 0; e < 4; ++e) xw[wr + (e ^ wx)] = mw[e];
    sp_wave_lds_sync();
#pragma unroll
    for (int e = 0; e < 4; ++e) mw[e] = xw[rd + ((8 * e) ^ t8) + (j ^ e)];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      *reinterpret_cast<sp_v4u32*>(dst2 + e * 128) = hw[e];            // (plain stores: non-temporal ones made this pass 3.5x slower)
      *reinterpret_cast<sp_v4u32*>(dst2 + SP_PLANE + e * 128) = mw[e];
    }
  }
  // msq: the four row groups of the workgroup -> one fp64 atomic per column
#pragma unroll
  for (int e = 0; e < 4; ++e) red[rg][c0 + e] = q[e];
  if (csum) {
#pragma unroll
    for (int e = 0; e < 4; ++e) redc[rg][c0 + e] = cs[e];
  }
  __syncthreads();
  if (msq && tid < pn.width) {
    const double s = double(red[0][tid]) + double(red[1][tid]) + double(red[2][tid]) + double(red[3][tid]);
    unsafeAtomicAdd(msq + pn.gcol0 + tid, s);
  }
  if (csum && tid < pn.width) unsafeAtomicAdd(csum + pn.gcol0 + tid, (redc[0][tid] + redc[1][tid]) + (redc[2][tid] + redc[3][tid]));
}

// ---------------------------------------------------------------------------
// Gram kernel
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256, 1) void k_gram_bf16x2(const SplitTile* __restrict__ tiles, int ntiles, int per_xcd, int64_t ksplit,
                                                        const char* __restrict__ planes, int64_t ksteps, int64_t steps_per_wg,
                                                        float* __restrict__ partial) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const WorkItem wi = locate_work(blockIdx.x, ntiles, per_xcd, ksplit);
  if (!wi.valid) return;
  const SplitTile t = tiles[wi.tile];
  const int64_t s0 = wi.chunk * steps_per_wg;
  const int64_t s1 = min(ksteps, s0 + steps_per_wg);
  if (s0 >= s1) return;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wave >> 1, wc = wave & 1;

  sp_v16f32 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
  const char* srcA = planes + (int64_t(t.pa) * ksteps + s0) * SP_PSTEP;
  const char* srcB = planes + (int64_t(t.pb) * ksteps + s0) * SP_PSTEP;
  const int nsteps = int(s1 - s0);
  // a diagonal tile (A side == B side): the two symmetric quadrants compute their upper MFMA tiles, and the wave of the
  // redundant quadrant (1, 0) takes the lower half of quadrant (0, 1) -- 30 MFMAs per k-step for the slowest wave instead of 48.
  // What is not computed lies below the diagonal of G and is never read (k_split_reduce skips it).
  int qr = wr, qc = wc, ti0 = 0, ti1 = 4;
  bool sym = false;
  if (t.diag && wr == wc) {
    sym = true;
    split_mma_core<1>(acc, smem, srcA, srcB, nsteps, wave, lane, qr, qc);
  } else if (t.diag && wr == 0) {
    ti1 = 2;
    split_mma_core<2>(acc, smem, srcA, srcB, nsteps, wave, lane, qr, qc);
  } else if (t.diag) {
    qr = 0; qc = 1; ti0 = 2;
    split_mma_core<3>(acc, smem, srcA, srcB, nsteps, wave, lane, qr, qc);
  } else {
    split_mma_core<0>(acc, smem, srcA, srcB, nsteps, wave, lane, qr, qc);
  }

  // epilogue: the chunk's fp32 sums -> this (chunk, tile)'s slot, row-major 256 x 256
  float* pt = partial + (wi.chunk * int64_t(ntiles) + wi.tile) * int64_t(SP_T * SP_T);
#pragma unroll
  for (int ti = 0; ti < 4; ++ti) {
    if (ti < ti0 || ti >= ti1) continue;
    float* prow = pt + (qr * 128 + ti * 32 + (lane & 31)) * SP_T + qc * 128 + 4 * (lane >> 5);
#pragma unroll
    for (int tj = 0; tj < 4; ++tj) {
      if (sym && tj < ti) continue;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const sp_v4f32 v = {acc[ti][tj][4 * g], acc[ti][tj][4 * g + 1], acc[ti][tj][4 * g + 2], acc[ti][tj][4 * g + 3]};
        *reinterpret_cast<sp_v4f32*>(prow + tj * 32 + 8 * g) = v;
      }
    }
  }
}

// G (upper tiles) += sum over the row chunks of the fp32 partial tiles, in fp64; diagonal: += sum_k mid^2 (the one dropped
// product that does not average out).  grid = (64, tiles), a thread owns 4 consecutive elements of a tile row.
__global__ __launch_bounds__(256) void k_split_reduce(const float* __restrict__ partial, const SplitTile* __restrict__ tiles, int ntiles,
                                                      int64_t ksplit, double* __restrict__ G, int64_t ldg, const double* __restrict__ msq) {
  const int tile = blockIdx.y;
  const SplitTile t = tiles[tile];
  const int e = (blockIdx.x * 256 + threadIdx.x) * 4;
  const int i = e >> 8, j = e & 255;
  if (i >= t.wa || j >= t.wb) return;
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
  const float* p = partial + int64_t(tile) * (SP_T * SP_T) + e;
  const int64_t stride = int64_t(ntiles) * (SP_T * SP_T);
  for (int64_t c = 0; c < ksplit; ++c) {
    const sp_v4f32 v = __builtin_nontemporal_load(reinterpret_cast<const sp_v4f32*>(p + c * stride));   // read once
    a0 += double(v[0]); a1 += double(v[1]); a2 += double(v[2]); a3 += double(v[3]);
  }
  const double a[4] = {a0, a1, a2, a3};
  double* g = G + (int64_t(t.out_row) + i) * ldg + t.out_col + j;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    if (j + q >= t.wb) break;
    if (t.diag && j + q < i) continue;          // below the diagonal of G: not authoritative anywhere (the pilot fix-up skips it too)
    double v = a[q];
    if (t.diag && i == j + q) v += msq[t.out_row + i];
    g[q] += v;
  }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
namespace {

// (i, j) panel pairs, i <= j, in launch order -- the order of gram.hip's tile table: whole 4 x 8 supertiles without a
// diagonal tile first (32 consecutive tiles share 12 panels through an XCD's L2), then the diagonal tiles, then the rest
std::vector<std::pair<int, int>> split_tile_order(int np) {
  std::vector<std::pair<int, int>> full, dg, rest;
  for (int I = 0; I < np; I += 4)
    for (int J = (I / 8) * 8; J < np; J += 8) {
      std::vector<std::pair<int, int>> blk;
      bool has_diag = false;
      for (int i = I; i < std::min(np, I + 4); ++i)
        for (int j = std::max(i, J); j < std::min(np, J + 8); ++j) { blk.emplace_back(i, j); has_diag = has_diag || i == j; }
      for (const auto& ij : blk) {
        if (blk.size() == 32 && !has_diag) full.push_back(ij);
        else (ij.first == ij.second ? dg : rest).push_back(ij);
      }
    }
  full.insert(full.end(), dg.begin(), dg.end());
  full.insert(full.end(), rest.begin(), rest.end());
  return full;
}

}  // namespace

size_t split_scratch_budget(ccz_ctx* c) {
  const double env_gb = env::live(env::SPLIT_SCRATCH_GB);
  const double cap = 0.4 * double(impl(c)->props.totalGlobalMem);
  return size_t(std::max(8.0 * 1048576.0, std::min(env_gb * 1073741824.0, cap)));
}

// rows per workgroup of the split pass: SP_RB on large inputs (fewer atomics), down to 32 so that short inputs (a DCCA batch,
// the Gamma matrix of a backward) still spread over the chip
static int split_rows_per_block(int64_t rows_pad, int64_t npanels, int ncu) {
  int rb = SP_RB;
  while (rb > 32 && ((rows_pad + rb - 1) / rb) * npanels < 2 * int64_t(ncu)) rb /= 2;
  return rb;
}

// Panel and tile tables of a set of view widths, on the device, kept with the handle: they depend on the widths only (the
// views' pointers and strides travel as a kernel argument), so a training loop or a fit loop uploads them once.
struct SplitTables {
  const SplitPanel* panels;
  const SplitTile* tiles;
  const GramTile* gtiles;      // the same tiles for loss.hip's preparation kernel (out_row / out_col / wa / wb / diag; a, b unused)
  int np, ntiles;
};

static SplitTables split_tables(ccz_ctx* c, const int64_t* cols, int n_views) {
  Impl* im = impl(c);
  uint64_t key = 1469598103934665603ull;
  auto mix = [&](uint64_t v) { key ^= v; key *= 1099511628211ull; };
  mix(uint64_t(n_views));
  int np = 0;
  for (int v = 0; v < n_views; ++v) { mix(uint64_t(cols[v])); np += int((cols[v] + SP_T - 1) / SP_T); }
  SplitTables tb;
  tb.np = np;
  for (auto& e : im->split_tabs)
    if (e.key == key && e.np == np) {                   // the hot path: a lookup, no allocation
      tb.panels = static_cast<const SplitPanel*>(e.panels.get());
      tb.tiles = static_cast<const SplitTile*>(e.tiles.get());
      tb.gtiles = static_cast<const GramTile*>(e.gtiles.get());
      tb.ntiles = e.ntiles;
      return tb;
    }
  std::vector<SplitPanel> panels;
  int64_t g0 = 0;
  for (int v = 0; v < n_views; ++v) {
    for (int64_t c0 = 0; c0 < cols[v]; c0 += SP_T)
      panels.push_back(SplitPanel{int32_t(v), int32_t(c0), int32_t(std::min<int64_t>(SP_T, cols[v] - c0)), int32_t(g0 + c0)});
    g0 += cols[v];
  }
  std::vector<SplitTile> tiles;
  std::vector<GramTile> gt;
  for (const auto& ij : split_tile_order(tb.np)) {
    SplitTile t;
    t.pa = ij.first; t.pb = ij.second;
    t.out_row = panels[ij.first].gcol0; t.out_col = panels[ij.second].gcol0;
    t.wa = panels[ij.first].width; t.wb = panels[ij.second].width;
    t.diag = ij.first == ij.second ? 1 : 0;
    t.pad_ = 0;
    tiles.push_back(t);
    GramTile g{};
    g.a = nullptr; g.b = nullptr; g.lda = 0; g.ldb = 0;
    g.out_row = t.out_row; g.out_col = t.out_col; g.wa = t.wa; g.wb = t.wb; g.diag = t.diag; g.pad_ = 0;
    gt.push_back(g);
  }
  tb.ntiles = int(tiles.size());
  if (im->split_tabs.size() >= 32) {                      // a caller cycling through many shapes: start over
    CCZ_HIP(hipStreamSynchronize(stream(c)));
    im->split_tabs.clear();
  }
  DevMem<> dp, dt, dg;
  CCZ_HIP(hipMalloc(dp.out(), std::max<size_t>(panels.size() * sizeof(SplitPanel), 256)));
  CCZ_HIP(hipMalloc(dt.out(), std::max<size_t>(tiles.size() * sizeof(SplitTile), 256)));
  CCZ_HIP(hipMalloc(dg.out(), std::max<size_t>(gt.size() * sizeof(GramTile), 256)));
  h2d_small(c, dp.get(), panels.data(), panels.size() * sizeof(SplitPanel));
  h2d_small(c, dt.get(), tiles.data(), tiles.size() * sizeof(SplitTile));
  h2d_small(c, dg.get(), gt.data(), gt.size() * sizeof(GramTile));
  tb.panels = static_cast<const SplitPanel*>(dp.get());
  tb.tiles = static_cast<const SplitTile*>(dt.get());
  tb.gtiles = static_cast<const GramTile*>(dg.get());
  im->split_tabs.push_back({key, std::move(dp), std::move(dt), std::move(dg), tb.np, tb.ntiles});
  return tb;
}

// (row starts on 4-element boundaries: 16 bytes of float, 8 bytes of a half type)
static bool split_views_arg(const ccz_view* views, int n_views, SplitViews* vws, int dtype = CCZ_F32) {
  bool aligned = true;
  const uintptr_t bytes = dtype == CCZ_F32 ? 16 : 8;
  for (int v = 0; v < n_views; ++v) {
    vws->data[v] = views[v].data;
    vws->ld[v] = views[v].ld;
    if (views[v].cols % 4 != 0 || views[v].ld % 4 != 0 || reinterpret_cast<uintptr_t>(views[v].data) % bytes != 0) aligned = false;
  }
  return aligned;
}

static void launch_split_pass(ccz_ctx* c, const SplitTables& tb, const SplitViews& vws, bool aligned, int64_t r0, int64_t rows, int64_t ksteps,
                              const float* pilot, char* planes, double* msq, double* colsum, int dtype = CCZ_F32) {
  const int rb = split_rows_per_block(ksteps * SP_K, tb.np, std::max(1, impl(c)->props.multiProcessorCount));
  const unsigned nrb = (unsigned)((ksteps * SP_K + rb - 1) / rb);
  // panels fastest in the grid (CCZ_SPLIT_ORDER=0: row blocks fastest, the first form).  Measured at the
  // metric shape, alternating runs (tools/r6_split_order.sh): 12.1 / 10.7 / 10.6 ms against 12.6 / 12.3 / 11.9 -- never slower.
  const int panel_fast = (env::live(env::SPLIT_ORDER) != 0 && nrb <= 65535u) ? 1 : 0;
  const dim3 grid = panel_fast ? dim3((unsigned)tb.np, nrb) : dim3(nrb, (unsigned)tb.np);
  auto* kern = aligned ? &k_split_bf16x2<float, true> : &k_split_bf16x2<float, false>;
  if (dtype == CCZ_BF16) kern = aligned ? &k_split_bf16x2<bf16_t, true> : &k_split_bf16x2<bf16_t, false>;
  else if (dtype == CCZ_F16) kern = aligned ? &k_split_bf16x2<f16_t, true> : &k_split_bf16x2<f16_t, false>;
  hipLaunchKernelGGL(kern, grid, dim3(256), 0, stream(c), tb.panels, vws, r0, rows, ksteps, pilot, planes, msq, colsum, rb, panel_fast);
}

// The K1-layout planes of ONE fp32 matrix X (rows x cols, ld): panels of 256 columns, `ksteps` k-steps of 16 rows each (rows past
// `rows` are zero) -- the B side of gemm_split.hip's product (X = Gamma: its rows are the contraction index).  No pilot, no msq.
void split_k1_layout(ccz_ctx* c, const float* X, int64_t rows, int64_t cols, int64_t ld, int64_t ksteps, char* planes) {
  const SplitTables tb = split_tables(c, &cols, 1);
  const ccz_view v{X, cols, ld};
  SplitViews vws{};
  const bool aligned = split_views_arg(&v, 1, &vws);
  launch_split_pass(c, tb, vws, aligned, 0, rows, ksteps, nullptr, planes, nullptr, nullptr);
  CCZ_LAUNCH_CHECK();
}

// row chunk per workgroup of the Gram kernel over `ksteps` k-steps: minimise rounds x (steps + fixed cost) like gram.hip::plan_rows;
// whole multiples of 8 chunks on a chip-filling grid select the chunk-per-XCD walk
struct SplitRowPlan { int64_t steps_per_wg, ksplit, nblocks; int per_xcd; };
static SplitRowPlan split_row_plan(int64_t ksteps, int ntiles, int64_t max_steps, int ncu) {
  int64_t best_k = 1;
  const int64_t kmin = std::max<int64_t>(1, (ksteps + max_steps - 1) / max_steps);
  const int64_t kmax = std::max<int64_t>(kmin, std::min<int64_t>(ksteps / 16, 8192));
  double best = 1e300;
  for (int64_t ks = kmin; ks <= kmax; ++ks) {
    const int64_t steps = (ksteps + ks - 1) / ks;
    const bool big = int64_t(ntiles) * ks >= 16 * int64_t(ncu);
    int64_t rounds;
    if (big && ks % 8 == 0) rounds = ((ks / 8) * int64_t(ntiles) + ncu / 8 - 1) / (ncu / 8);
    else if (big) rounds = (int64_t((ntiles + 7) / 8) * ks + ncu / 8 - 1) / (ncu / 8);
    else rounds = (int64_t(ntiles) * ks + ncu - 1) / ncu;
    const double cost = (big && ks % 8 != 0 ? 1.03 : 1.0) * double(rounds) * double(steps + 24);
    if (cost < best) { best = cost; best_k = ks; }
  }
  SplitRowPlan rp;
  rp.steps_per_wg = (ksteps + best_k - 1) / best_k;
  rp.ksplit = (ksteps + rp.steps_per_wg - 1) / rp.steps_per_wg;
  const bool sliced = int64_t(ntiles) * rp.ksplit >= 16 * int64_t(ncu);
  const bool xchunks = sliced && rp.ksplit % 8 == 0 && env::live(env::SPLIT_WALK) != 1;      // (1: slices of the tile list instead)
  rp.per_xcd = xchunks ? -1 : (sliced ? (ntiles + 7) / 8 : 0);
  rp.nblocks = xchunks ? int64_t(ntiles) * rp.ksplit : (sliced ? int64_t(8) * rp.per_xcd * rp.ksplit : int64_t(ntiles) * rp.ksplit);
  if (rp.nblocks > 0x7fffffffLL) fail(CCZ_EUNSUP, "gram (split route): grid too large");
  if ((rp.steps_per_wg + SP_NST) * SP_PSTEP > 0x7fffffffLL) fail(CCZ_EUNSUP, "gram (split route): row chunk too long");
  return rp;
}

// Loss fast path on the split route (loss.hip: pair_core -> k_loss_prep_partials): the pilot-shifted Gram of a DCCA batch as per-(row
// chunk, tile) fp32 partial tiles -- the layout of gram.hip's staged kernel (slot = chunk * ntiles + tile, full tiles, no plan) --
// plus the exact column sums, the pilot and sum mid^2 for the diagonal.  Three launches: k_colsum_pilot (which also clears msq),
// the split pass, the MFMA kernel; nothing is reduced here (the consumer adds the chunks up in fp64 while it forms Ce).
// Default: from 32768 rows on (K1's own rule: there the route is at least as accurate as the fp32 kernel).  CCZ_LOSS_K1_SPLIT=2 takes
// it from 4096 rows on (8192 rows: 3.5e-7 against the fp32 kernel's 2.2e-7 -- the reference forms these moments by a float32 matmul
// and inverts them through a float32 eigh, cca_zoo/deep/objectives.py:9-21, :86-97, both looser): measured at BASELINE configs[3]
// (batch 8192, 2 x 512) the loss alone gets faster (0.63 -> 0.56 ms with the split backward) but a TRAINING STEP gets slower
// (2.50 -> 2.60 ms): the bf16 MFMA bursts pull the chip's clock down and the encoders' GEMMs next to them run ~10 % longer
// (profiles/r06_loss_c4.md).  So small batches keep the fp32 kernels unless asked.  CCZ_LOSS_K1_SPLIT=0: never.
bool gram_partials_split_f32(ccz_ctx* c, const ccz_view* views, int n_views, int64_t n, GramPartials* out) {
  const int mode = env::live(env::LOSS_K1_SPLIT);
  if (mode == 0 || c->k1_route == CCZ_K1_FP32) return false;
  if (n_views < 1 || n_views > 8 || n < (mode >= 2 ? 4096 : 32768)) return false;
  int64_t D = 0;
  int64_t cols[8];
  for (int v = 0; v < n_views; ++v) { cols[v] = views[v].cols; D += views[v].cols; }
  if (D < 512 || (D + 255) / 256 > 64 || double(n) * double(D) * double(D + 1) < 5e9) return false;
  Impl* im = impl(c);
  hipStream_t st = stream(c);
  const int ncu = std::max(1, im->props.multiProcessorCount);
  const SplitTables tb = split_tables(c, cols, n_views);
  const int64_t ksteps = (n + SP_K - 1) / SP_K;
  const SplitRowPlan rp = split_row_plan(ksteps, tb.ntiles, 16384 / SP_K, ncu);
  const int64_t partial_bytes = rp.ksplit * int64_t(tb.ntiles) * (SP_T * SP_T * 4);
  if (rp.per_xcd != 0 || partial_bytes > env::gram_partial_cap()) return false;           // a chip-filling grid: the general route through ccz_moments
  SplitViews vws{};
  const bool aligned = split_views_arg(views, n_views, &vws);
  double* msq = static_cast<double*>(dev_alloc(c, size_t(D) * 8));
  out->msq = msq;
  out->colsum = static_cast<double*>(dev_alloc(c, size_t(D) * 8));
  out->pilot = static_cast<float*>(dev_alloc(c, size_t(D) * 4));
  out->partial = static_cast<float*>(dev_alloc(c, size_t(partial_bytes)));
  out->planes = static_cast<char*>(dev_alloc(c, size_t(tb.np) * size_t(ksteps) * SP_PSTEP));
  out->tile_plan = nullptr;
  if (!colsum_pilot_f32(c, views, n_views, n, D, out->colsum, out->pilot, msq, D)) {
    gram_partials_release(c, out);
    return false;
  }
  launch_split_pass(c, tb, vws, aligned, 0, n, ksteps, out->pilot, out->planes, msq, nullptr);
  const size_t fifo_bytes = size_t(SP_NST) * SP_STAGE;
  sp_allow_lds(reinterpret_cast<const void*>(&k_gram_bf16x2), c->device, int(fifo_bytes));
  hipLaunchKernelGGL(k_gram_bf16x2, dim3((unsigned)rp.nblocks), dim3(256), fifo_bytes, st, tb.tiles, tb.ntiles, rp.per_xcd, rp.ksplit, out->planes, ksteps,
                     rp.steps_per_wg, out->partial);
  CCZ_LAUNCH_CHECK();
  out->tiles = tb.gtiles;
  out->ntiles = tb.ntiles;
  out->ksplit = rp.ksplit;
  c->last_pilot = 1;
  c->last_route = CCZ_K1_BF16X2;
  return true;
}

// Does the split route pay for this launch?  (auto mode)  It carries an HBM pass over the rows, a reduce over the partial
// tiles and two small table uploads; below ~1e11 algorithmic flops the fp32 kernel's single launch wins.
bool gram_split_worthwhile(int64_t n, int64_t D) {
  const double min_flop = env::live(env::SPLIT_MIN_FLOP);
  // n >= 32768: from there on the route's error against float64 moments is at or below the fp32 kernel's on the same rows
  // (the dropped 2^-16 terms average out over the rows, the fp32 kernel's accumulation error grows with them; measured
  // crossover 20k - 30k rows, tools/k1_route_check.py) -- below it the route is only taken when asked for
  return n >= 32768 && D >= 256 && double(n) * double(D) * double(D + 1) >= min_flop;
}

// G (upper tiles) += sum over rows of d d' for d = x - pilot (pilot may be null: d = x), through the split-bf16 route;
// dtype: the views' element type (CCZ_F32, or CCZ_BF16 / CCZ_F16: widened exactly by the split pass's load);
// colsum (may be null) += the exact fp64 column sums of x, gathered by the split pass on its way over the rows.
// Per row super-chunk one straight chain on the handle's stream: zero msq, split pass, MFMA kernel, reduce.  With time_it four HIP
// events bracket the three stages (one host wait per row super-chunk) into c->last_split_ms / last_mfma_ms / last_reduce_ms.
// (Round 6 also built a piped form, the split pass of the next row piece on a CU-masked side stream under the MFMA kernel of the
// current one: slower in every setting, profiles/r06_split_pipe_sweep.log and DESIGN.md section 7 item 2, and removed.)
void gram_split_f32(ccz_ctx* c, const ccz_view* views, int n_views, int64_t n, double* G, int64_t D, const float* pilot, double* colsum,
                    bool time_it, int dtype) {
  Impl* im = impl(c);
  hipStream_t st = stream(c);
  // ---- panels and tiles (device tables cached with the handle by the views' widths) ----
  if (n_views > SP_MAXV) fail(CCZ_EUNSUP, "gram (split route): more than %d views", SP_MAXV);
  if (D > 0x7fffffffLL - 256) fail(CCZ_EUNSUP, "gram (split route): stacked width too large");
  int64_t cols[SP_MAXV];
  for (int v = 0; v < n_views; ++v) cols[v] = views[v].cols;
  const SplitTables tb = split_tables(c, cols, n_views);
  SplitViews vws{};
  const bool aligned = split_views_arg(views, n_views, &vws, dtype);
  const int np = tb.np, ntiles = tb.ntiles;
  PoolBuf<double> msq(c, D);
  // ---- rows per launch (scratch budget) and per workgroup ----
  const int ncu = std::max(1, im->props.multiProcessorCount);
  const int64_t max_steps = std::max<int64_t>(1, env::live(env::SPLIT_ROWS) / SP_K);
  const int64_t unit = max_steps * SP_K;
  const double per_row = double(np) * SP_PSTEP / SP_K + double(ntiles) * (SP_T * SP_T * 4) / double(unit);
  const size_t budget = split_scratch_budget(c);
  int64_t launch_rows = std::max<int64_t>(int64_t(double(budget) / per_row) / unit * unit, unit);
  const int64_t n_launch = (n + launch_rows - 1) / launch_rows;
  launch_rows = ((n + n_launch - 1) / n_launch + SP_K - 1) / SP_K * SP_K;       // equal super-chunks
  const size_t fifo_bytes = size_t(SP_NST) * SP_STAGE;
  sp_allow_lds(reinterpret_cast<const void*>(&k_gram_bf16x2), c->device, int(fifo_bytes));
  c->last_split_ms = c->last_mfma_ms = c->last_reduce_ms = 0.0;
  // ---- plan, allocate, and only then enqueue: every super-chunk but the last has launch_rows rows, and the scratch is sized for the
  // larger of the two plans (split_row_plan is a cost search: the shorter last super-chunk may come out with MORE row chunks), so
  // an allocation that fails does so before anything has been added to G ----
  PoolBuf<char> planes;
  PoolBuf<float> partial;
  SplitRowPlan rp_full, rp_last;
  for (;;) {
    const int64_t full_steps = (std::min(launch_rows, n) + SP_K - 1) / SP_K;
    const int64_t last_steps = (n - (n - 1) / launch_rows * launch_rows + SP_K - 1) / SP_K;
    rp_full = split_row_plan(full_steps, ntiles, max_steps, ncu);
    rp_last = split_row_plan(last_steps, ntiles, max_steps, ncu);
    try {
      planes = PoolBuf<char>(c, int64_t(np) * full_steps * SP_PSTEP);
      partial = PoolBuf<float>(c, std::max(rp_full.ksplit, rp_last.ksplit) * int64_t(ntiles) * (SP_T * SP_T));
      break;
    } catch (const Error& e) {
      // the scratch did not fit (another library holds most of HBM): halve the row super-chunk and plan again
      if (e.code != CCZ_ENOMEM || launch_rows <= unit) throw;
      planes.reset();
      launch_rows = std::max<int64_t>(unit, launch_rows / 2 / unit * unit);
    }
  }
  hipEvent_t ev[4] = {};               // before the split pass, after it, after the MFMA kernel, after the reduce
  for (int q = 0; time_it && q < 4; ++q) {
    if (!im->sp_ev[q]) CCZ_HIP(hipEventCreate(im->sp_ev[q].out()));
    ev[q] = im->sp_ev[q].get();
  }
  for (int64_t r0 = 0; r0 < n; r0 += launch_rows) {
    const int64_t rows = std::min(launch_rows, n - r0), ksteps = (rows + SP_K - 1) / SP_K;
    const SplitRowPlan& rp = r0 + launch_rows < n ? rp_full : rp_last;
    zero(c, msq, size_t(D) * 8);
    if (time_it) CCZ_HIP(hipEventRecord(ev[0], st));
    launch_split_pass(c, tb, vws, aligned, r0, rows, ksteps, pilot, planes, msq, colsum, dtype);
    if (time_it) CCZ_HIP(hipEventRecord(ev[1], st));
    hipLaunchKernelGGL(k_gram_bf16x2, dim3((unsigned)rp.nblocks), dim3(256), fifo_bytes, st, tb.tiles, ntiles, rp.per_xcd, rp.ksplit, planes.get(), ksteps,
                       rp.steps_per_wg, partial.get());
    if (time_it) CCZ_HIP(hipEventRecord(ev[2], st));
    hipLaunchKernelGGL(k_split_reduce, dim3(64, (unsigned)ntiles), dim3(256), 0, st, partial.get(), tb.tiles, ntiles, rp.ksplit, G, D, msq.get());
    CCZ_LAUNCH_CHECK();
    if (time_it) {
      CCZ_HIP(hipEventRecord(ev[3], st));
      CCZ_HIP(hipEventSynchronize(ev[3]));
      float a = 0.f;
      CCZ_HIP(hipEventElapsedTime(&a, ev[0], ev[1]));
      c->last_split_ms += a;
      CCZ_HIP(hipEventElapsedTime(&a, ev[1], ev[2]));
      c->last_mfma_ms += a;
      CCZ_HIP(hipEventElapsedTime(&a, ev[2], ev[3]));
      c->last_reduce_ms += a;
    }
  }
}

}  // namespace ccz
