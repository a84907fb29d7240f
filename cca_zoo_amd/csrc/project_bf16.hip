// transform / score of bfloat16 rows:  out (n x k, fp32) = X W - 1 bias'  (bias = mean' W, k <= 64 directions), X read as it lies.
//
// A bf16 element is already an exact operand of v_mfma_f32_32x32x16_bf16, so -- unlike project_split.hip, whose structure this
// is -- X needs no pilot, no split and no VALU work at all: lane l of a row tile DMAs 16 bytes of row l & 31 (columns 8 (l >> 5)
// .. + 7 of a k-step) into LDS and reads its own 16 bytes back as the MFMA operand.  Only W is split: three bf16 planes
// hi + mid + lo = fl32(W) (k_project_prep's layout, prepared once per call), and per k-step and column tile
//   acc += Wh x;  acc += Wm x;  acc += Wl x        (every product exact in float32, one fp32 accumulator).
// The centring row is NOT accumulated with atomics: bias = mean' W comes from the fp64 gemm (as for the fp32 kernel) and is
// subtracted in the epilogue, so two calls give the same bits.
//
// A wave owns 64 rows (2 row tiles) and two wave-private LDS-DMA rings, no barrier anywhere:
//   X ring  2 slots of 64 columns (four k-steps, 8 KiB: [row tile 2][k-step 4][1 KiB]).  A slot's eight DMAs are issued together,
//           row tile by row tile, so the four 32-byte pieces of a row's 128-byte line are requested back to back.
//   W ring  4 slots of ONE k-step ([plane 3][column tile NJ][1 KiB]: 6 KiB, 3 KiB when k <= 32), three k-steps ahead.  The planes
//           come from L2 (1.5 MB at d = 4096) and 64 columns of them would be 24 KiB per slot: four waves could not hold two.
// 4 x (16 + 24) KiB = 160 KiB: one workgroup per CU.
// Issue order (W = the DMAs of one k-step's planes, X = those of one slot):  prologue X0 W0 W1 W2;  step (slot S, k-step q of it):
// wait, read the fragments, issue W(4 S + q + 3) and, at q == 0, X(S + 1) behind it, then the MFMAs.  What is younger than the
// data a step needs is therefore two k-steps of W at q == 0 and two k-steps of W plus one slot of X otherwise: the counted waits.
// Rows past n and k-steps past d are requested with an offset past the descriptor's range and arrive as zeros; the plane buffer
// is allocated (and zero-filled) for every k-step the run-ahead asks for.
#include <algorithm>
#include <cstdlib>

#include "hip_common.h"
#include "split_mma.h"

namespace ccz {

namespace {

constexpr int PB_XSLOT = 8192;                    // bytes of an X slot: 64 rows x 64 columns bf16
constexpr int PB_XR = 2;                          // X slots per wave
constexpr int PB_WR = 4;                          // W slots (k-steps) per wave: equals the k-steps of an X slot, so slot = q
constexpr int PB_WSTEP = 3 * 2048;                // bytes of one k-step in the plane buffer: [plane 3][column tile 2][1 KiB]
constexpr int PB_OOB = 0x7ffffff0;                // a buffer offset past every descriptor this kernel builds
constexpr int64_t PB_MAXBYTES = 0x7fff0000LL;     // largest X panel (64 rows) a descriptor may span

template <int NJ> struct PB {
  static constexpr int WB = 3 * NJ * 1024;                         // bytes of a W slot
  static constexpr int WD = 3 * NJ;                                // DMAs of a W slot
  static constexpr int XD = 8;                                     // DMAs of an X slot
  static constexpr int WAVE = PB_XR * PB_XSLOT + PB_WR * WB;       // LDS bytes per wave
};

template <int NJ>
__global__ __launch_bounds__(256, 1) void k_project_bf16(const unsigned short* __restrict__ X, int64_t n, int64_t d, int64_t ld,
                                                          const char* __restrict__ planes, int nsteps_alloc, const double* __restrict__ bias,
                                                          float* __restrict__ out, int64_t ldo, int k) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int WB = PB<NJ>::WB, WD = PB<NJ>::WD, XD = PB<NJ>::XD;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t m0 = (int64_t(blockIdx.x) * 4 + wave) * 64;
  if (m0 >= n) return;
  const int64_t rows = min<int64_t>(64, n - m0);
  const int nsteps = int(d / 16);
  const int nslots = (nsteps + 3) / 4;
  char* ring = smem + wave * PB<NJ>::WAVE;
  char* wring = ring + PB_XR * PB_XSLOT;
  const char* rd = ring + lane * 16;
  const char* rdw = wring + lane * 16;
  const __amdgpu_buffer_rsrc_t srcX = panel_rsrc(X + m0 * ld, ((rows - 1) * ld + d) * 2);
  const __amdgpu_buffer_rsrc_t srcW = panel_rsrc(planes, int64_t(nsteps_alloc) * PB_WSTEP);
  int voffX[2];
#pragma unroll
  for (int mt = 0; mt < 2; ++mt) voffX[mt] = int(((mt * 32 + (lane & 31)) * ld + 8 * (lane >> 5)) * 2);     // (rows past the shard: past the range)
  const int voffW = lane * 16;

  sp_v16f32 acc[2][NJ];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  // the planes of k-step ks (always inside the allocation) into W slot `wslot`
  auto dmaW = [&](int wslot, int ks) {
#pragma unroll
    for (int p = 0; p < 3; ++p)
#pragma unroll
      for (int jt = 0; jt < NJ; ++jt)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(srcW, (sp_lds_ptr)(wring + wslot * WB + (p * NJ + jt) * 1024), 16, voffW,
                                                 ks * PB_WSTEP + p * 2048 + jt * 1024, 0, 0);
  };
  // the 64 columns of slot S into X buffer b: per row tile the four pieces of a row's line; k-steps past d: zeros
  auto dmaX = [&](int b, int S) {
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int ks = 4 * S + q;
        const bool live = ks < nsteps;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(srcX, (sp_lds_ptr)(ring + b * PB_XSLOT + (mt * 4 + q) * 1024), 16, live ? voffX[mt] : PB_OOB,
                                                 live ? ks * 32 : 0, 0, 0);
      }
  };
  static_assert(XD == 8 && (2 * WD == 12 || 2 * WD == 6), "the counted waits below assume these DMA counts");
  dmaX(0, 0);
#pragma unroll
  for (int s = 0; s < PB_WR - 1; ++s) dmaW(s, s);
  const int nloop = (nslots + PB_XR - 1) / PB_XR;
  for (int it = 0; it < nloop; ++it) {
#pragma unroll
    for (int u = 0; u < PB_XR; ++u) {
      const int S = it * PB_XR + u;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int ks = 4 * S + q;
        // everything but the two newest k-steps of W (and, past q == 0, the next slot of X) has landed
        if (NJ == 2) {
          if (q == 0) asm volatile("s_waitcnt vmcnt(12)" ::: "memory");
          else asm volatile("s_waitcnt vmcnt(20)" ::: "memory");
        } else {
          if (q == 0) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
          else asm volatile("s_waitcnt vmcnt(14)" ::: "memory");
        }
        if (S >= nslots) {                          // (the ring period past the last slot: keep the DMA count, skip the arithmetic)
          dmaW((q + PB_WR - 1) % PB_WR, ks + PB_WR - 1);
          if (q == 0) dmaX(u ^ 1, S + 1);
          continue;
        }
        sp_v8bf16 w[3][NJ], x[2];
#pragma unroll
        for (int p = 0; p < 3; ++p)
#pragma unroll
          for (int jt = 0; jt < NJ; ++jt) w[p][jt] = *reinterpret_cast<const sp_v8bf16*>(rdw + q * WB + (p * NJ + jt) * 1024);
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) x[mt] = *reinterpret_cast<const sp_v8bf16*>(rd + u * PB_XSLOT + (mt * 4 + q) * 1024);
        // refill: the W slot of k-step ks - 1 and, at the head of a slot, the X buffer of slot S - 1 (both consumed a k-step ago)
        dmaW((q + PB_WR - 1) % PB_WR, ks + PB_WR - 1);
        if (q == 0) dmaX(u ^ 1, S + 1);
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
          for (int jt = 0; jt < NJ; ++jt)
#pragma unroll
            for (int p = 0; p < 3; ++p) acc[mt][jt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w[p][jt], x[mt], acc[mt][jt], 0, 0, 0);
      }
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  // epilogue: lane l of tile (mt, jt): sample m0 + 32 mt + (l & 31), directions 32 jt + (r & 3) + 8 (r >> 2) + 4 (l >> 5)
#pragma unroll
  for (int mt = 0; mt < 2; ++mt) {
    const int64_t m = m0 + mt * 32 + (lane & 31);
    if (m >= n) continue;
#pragma unroll
    for (int jt = 0; jt < NJ; ++jt)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int j = jt * 32 + 8 * g + 4 * (lane >> 5);
        if (j >= k) continue;
        float v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = bias && j + e < k ? float(double(acc[mt][jt][4 * g + e]) - bias[j + e]) : acc[mt][jt][4 * g + e];
        float* o = out + m * ldo + j;
        if (j + 3 < k && (reinterpret_cast<uintptr_t>(o) & 15) == 0) {
          *reinterpret_cast<sp_v4f32*>(o) = sp_v4f32{v[0], v[1], v[2], v[3]};
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (j + e < k) o[e] = v[e];
        }
      }
  }
}

template <int NJ>
void launch(ccz_ctx* c, const void* X, int64_t n, int64_t d, int64_t ld, const char* planes, int nsteps_alloc, const double* bias, float* out,
            int64_t ldo, int k) {
  const size_t lds = size_t(4) * PB<NJ>::WAVE;
  sp_allow_lds(reinterpret_cast<const void*>(&k_project_bf16<NJ>), c->device, int(lds));
  const int64_t wgs = (n + 255) / 256;
  hipLaunchKernelGGL(k_project_bf16<NJ>, dim3((unsigned)wgs), dim3(256), lds, stream(c), static_cast<const unsigned short*>(X), n, d, ld, planes,
                     nsteps_alloc, bias, out, ldo, k);
  CCZ_LAUNCH_CHECK();
}

}  // namespace

bool project_bf16_eligible(int64_t n, int64_t d, int64_t k, int64_t ld, const void* X, int64_t ldo) {
  if (env::live(env::PROJECT_BF16) == 0) return false;
  if (n < 1 || k < 1 || k > 64 || d < 16 || d % 16 != 0 || ld < d || ld % 8 != 0 || reinterpret_cast<uintptr_t>(X) % 16 != 0 || ldo < k) return false;
  if ((64 * ld + d) * 2 > PB_MAXBYTES) return false;              // a wave's 64 rows behind one 32-bit buffer offset
  if ((d / 16 + 16) * int64_t(PB_WSTEP) > PB_MAXBYTES) return false;   // the planes behind one
  if ((n + 255) / 256 > 0x7fffffffLL) return false;
  return true;
}

void project_bf16(ccz_ctx* c, const void* X, int64_t n, int64_t d, int64_t ld, const double* bias, const double* W, int64_t k, float* out,
                  int64_t ldo) {
  const int64_t nslots = (d / 16 + 3) / 4, nloop = (nslots + PB_XR - 1) / PB_XR;
  const int64_t nsteps_alloc = 4 * PB_XR * nloop + PB_WR - 1;       // the last step of the loop asks for k-step 8 nloop + 2
  PoolBuf<char> planes(c, nsteps_alloc * PB_WSTEP);
  project_prep_planes3(c, W, d, k, nsteps_alloc, planes);
  if (k <= 32) launch<1>(c, X, n, d, ld, planes, int(nsteps_alloc), bias, out, ldo, int(k));
  else launch<2>(c, X, n, d, ld, planes, int(nsteps_alloc), bias, out, ldo, int(k));
}

}  // namespace ccz
