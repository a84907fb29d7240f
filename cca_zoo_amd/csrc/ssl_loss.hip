// Moment-map losses: the eigen-free objectives of the reference's self-supervised models, value + closed-form input gradients.
//
//   EY            cca_zoo/deep/_dcca_ey.py:10-111       -2 tr C + tr(V V_ind)
//   Barlow Twins  cca_zoo/deep/_barlowtwins.py:83-112   sum_i (1 - C_ii)^2 + lam sum_{i != j} C_ij^2,  C = z_1'z_2 / n (raw moments)
//   VICReg        cca_zoo/deep/_vicreg.py:12-67,142-169 sim mean((z_1 - z_2)^2) + std sum_a mean relu(1 - sigma_a) + cov sum_a offdiag(S_aa)^2 / d
//   SDL           cca_zoo/deep/_dcca_sdl.py:12-26,100-121  mean((z_1 - z_2)^2) + lam sum_a mean |offdiag S_aa|
//
// For m views of ONE width d (D = m d) each of them is a function of the batch second moments [G | s] of Z = [z_1 .. z_m] -- the matrix
// K1 builds for CCALoss -- and each gradient is one sample-side product
//     dZ = (Z - 1 mu') Gamma_c + Z Gamma_r  =  Z Gamma - 1 (mu' Gamma_c),      Gamma = Gamma_c + Gamma_r,
// Gamma_c the part that acts on centred data (covariance terms), Gamma_r the part that acts on raw data (Barlow Twins' raw cross
// moments, the squared difference of VICReg / SDL).  The state a forward leaves has the layout of the pairwise CCA loss (loss.hip:
// pair_loss_state_bytes_impl), so ccz_pair_loss_backward serves unchanged on all of its routes:
//     [Gamma fp64 (D x D) | mu' Gamma_c (D) | mu (D) | mu' Gamma_c - fl32(mu)' Gamma (D) | Gamma fp32 (D x D)]
// The fourth row is what the split-bf16 backward subtracts after it has shifted the rows by fl32(mu) (gemm_split.hip): for the CCA
// loss (Gamma_r = 0) that is the pilot correction (mu - fl32(mu))' Gamma; written as above it reproduces the centring row exactly
// whatever Gamma_r is.
//
// Launches of one forward: K1 (moments_impl, pilot always on for fp32: no host read-back), k_sqdiff for VICReg / SDL (the VALUE of
// mean((z_1 - z_2)^2) is not formed from the Gram: tr G_11 + tr G_22 - 2 tr G_12 cancels to the rounding level of the fp32 Gram when
// z_1 ~ z_2, the state training drives towards; its gradient is linear in Z and goes through Gamma_r), k_moment_map, k_moment_finish.
// With an independent batch (EY) K1, the map and the finish run once more for its own Gamma.  Every cross-workgroup sum goes through
// per-workgroup partials that the NEXT launch adds in index order: no atomics in this file (K1 keeps its own order of summation).
// Enqueue-only.
#include <algorithm>
#include <cmath>

#include "hip_common.h"
#include "half_cvt.h"
#include "reduce.h"

namespace ccz {

int64_t pair_loss_state_bytes_impl(int dtype, const int64_t* dims, int m);   // loss.hip

namespace {

constexpr int SMAXV = 8;               // views one pass serves (as the pairwise CCA loss)
constexpr int SQ_MAX_BLOCKS = 1024;    // workgroups of k_sqdiff
constexpr double VICREG_EPS = 1e-4;    // the reference's constant inside the square root (_vicreg.py:37)

struct MomentMapArgs {
  int kind;          // CCZ_MOMENT_*
  int role;          // 0: the batch itself (terms + its Gamma); 1: EY's independent batch (its Gamma only)
  int m;
  int has_other;     // EY: a second set of moments (role 0: the independent batch's; role 1: the batch's)
  int64_t d, D;
  double n, n_other;
  double p0, p1, p2; // the loss's coefficients
};

__device__ __forceinline__ double cov_at(const double* __restrict__ G, const double* __restrict__ s, int64_t D, double inv_n, double inv_nm1,
                                         int64_t i, int64_t j) {
  const double g = i <= j ? G[i * D + j] : G[j * D + i];       // K1 leaves the upper triangle
  return (g - s[i] * s[j] * inv_n) * inv_nm1;
}

// V = (1 / m) sum_a S_aa at (p, q)
__device__ __forceinline__ double ey_v_at(const double* __restrict__ G, const double* __restrict__ s, int64_t D, int64_t d, int m, double inv_n,
                                          double inv_nm1, int64_t p, int64_t q) {
  double v = 0.0;
  for (int a = 0; a < m; ++a) v += cov_at(G, s, D, inv_n, inv_nm1, a * d + p, a * d + q);
  return v / double(m);
}

// One 64 x 64 tile of Gamma per workgroup (rows i = source column of Z, columns j = gradient column), as k_loss_tail: Gamma in
// fp64 and fp32, this tile's share of the centring row and of the split route's row (pbias / pcorr [tile row][j]) and of the terms
// (pterms [tile][3]).  gamma == null (no gradient wanted): the terms only.  grid (ceil(D / 64), ceil(D / 64)) x 256.
__global__ __launch_bounds__(256) void k_moment_map(MomentMapArgs A, const double* __restrict__ G, const double* __restrict__ s,
                                                    const double* __restrict__ Go, const double* __restrict__ so, double* __restrict__ gamma,
                                                    float* __restrict__ g32, double* __restrict__ pbias, double* __restrict__ pcorr,
                                                    double* __restrict__ pterms) {
  __shared__ double red[4][64];
  __shared__ double redc[4][64];
  __shared__ double sh[4];
  const int c = threadIdx.x & 63, rg = threadIdx.x >> 6;
  const int64_t D = A.D, d = A.d;
  const int64_t j = int64_t(blockIdx.x) * 64 + c, i0 = int64_t(blockIdx.y) * 64;
  const double inv_n = 1.0 / A.n, inv_nm1 = 1.0 / (A.n - 1.0);
  const double ino = 1.0 / A.n_other, ino1 = 1.0 / (A.n_other - 1.0);
  const double dd = double(d), md = double(A.m);
  double bsum = 0.0, csum = 0.0, t0 = 0.0, t1 = 0.0, t2 = 0.0;
  if (j < D) {
    const int b = int(j / d);
    const int64_t jb = j - int64_t(b) * d;
    const int64_t i1 = i0 + 64 < D ? i0 + 64 : D;
    for (int64_t i = i0 + rg; i < i1; i += 4) {
      const int a = int(i / d);
      const int64_t ia = i - int64_t(a) * d;
      const bool dg = ia == jb;
      double gc = 0.0, gr = 0.0;
      if (A.kind == CCZ_MOMENT_EY) {
        if (A.role == 0) {
          if (dg) {
            gc = -4.0 / md * inv_nm1;
            t0 += 2.0 / md * cov_at(G, s, D, inv_n, inv_nm1, i, j);
          }
          if (a == b) {
            double v = 0.0, vo;
            if (!A.has_other) {
              v = vo = ey_v_at(G, s, D, d, A.m, inv_n, inv_nm1, ia, jb);
            } else {
              vo = ey_v_at(Go, so, D, d, A.m, ino, ino1, ia, jb);
              if (a == 0) v = ey_v_at(G, s, D, d, A.m, inv_n, inv_nm1, ia, jb);
            }
            gc += (A.has_other ? 2.0 : 4.0) / md * inv_nm1 * vo;
            if (a == 0) t1 += v * vo;
          }
        } else if (a == b) {
          gc = 2.0 / md * inv_nm1 * ey_v_at(Go, so, D, d, A.m, ino, ino1, ia, jb);
        }
      } else if (A.kind == CCZ_MOMENT_BARLOW) {
        if (a != b) {
          const int64_t p = a == 0 ? ia : jb, q = a == 0 ? jb : ia;      // C_pq = (z_1' z_2)_pq / n; Gamma is symmetric
          const double C = G[p * D + d + q] * inv_n;
          gr = (p == q ? -2.0 * (1.0 - C) : 2.0 * A.p0 * C) * inv_n;
          if (a == 0) {
            if (p == q) t0 += (1.0 - C) * (1.0 - C);
            else t1 += C * C;
          }
        }
      } else if (A.kind == CCZ_MOMENT_VICREG) {
        if (a == b) {
          const double S = cov_at(G, s, D, inv_n, inv_nm1, i, j);
          if (!dg) {
            gc = A.p2 * 4.0 * S / dd * inv_nm1;
            t2 += S * S / dd;
          } else {
            const double sig = sqrt(S + VICREG_EPS);
            if (sig < 1.0) {
              gc = -A.p1 / (sig * dd) * inv_nm1;
              t1 += (1.0 - sig) / dd;
            }
          }
        }
        if (dg) gr = (a == b ? 2.0 : -2.0) * A.p0 * inv_n / dd;
      } else {   // CCZ_MOMENT_SDL
        if (a == b && !dg) {
          const double S = cov_at(G, s, D, inv_n, inv_nm1, i, j);
          const double sg = double(S > 0.0) - double(S < 0.0);
          gc = A.p0 * 2.0 * sg / (dd * (dd - 1.0)) * inv_nm1;
          t1 += fabs(S) / (dd * (dd - 1.0));
        }
        if (dg && a < 2 && b < 2) gr = (a == b ? 2.0 : -2.0) * inv_n / dd;
      }
      if (gamma) {
        const double g = gc + gr;
        gamma[i * D + j] = g;
        if (g32) g32[i * D + j] = float(g);
        const double mi = s[i] * inv_n;
        bsum += mi * gc;
        csum += mi * gc - double(float(mi)) * g;
      }
    }
  }
  red[rg][c] = bsum;
  redc[rg][c] = csum;
  __syncthreads();
  if (gamma && rg == 0 && j < D) {
    pbias[int64_t(blockIdx.y) * D + j] = red[0][c] + red[1][c] + red[2][c] + red[3][c];
    pcorr[int64_t(blockIdx.y) * D + j] = redc[0][c] + redc[1][c] + redc[2][c] + redc[3][c];
  }
  if (A.role == 0) {
    t0 = block_sum<4>(t0, sh);
    t1 = block_sum<4>(t1, sh);
    t2 = block_sum<4>(t2, sh);
    if (threadIdx.x == 0) {
      double* pt = pterms + (int64_t(blockIdx.y) * gridDim.x + blockIdx.x) * 3;
      pt[0] = t0; pt[1] = t1; pt[2] = t2;
    }
  }
}

// The partials in index order: the state's three rows (centring row, batch mean, split-route row; one thread per column) and -- workgroup
// 0, role 0 -- the terms (3 doubles, optional) and the objective (one element of dtype).  grid ceil(D / 256) (state) or 1, x 256.
__global__ __launch_bounds__(256) void k_moment_finish(MomentMapArgs A, const double* __restrict__ s, int tiles, const double* __restrict__ pbias,
                                                       const double* __restrict__ pcorr, const double* __restrict__ pterms,
                                                       const double* __restrict__ sq_part, int nsq, double* __restrict__ rows, int dtype,
                                                       void* __restrict__ loss, double* __restrict__ terms) {
  __shared__ double sh[4];
  const int64_t D = A.D;
  const int64_t j = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (rows && j < D) {
    double b = 0.0, cr = 0.0;
    for (int ty = 0; ty < tiles; ++ty) {
      b += pbias[int64_t(ty) * D + j];
      cr += pcorr[int64_t(ty) * D + j];
    }
    rows[j] = b;
    rows[D + j] = s[j] / A.n;
    rows[2 * D + j] = cr;
  }
  if (blockIdx.x != 0 || A.role != 0) return;
  double t0 = 0.0, t1 = 0.0, t2 = 0.0, sq = 0.0;
  for (int t = threadIdx.x; t < tiles * tiles; t += 256) {
    t0 += pterms[3 * t];
    t1 += pterms[3 * t + 1];
    t2 += pterms[3 * t + 2];
  }
  for (int t = threadIdx.x; t < nsq; t += 256) sq += sq_part[t];
  t0 = block_sum<4>(t0, sh);
  t1 = block_sum<4>(t1, sh);
  t2 = block_sum<4>(t2, sh);
  sq = block_sum<4>(sq, sh);
  if (threadIdx.x != 0) return;
  double obj;
  if (A.kind == CCZ_MOMENT_EY) {
    obj = -t0 + t1;                                 // rewards, penalties
  } else if (A.kind == CCZ_MOMENT_BARLOW) {
    obj = t0 + A.p0 * t1;                           // invariance, redundancy
  } else if (A.kind == CCZ_MOMENT_VICREG) {
    t0 = sq / (A.n * double(A.d));                  // sim, var, cov
    obj = A.p0 * t0 + A.p1 * t1 + A.p2 * t2;
  } else {
    t0 = sq / (A.n * double(A.d));                  // l2, sdl
    obj = t0 + A.p0 * t1;
  }
  if (terms) { terms[0] = t0; terms[1] = t1; terms[2] = t2; }
  if (dtype == CCZ_F32) *static_cast<float*>(loss) = float(obj);
  else *static_cast<double*>(loss) = obj;
}

template <typename T, int V>
struct alignas(sizeof(T) * V) VecOf {
  T v[V];
};

// part[workgroup] = this workgroup's share of sum (z_1 - z_2)^2 over the n x d elements of two views where they lie: V elements
// of a row per load, fp64 from the subtraction on (per thread, by wavefront shuffle, across the waves).
template <typename T, int V>
__global__ __launch_bounds__(256) void k_sqdiff(const T* __restrict__ z1, int64_t ld1, const T* __restrict__ z2, int64_t ld2, int64_t n, int64_t d,
                                                double* __restrict__ part) {
  __shared__ double sh[4];
  const int64_t dv = d / V, total = n * dv, stride = int64_t(gridDim.x) * 256;
  const int64_t srow = stride / dv, scol = stride - srow * dv;
  int64_t e = int64_t(blockIdx.x) * 256 + threadIdx.x;
  int64_t row = e / dv, col = e - row * dv;
  double acc = 0.0;
  for (; e < total; e += stride) {
    const VecOf<T, V> x = *reinterpret_cast<const VecOf<T, V>*>(z1 + row * ld1 + col * V);
    const VecOf<T, V> y = *reinterpret_cast<const VecOf<T, V>*>(z2 + row * ld2 + col * V);
#pragma unroll
    for (int k = 0; k < V; ++k) {
      const double df = to_f64(x.v[k]) - to_f64(y.v[k]);
      acc += df * df;
    }
    row += srow;
    col += scol;
    if (col >= dv) { col -= dv; ++row; }
  }
  acc = block_sum<4>(acc, sh);
  if (threadIdx.x == 0) part[blockIdx.x] = acc;
}

template <typename T, int V>
void launch_sqdiff(hipStream_t st, int nblocks, const ccz_view& a, const ccz_view& b, int64_t n, double* part) {
  hipLaunchKernelGGL((k_sqdiff<T, V>), dim3((unsigned)nblocks), dim3(256), 0, st, static_cast<const T*>(a.data), a.ld, static_cast<const T*>(b.data),
                     b.ld, n, a.cols, part);
}

bool vec_ok(const ccz_view& v, size_t bytes, int64_t V) {
  return v.cols % V == 0 && v.ld % V == 0 && reinterpret_cast<uintptr_t>(v.data) % bytes == 0;
}

void check_views(const ccz_view* z, int m, int64_t d, const char* what) {
  for (int a = 0; a < m; ++a) {
    if (!z[a].data || z[a].cols < 1 || z[a].ld < z[a].cols) fail(CCZ_EINVAL, "moment loss: bad shape (%s view %d)", what, a);
    if (z[a].cols != d) fail(CCZ_EINVAL, "moment loss: every view must have the same width (%s view %d has %lld, view 0 has %lld)", what, a,
                             (long long)z[a].cols, (long long)d);
  }
}

// map + finish of one set of moments
void map_and_finish(ccz_ctx* c, const MomentMapArgs& A, int dtype, const double* mom, const double* mom_other, const double* sq_part, int nsq,
                    void* state, void* loss_dev, double* terms_dev) {
  hipStream_t st = stream(c);
  const int64_t D = A.D;
  const int tiles = int((D + 63) / 64);
  double* gamma = static_cast<double*>(state);
  float* g32 = (gamma && dtype == CCZ_F32) ? reinterpret_cast<float*>(gamma + (D + 3) * D) : nullptr;
  DBuf pterms(c, A.role == 0 ? int64_t(tiles) * tiles * 3 : 0), prow(c, gamma ? int64_t(tiles) * D * 2 : 0);
  double* pbias = prow.get();
  double* pcorr = gamma ? pbias + int64_t(tiles) * D : nullptr;
  hipLaunchKernelGGL(k_moment_map, dim3((unsigned)tiles, (unsigned)tiles), dim3(256), 0, st, A, mom, mom + D * D, mom_other,
                     mom_other ? mom_other + D * D : nullptr, gamma, g32, pbias, pcorr, pterms.get());
  CCZ_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_moment_finish, dim3((unsigned)(gamma ? (D + 255) / 256 : 1)), dim3(256), 0, st, A, mom + D * D, tiles, pbias, pcorr,
                     pterms.get(), sq_part, nsq, gamma ? gamma + D * D : nullptr, dtype, loss_dev, terms_dev);
  CCZ_LAUNCH_CHECK();
}

}  // namespace

int64_t moment_loss_state_bytes_impl(int dtype, int64_t d, int m) {
  if (m < 2 || m > SMAXV || d < 1) return -1;
  int64_t dims[SMAXV];
  for (int a = 0; a < m; ++a) dims[a] = d;
  return pair_loss_state_bytes_impl(dtype, dims, m);
}

void moment_loss_forward_impl(ccz_ctx* c, int dtype, int kind, const double* params, const ccz_view* z, int m, int64_t n, const ccz_view* zi,
                              int64_t n_ind, void* loss_dev, double* terms_dev, void* state, void* state_ind) {
  if (dtype != CCZ_F32 && dtype != CCZ_F64 && !is_half_dtype(dtype)) fail(CCZ_EUNSUP, "moment loss: dtype must be CCZ_F32, CCZ_F64, CCZ_BF16 or CCZ_F16");
  // half views: K1 and the squared difference read them where they lie (widened exactly on load); the map, the loss element and the
  // state behind them are float32's
  const int vdtype = dtype;
  if (is_half_dtype(dtype)) dtype = CCZ_F32;
  if (kind < CCZ_MOMENT_EY || kind > CCZ_MOMENT_SDL) fail(CCZ_EINVAL, "moment loss: unknown kind %d", kind);
  if (!z || !loss_dev) fail(CCZ_EINVAL, "moment loss: null argument");
  const bool two = kind == CCZ_MOMENT_BARLOW || kind == CCZ_MOMENT_VICREG;
  if (two ? m != 2 : (m < 2 || m > SMAXV)) fail(CCZ_EUNSUP, "moment loss: %s views are supported, got %d", two ? "exactly 2" : "2 .. 8", m);
  if (n < 2) fail(CCZ_EINVAL, "moment loss: bad shape (at least 2 rows are required)");
  const int64_t d = z[0].cols;
  check_views(z, m, d, "");
  if (kind == CCZ_MOMENT_SDL && d < 2) fail(CCZ_EINVAL, "moment loss: SDL needs at least 2 columns per view");
  if (kind != CCZ_MOMENT_EY && !params) fail(CCZ_EINVAL, "moment loss: null argument (params)");
  if (zi) {
    if (kind != CCZ_MOMENT_EY) fail(CCZ_EINVAL, "moment loss: only EY takes an independent batch");
    if (n_ind < 2) fail(CCZ_EINVAL, "moment loss: bad shape (at least 2 independent rows are required)");
    check_views(zi, m, d, "independent");
  } else if (state_ind) {
    fail(CCZ_EINVAL, "moment loss: a state for an independent batch that was not given");
  }
  const int64_t D = int64_t(m) * d;
  hipStream_t st = stream(c);
  const int pilot = dtype == CCZ_F32 ? 2 : 0;       // always shifted, decided on the device: no read-back
  DBuf mom(c, D * D + D), momi(c, zi ? D * D + D : 0);
  moments_impl(c, vdtype, z, m, n, true, mom, false, pilot, false);
  if (zi) moments_impl(c, vdtype, zi, m, n_ind, true, momi, false, pilot, false);
  int nsq = 0;
  DBuf sq_part;
  if (kind == CCZ_MOMENT_VICREG || kind == CCZ_MOMENT_SDL) {
    const bool f32 = vdtype == CCZ_F32, f64 = vdtype == CCZ_F64;
    const int per16 = f32 ? 4 : (f64 ? 2 : 8);          // elements of a 16-byte load
    const bool vec = vec_ok(z[0], 16, per16) && vec_ok(z[1], 16, per16);
    const int64_t items = n * d / (vec ? per16 : 1);
    nsq = int(std::min<int64_t>(SQ_MAX_BLOCKS, std::max<int64_t>(1, (items + 1023) / 1024)));
    sq_part = DBuf(c, nsq);
    if (f32) {
      if (vec) launch_sqdiff<float, 4>(st, nsq, z[0], z[1], n, sq_part);
      else launch_sqdiff<float, 1>(st, nsq, z[0], z[1], n, sq_part);
    } else if (f64) {
      if (vec) launch_sqdiff<double, 2>(st, nsq, z[0], z[1], n, sq_part);
      else launch_sqdiff<double, 1>(st, nsq, z[0], z[1], n, sq_part);
    } else if (vdtype == CCZ_BF16) {
      if (vec) launch_sqdiff<bf16_t, 8>(st, nsq, z[0], z[1], n, sq_part);
      else launch_sqdiff<bf16_t, 1>(st, nsq, z[0], z[1], n, sq_part);
    } else {
      if (vec) launch_sqdiff<f16_t, 8>(st, nsq, z[0], z[1], n, sq_part);
      else launch_sqdiff<f16_t, 1>(st, nsq, z[0], z[1], n, sq_part);
    }
    CCZ_LAUNCH_CHECK();
  }
  MomentMapArgs A{};
  A.kind = kind; A.role = 0; A.m = m; A.has_other = zi ? 1 : 0;
  A.d = d; A.D = D;
  A.n = double(n); A.n_other = zi ? double(n_ind) : double(n);
  A.p0 = params ? params[0] : 0.0;
  A.p1 = (params && kind == CCZ_MOMENT_VICREG) ? params[1] : 0.0;
  A.p2 = (params && kind == CCZ_MOMENT_VICREG) ? params[2] : 0.0;
  map_and_finish(c, A, dtype, mom, zi ? momi.get() : nullptr, sq_part.get(), nsq, state, loss_dev, terms_dev);
  if (zi && state_ind) {
    MomentMapArgs B = A;
    B.role = 1; B.has_other = 1;
    B.n = double(n_ind); B.n_other = double(n);
    map_and_finish(c, B, dtype, momi, mom, nullptr, 0, state_ind, loss_dev, nullptr);
  }
}

}  // namespace ccz
