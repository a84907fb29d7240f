// The random draws of permutation_test and bootstrap, made where they are used (cca_zoo_amd/model_selection/_resample.py;
// the reference has no counterpart -- the specification is tests/draw_restatement.py).  Both are pure functions of
// (seed, b, n), b the resample's index in the whole call, on the stream convention of svi.hip / nuts.hip:
//   stream(seed, b, site) = splitmix64(splitmix64(splitmix64(seed) + b) + site)
//   key(seed, b, site, j) = splitmix64(stream(seed, b, site) ^ splitmix64(j))
//   pi_b = argsort_j key(seed, b, CCZ_DRAW_SITE_PERM, j)                 m_b[s] = #{j < n : (key(seed, b, CCZ_DRAW_SITE_BOOT, j) * n) >> 64 = s}
// splitmix64 is a bijection of the 64-bit words (an add, two xor-shifts and two odd multiplications, each invertible), so
// j -> key is one-to-one: the n keys of a stream are pairwise distinct, the order is total and there is no tie rule.
// Integer arithmetic and integer atomics only: the result has no rounding and no order of summation to depend on.
//
// Permutations: a one-level bucket sort of keys that are never stored (a key is recomputed from j wherever it is needed).
// The key range is cut into nb = ceil(n / bucket_rows) equal buckets, bucket = (key * nb) >> 64, monotone in the key, so the
// sorted buckets one after the other are the sorted keys.
//   k_draw_count    grid (stripe of DRAW_STRIPE j's, permutation).  Bucket histogram of the stripe: in LDS when nb <= DRAW_HIST
//                   (then one global add per non-empty bucket and workgroup), else straight into cnt[permutation][nb].
//   k_draw_scan     grid (permutation).  cnt -> exclusive prefix sums, in place: one workgroup walks the nb counts in tiles of
//                   1024 with a carry (nb reaches 2^21 at n = 2^31 and the default bucket_rows).
//   k_draw_scatter  grid as k_draw_count.  A slot from the bucket's cursor (the prefix sum, which thereby becomes the bucket's
//                   end) and tmp[permutation][slot] = j.  nb <= DRAW_HIST: the stripe's histogram in LDS first, ONE returning
//                   global add per non-empty bucket reserves the stripe's slots, the slots are dealt by LDS adds.  The order
//                   inside a bucket is whatever the atomics gave; its contents are not.
//   k_draw_sort     grid (bucket, permutation).  A bucket of at most CCZ_DRAW_SORT_CAP rows: (key, j) into LDS, a bitonic
//                   network (the flip form: every comparator puts the smaller key at the lower place, so places >= the load
//                   stand for +inf and their comparators are skipped), perms[b][start + rank] = j, contiguous.  A larger
//                   bucket (it does not occur at the default bucket_rows: the load is 1024 +- 32) is ranked by counting:
//                   256 rows at a time against every tile of CCZ_DRAW_SORT_CAP keys staged in LDS -- quadratic, correct.
// Every index that is dereferenced is checked against its array, so a wrong count could spoil values but not fault.
//
// Multiplicities: the rows are zeroed, then k_draw_counts adds 1 to counts[b][idx_j] for every draw j (one no-return integer
// atomic per draw; integer adds commute).
#include <algorithm>

#include "abi_guard.h"
#include "hip_common.h"
#include "rng_hash.h"

namespace ccz {

namespace {

constexpr int DRAW_CAP = CCZ_DRAW_SORT_CAP;          // rows of a bucket that are sorted in LDS
constexpr int DRAW_HIST = 4096;                      // buckets whose histogram a workgroup keeps in LDS
constexpr int DRAW_STRIPE = 16384;                   // j's per workgroup of the count and scatter passes
constexpr int DRAW_COUNT_STRIPE = 4096;              // draws per workgroup of k_draw_counts
constexpr int64_t DRAW_SCRATCH = int64_t(1) << 26;   // 32-bit words of scratch per launch group (256 MiB)
constexpr int64_t DRAW_MAXBATCH = 65535;             // gridDim.y

__host__ __device__ inline uint64_t draw_stream(uint64_t seed, uint64_t b, uint64_t site) {
  return splitmix64(splitmix64(splitmix64(seed) + b) + site);
}
__device__ __forceinline__ uint64_t draw_key(uint64_t strm, uint64_t j) { return splitmix64(strm ^ splitmix64(j)); }
__device__ __forceinline__ unsigned draw_bucket(uint64_t key, unsigned nb) { return unsigned(__umul64hi(key, uint64_t(nb))); }

template <bool IN_LDS>
__global__ void __launch_bounds__(256) k_draw_count(uint64_t seed, int64_t first, int64_t n, unsigned nb, unsigned* __restrict__ cnt) {
  __shared__ unsigned hist[IN_LDS ? DRAW_HIST : 1];
  const int tid = threadIdx.x;
  const uint64_t strm = draw_stream(seed, uint64_t(first) + blockIdx.y, CCZ_DRAW_SITE_PERM);
  unsigned* mine = cnt + int64_t(blockIdx.y) * nb;
  if (IN_LDS) {
    for (unsigned b = tid; b < nb; b += 256) hist[b] = 0u;
    __syncthreads();
  }
  const int64_t j0 = int64_t(blockIdx.x) * DRAW_STRIPE;
  const int64_t j1 = j0 + DRAW_STRIPE < n ? j0 + DRAW_STRIPE : n;
  for (int64_t j = j0 + tid; j < j1; j += 256) {
    const unsigned b = draw_bucket(draw_key(strm, uint64_t(j)), nb);
    if (IN_LDS) atomicAdd(&hist[b], 1u); else atomicAdd(&mine[b], 1u);
  }
  if (IN_LDS) {
    __syncthreads();
    for (unsigned b = tid; b < nb; b += 256) {
      const unsigned v = hist[b];
      if (v) atomicAdd(&mine[b], v);
    }
  }
}

__global__ void __launch_bounds__(256) k_draw_scan(unsigned nb, unsigned* __restrict__ cnt) {
  __shared__ unsigned s[256];
  const int tid = threadIdx.x;
  unsigned* mine = cnt + int64_t(blockIdx.x) * nb;
  unsigned carry = 0u;
  for (unsigned t0 = 0; t0 < nb; t0 += 1024u) {
    unsigned v[4], sum = 0u;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const unsigned e = t0 + 4u * tid + i;
      v[i] = e < nb ? mine[e] : 0u;
      sum += v[i];
    }
    s[tid] = sum;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {
      const unsigned t = tid >= off ? s[tid - off] : 0u;
      __syncthreads();
      s[tid] += t;
      __syncthreads();
    }
    unsigned run = carry + s[tid] - sum;                 // exclusive: everything before this thread's four
    carry += s[255];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const unsigned e = t0 + 4u * tid + i;
      if (e < nb) mine[e] = run;
      run += v[i];
    }
    __syncthreads();                                     // s is rewritten by the next tile
  }
}

template <bool IN_LDS>
__global__ void __launch_bounds__(256) k_draw_scatter(uint64_t seed, int64_t first, int64_t n, unsigned nb, unsigned* __restrict__ cur,
                                                      int* __restrict__ tmp) {
  __shared__ unsigned hist[IN_LDS ? DRAW_HIST : 1];
  const int tid = threadIdx.x;
  const uint64_t strm = draw_stream(seed, uint64_t(first) + blockIdx.y, CCZ_DRAW_SITE_PERM);
  unsigned* mine = cur + int64_t(blockIdx.y) * nb;
  int* out = tmp + int64_t(blockIdx.y) * n;
  const int64_t j0 = int64_t(blockIdx.x) * DRAW_STRIPE;
  const int64_t j1 = j0 + DRAW_STRIPE < n ? j0 + DRAW_STRIPE : n;
  if (IN_LDS) {
    for (unsigned b = tid; b < nb; b += 256) hist[b] = 0u;
    __syncthreads();
    for (int64_t j = j0 + tid; j < j1; j += 256) atomicAdd(&hist[draw_bucket(draw_key(strm, uint64_t(j)), nb)], 1u);
    __syncthreads();
    for (unsigned b = tid; b < nb; b += 256) {
      const unsigned v = hist[b];
      if (v) hist[b] = atomicAdd(&mine[b], v);           // the stripe's first slot in bucket b
    }
    __syncthreads();
  }
  for (int64_t j = j0 + tid; j < j1; j += 256) {
    const unsigned b = draw_bucket(draw_key(strm, uint64_t(j)), nb);
    const unsigned slot = IN_LDS ? atomicAdd(&hist[b], 1u) : atomicAdd(&mine[b], 1u);
    if (int64_t(slot) < n) out[slot] = int(j);
  }
}

__device__ __forceinline__ void draw_order(uint64_t* keys, int* vals, int i, int l) {
  const uint64_t a = keys[i], b = keys[l];
  if (a > b) {
    keys[i] = b; keys[l] = a;
    const int t = vals[i]; vals[i] = vals[l]; vals[l] = t;
  }
}

__global__ void __launch_bounds__(256) k_draw_sort(uint64_t seed, int64_t first, int64_t n, unsigned nb, const unsigned* __restrict__ cur,
                                                   const int* __restrict__ tmp, int* __restrict__ perms) {
  __shared__ uint64_t keys[DRAW_CAP];
  __shared__ int vals[DRAW_CAP];
  const int tid = threadIdx.x;
  const unsigned bkt = blockIdx.x;
  const uint64_t strm = draw_stream(seed, uint64_t(first) + blockIdx.y, CCZ_DRAW_SITE_PERM);
  const unsigned* mine = cur + int64_t(blockIdx.y) * nb;
  int64_t end = int64_t(mine[bkt]), start = bkt ? int64_t(mine[bkt - 1]) : 0;      // after the scatter a cursor is its bucket's end
  end = end > n ? n : end;
  start = start > end ? end : start;
  const int64_t m = end - start;
  const int* src = tmp + int64_t(blockIdx.y) * n + start;
  int* dst = perms + int64_t(blockIdx.y) * n + start;
  if (m <= DRAW_CAP) {
    const int mm = int(m);
    for (int i = tid; i < mm; i += 256) {
      const int j = src[i];
      keys[i] = draw_key(strm, uint64_t(unsigned(j)));
      vals[i] = j;
    }
    for (int lk = 1; (1 << (lk - 1)) < mm; ++lk) {       // merges of blocks of k = 2^lk places, up to the first k >= mm
      const int k = 1 << lk, half = k >> 1;              // (shifts and masks: a division per pair cost more than the pair)
      __syncthreads();
      for (int t = tid; 2 * t < mm + half; t += 256) {   // (pairs whose lower place is < mm)
        const int blk = t >> (lk - 1), off = t & (half - 1);
        const int i = (blk << lk) + off, l = (blk << lk) + k - 1 - off;
        if (l < mm) draw_order(keys, vals, i, l);
      }
      for (int ld = lk - 2; ld >= 0; --ld) {             // partners d = 2^ld apart
        const int d = 1 << ld;
        __syncthreads();
        for (int t = tid; 2 * t < mm + d; t += 256) {
          const int i = ((t >> ld) << (ld + 1)) + (t & (d - 1)), l = i + d;
          if (l < mm) draw_order(keys, vals, i, l);
        }
      }
    }
    __syncthreads();
    for (int i = tid; i < mm; i += 256) dst[i] = vals[i];
    return;
  }
  // oversize: the place of a row is the number of smaller keys in its bucket (the keys are distinct)
  for (int64_t i0 = 0; i0 < m; i0 += 256) {
    const int64_t i = i0 + tid;
    const int j = i < m ? src[i] : 0;
    const uint64_t key = draw_key(strm, uint64_t(unsigned(j)));
    int64_t rank = 0;
    for (int64_t t0 = 0; t0 < m; t0 += DRAW_CAP) {
      const int len = int(m - t0 < DRAW_CAP ? m - t0 : DRAW_CAP);
      __syncthreads();
      for (int t = tid; t < len; t += 256) keys[t] = draw_key(strm, uint64_t(unsigned(src[t0 + t])));
      __syncthreads();
      for (int t = 0; t < len; ++t) rank += keys[t] < key ? 1 : 0;
    }
    if (i < m && rank < m) dst[rank] = j;
  }
}

__global__ void __launch_bounds__(256) k_draw_counts(uint64_t seed, int64_t first, int64_t n, int* __restrict__ counts) {
  const uint64_t strm = draw_stream(seed, uint64_t(first) + blockIdx.y, CCZ_DRAW_SITE_BOOT);
  int* mine = counts + int64_t(blockIdx.y) * n;
  const int64_t j0 = int64_t(blockIdx.x) * DRAW_COUNT_STRIPE;
  const int64_t j1 = j0 + DRAW_COUNT_STRIPE < n ? j0 + DRAW_COUNT_STRIPE : n;
  for (int64_t j = j0 + threadIdx.x; j < j1; j += 256)
    atomicAdd(&mine[__umul64hi(draw_key(strm, uint64_t(j)), uint64_t(n))], 1);       // (key * n) >> 64 < n
}

// The checks both entries make, in the order of check_two_views (resample_dev.h): counts, pointers, what is not supported.
void check_draw(const char* name, const char* counted, bool counts_ok, bool pointer, int64_t n) {
  if (!counts_ok) fail(CCZ_EINVAL, "%s: %s", name, counted);
  if (!pointer) fail(CCZ_EINVAL, "%s: null pointer", name);
  if (n >= (int64_t(1) << 31)) fail(CCZ_EUNSUP, "%s: fewer than 2^31 rows, got %lld", name, (long long)n);
}

void draw_permutations_impl(ccz_ctx* c, int64_t n, int64_t nperm, uint64_t seed, int64_t first, int64_t bucket_rows, int32_t* perms) {
  check_draw("draw_permutations", "n and nperm must be positive, first and bucket_rows not negative",
             n >= 1 && nperm >= 1 && first >= 0 && bucket_rows >= 0, perms != nullptr, n);
  const int64_t rows = bucket_rows ? bucket_rows : CCZ_DRAW_BUCKET_ROWS;
  const unsigned nb = unsigned((n + rows - 1) / rows);   // <= n < 2^31
  const unsigned nstripe = unsigned((n + DRAW_STRIPE - 1) / DRAW_STRIPE);
  // scratch of one permutation: nb cursors and the n rows in bucket order; a launch group is as many permutations as fit
  const int64_t per = n + int64_t(nb);
  const int64_t cap = std::min(nperm, std::max<int64_t>(1, std::min<int64_t>(DRAW_SCRATCH / per, DRAW_MAXBATCH)));
  PoolBuf<unsigned> scratch(c, cap * per);
  unsigned* cur = scratch.get();
  int* tmp = reinterpret_cast<int*>(scratch.get() + cap * int64_t(nb));
  const bool in_lds = nb <= unsigned(DRAW_HIST);
  for (int64_t b0 = 0; b0 < nperm; b0 += cap) {
    const unsigned g = unsigned(std::min(cap, nperm - b0));
    zero(c, cur, size_t(g) * nb * sizeof(unsigned));
    if (in_lds) hipLaunchKernelGGL(k_draw_count<true>, dim3(nstripe, g), dim3(256), 0, stream(c), seed, first + b0, n, nb, cur);
    else hipLaunchKernelGGL(k_draw_count<false>, dim3(nstripe, g), dim3(256), 0, stream(c), seed, first + b0, n, nb, cur);
    CCZ_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_draw_scan, dim3(g), dim3(256), 0, stream(c), nb, cur);
    CCZ_LAUNCH_CHECK();
    if (in_lds) hipLaunchKernelGGL(k_draw_scatter<true>, dim3(nstripe, g), dim3(256), 0, stream(c), seed, first + b0, n, nb, cur, tmp);
    else hipLaunchKernelGGL(k_draw_scatter<false>, dim3(nstripe, g), dim3(256), 0, stream(c), seed, first + b0, n, nb, cur, tmp);
    CCZ_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_draw_sort, dim3(nb, g), dim3(256), 0, stream(c), seed, first + b0, n, nb, cur, tmp, perms + b0 * n);
    CCZ_LAUNCH_CHECK();
  }
}

void draw_counts_impl(ccz_ctx* c, int64_t n, int64_t nboot, uint64_t seed, int64_t first, int32_t* counts) {
  check_draw("draw_counts", "n and nboot must be positive, first not negative", n >= 1 && nboot >= 1 && first >= 0, counts != nullptr, n);
  const unsigned nstripe = unsigned((n + DRAW_COUNT_STRIPE - 1) / DRAW_COUNT_STRIPE);
  zero(c, counts, size_t(nboot) * size_t(n) * sizeof(int32_t));
  for (int64_t b0 = 0; b0 < nboot; b0 += DRAW_MAXBATCH) {
    const unsigned g = unsigned(std::min(DRAW_MAXBATCH, nboot - b0));
    hipLaunchKernelGGL(k_draw_counts, dim3(nstripe, g), dim3(256), 0, stream(c), seed, first + b0, n, counts + b0 * n);
    CCZ_LAUNCH_CHECK();
  }
}

}  // namespace

}  // namespace ccz

extern "C" {

int ccz_draw_permutations(ccz_handle h, int64_t n, int64_t nperm, uint64_t seed, int64_t first, int64_t bucket_rows, int32_t* perms_dev) {
  CCZ_GUARD(h, ccz::draw_permutations_impl(h, n, nperm, seed, first, bucket_rows, perms_dev));
}

int ccz_draw_counts(ccz_handle h, int64_t n, int64_t nboot, uint64_t seed, int64_t first, int32_t* counts_dev) {
  CCZ_GUARD(h, ccz::draw_counts_impl(h, n, nboot, seed, first, counts_dev));
}

}  // extern "C"
