// tsamd_kinship: admixture-adjusted pairwise relatedness of m listed individuals over a list of locations (gfx950).
//
// With q(n, j) = sum_k Ebeta[j][k] Etheta[n][k], r = y - 2q and s = sqrt(q (1 - q)) for every stored entry (both 0 where the
// code is 01: kin_terms, tsamd_kin_plan.h), num = R^T R and den = S^T S over the listed locations and kin = num / (4 den): the
// REAP estimator (Thornton et al. 2012) on what the engine holds.  Reads the state, writes none of it.
//
// ts_kin_resid<K> -- the only K-dependent part; every entry is computed once, not once per partner tile.  One thread per
// listed individual (row): it gathers the individual's gamma once and normalises it as tsamd_get_theta does (gamma / sum in
// ascending k; K = 1..32 in registers, the run-time-K form divides per use), a workgroup stages Ebeta = lambda0 / (lambda0 +
// lambda1) of kKinResidBatch locations in LDS as ts_loglik does, a thread reads the byte of the 2-bit column that holds its
// individual and writes r and s to two arrays [len4][mpad], row (individual) contiguous.  Padding rows (m .. mpad) and the
// chunk's tail (len .. len4, whole k-steps) are written as zeros.
//
// ts_kin_syrk -- K-independent, one instantiation: two symmetric rank-L updates on the matrix cores.  Grid (tile pairs ti <=
// tj, segments); a workgroup of 4 waves owns the T x T tile (T = kKinTile = 64) of BOTH products for its segment's locations,
// wave w the 32 x 32 quarter (w >> 1, w & 1) as 2 x 2 blocks of v_mfma_f64_16x16x4_f64: 8 accumulators of 4 doubles, 64
// registers.  A k-step covers 4 locations: the A operand of lane l is r (s for the second product) of location 4 step + (l >> 4)
// at individual l & 15 of the block row, the B operand the same of the partner tile, one double per lane.  The operands of
// kKinStageSteps k-steps (16 locations: 4 arrays x 16 rows x 64 doubles = 32 KB) go through LDS so that the four waves share
// them; the next stage's rows are requested from memory before the current stage's arithmetic.  C read-out: lane l holds, in
// register g of a block, row (l >> 4) + 4 g and column l & 15 -- the f64 map, not the f32 one.
// Per stage and wave: 16 ds_read_b64 against 32 MFMAs of 2048 flops.  Per tile pair and location the workgroup reads 4 x 64
// doubles (2 KB) for 2 x 2 x 64 x 64 = 16 384 flops: 8 flop per byte from L2 / HBM (the r / s scratch of a chunk is at most
// 256 MB and is re-read by every tile pair).  T = 128 would double that at 256 accumulator registers per lane; the resource
// table (profiles/r06_kernel_resources.txt) shows T = 64 at 0 scratch with room for two workgroups per compute unit.
//
// ts_kin_finish adds a tile's segments in ascending order onto the call's accumulators [mpad][mpad], chunk after chunk;
// ts_kin_mirror copies the upper triangle onto the lower after the last chunk and ts_kin_form divides.
//
// Summation order (no floating-point atomics): inside a segment the MFMA accumulates the k-steps in listed order; segments
// ascending; chunks ascending.  Two identical calls give identical bits.  A pair's value depends on the segment and chunk
// boundaries (hence on m, which sets them) by rounding only.
#pragma once
#include "tsamd_device.h"
#include "tsamd_kin_plan.h"

namespace tsamd {

template <int KC>
__global__ __launch_bounds__(256) void ts_kin_resid(const KinArgs a) {
  constexpr int KMAX = KC > 0 ? KC : TSAMD_MAX_K;
  __shared__ double s_eb[kKinResidBatch * KMAX];
  __shared__ uint32_t s_loc[kKinResidBatch];
  const uint32_t K = KC > 0 ? (uint32_t)KC : a.K;
  const uint32_t tid = threadIdx.x;
  const uint32_t row = blockIdx.x * kKinBlock + tid;
  const uint32_t b0 = blockIdx.y * kKinResidBatch;               // first row (location of the chunk) of this workgroup
  const uint32_t nb = min(kKinResidBatch, a.len4 - b0);          // rows it writes ...
  const uint32_t nl = b0 < a.len ? min(nb, a.len - b0) : 0u;     // ... of which listed locations; the others are the zero tail
  const uint32_t n = row < a.mpad ? a.ids[row] : 0xffffffffu;
  const bool live = n != 0xffffffffu;

  if (tid < nl) s_loc[tid] = a.locs[b0 + tid];
  for (uint32_t e = tid; e < nl * K; e += kKinBlock) {
    const uint32_t j = e / K, k = e - j * K;
    const double2 l = reinterpret_cast<const double2 *>(a.lam)[(size_t)a.locs[b0 + j] * K + k];
    double s = 0.0;  // (as ts_export_loc adds them)
    s += l.x;
    s += l.y;
    s_eb[e] = l.x / s;
  }

  // normalised theta of the thread's individual, exactly what tsamd_get_theta returns: gamma / (sum in ascending k)
  double th[KC > 0 ? KC : 1];
  double gsum = 0.0;
  if constexpr (KC > 0) {
#pragma unroll
    for (int k = 0; k < KC; ++k) {
      th[k] = live ? a.gam[(size_t)k * a.npad + n] : 1.0;
      gsum += th[k];
    }
#pragma unroll
    for (int k = 0; k < KC; ++k) th[k] = th[k] / gsum;
  } else {
    for (uint32_t k = 0; k < K; ++k) gsum += live ? a.gam[(size_t)k * a.npad + n] : 1.0;
  }
  __syncthreads();
  if (row >= a.mpad) return;

  const uint8_t *mybyte = a.bed + (live ? (n >> 2) : 0u);
  const uint32_t shift = 2u * (n & 3u);
  for (uint32_t j = 0; j < nb; ++j) {
    double r = 0.0, s = 0.0;
    if (live && j < nl) {
      const uint32_t code = ((uint32_t)mybyte[(size_t)s_loc[j] * a.colstride] >> shift) & 3u;
      double q = 0.0;
      if constexpr (KC > 0) {
#pragma unroll
        for (int k = 0; k < KC; ++k) q = fma(s_eb[j * KC + k], th[k], q);
      } else {
        for (uint32_t k = 0; k < K; ++k) q = fma(s_eb[j * K + k], a.gam[(size_t)k * a.npad + n] / gsum, q);
      }
      kin_terms(q, code, &r, &s);
    }
    a.r[(size_t)(b0 + j) * a.mpad + row] = r;
    a.s[(size_t)(b0 + j) * a.mpad + row] = s;
  }
}

typedef double kin_f64x4 __attribute__((ext_vector_type(4)));

// grid (pairs of this launch, segments).  seg_steps k-steps per segment, `steps` in the chunk.
__global__ __launch_bounds__(256) void ts_kin_syrk(const double *__restrict__ R, const double *__restrict__ S, uint32_t mpad, uint32_t ntiles,
                                                   uint32_t pair0, uint32_t steps, uint32_t seg_steps, double *__restrict__ part) {
  constexpr uint32_t T = kKinTile, ROWS = kKinStageSteps * kKinStep;  // 16 locations per stage
  constexpr uint32_t LD = T + 16u;                                    // row stride in doubles: the 4 rows of a k-step fall on distinct banks
  constexpr uint32_t PER = 4u * ROWS * T / 2u / kKinBlock;            // double2 loads per thread and stage: 8
  static_assert(T == 64u && kKinBlock == 256u && 2u * kKinBlock == ROWS * T / 2u, "2 x 2 waves of 32 x 32; an array of a stage is two loads per thread");
  __shared__ double sh[4][ROWS][LD];  // r of tile ti, r of tile tj, s of tile ti, s of tile tj: 40 KB

  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const KinPair pr = kin_pair(pair0 + blockIdx.x, ntiles);
  const uint32_t ti = pr.ti, tj = pr.tj;
  const uint32_t seg = blockIdx.y;
  const uint32_t st_begin = seg * seg_steps, st_end = min(steps, st_begin + seg_steps);
  const uint32_t wr = (wave >> 1) * 32u, wc = (wave & 1u) * 32u;
  const uint32_t lk = lane >> 4, li = lane & 15u;

  kin_f64x4 acc[2][2][2];  // [product][block row][block column]
#pragma unroll
  for (int p = 0; p < 2; ++p)
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) acc[p][i][j] = kin_f64x4{0.0, 0.0, 0.0, 0.0};

  // load u of a thread: array u / 2, then row and double2 column by thread; rows past the segment's end are not loaded (zeros)
  double2 pre[PER];
  auto fetch = [&](uint32_t st0) {
    const uint32_t nrows = min(kKinStageSteps, st_end - st0) * kKinStep;
#pragma unroll
    for (uint32_t u = 0; u < PER; ++u) {
      const uint32_t arr = u >> 1, rem = (u & 1u) * kKinBlock + tid, row = rem / (T / 2u), c2 = rem % (T / 2u);  // (two loads per array)
      const double *src = (arr & 2u) ? S : R;
      const uint32_t tile = (arr & 1u) ? tj : ti;
      pre[u] = row < nrows ? *reinterpret_cast<const double2 *>(src + (size_t)(st0 * kKinStep + row) * mpad + tile * T + 2u * c2)
                           : double2{0.0, 0.0};
    }
  };
  auto stage = [&]() {
#pragma unroll
    for (uint32_t u = 0; u < PER; ++u) {
      const uint32_t arr = u >> 1, rem = (u & 1u) * kKinBlock + tid, row = rem / (T / 2u), c2 = rem % (T / 2u);
      *reinterpret_cast<double2 *>(&sh[arr][row][2u * c2]) = pre[u];
    }
  };

  if (st_begin < st_end) fetch(st_begin);
  for (uint32_t st0 = st_begin; st0 < st_end; st0 += kKinStageSteps) {
    __syncthreads();  // (the previous stage has been read)
    stage();
    __syncthreads();
    if (st0 + kKinStageSteps < st_end) fetch(st0 + kKinStageSteps);
#pragma unroll
    for (uint32_t kk = 0; kk < kKinStageSteps; ++kk) {  // (k-steps past the segment's end multiply zeros)
      const uint32_t row = kk * kKinStep + lk;
#pragma unroll
      for (int p = 0; p < 2; ++p) {
        double av[2], bv[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) av[i] = sh[2 * p][row][wr + 16u * i + li], bv[i] = sh[2 * p + 1][row][wc + 16u * i + li];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j) acc[p][i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[i], bv[j], acc[p][i][j], 0, 0, 0);
      }
    }
  }

  // the f64 C map: register g of lane l is row (l >> 4) + 4 g, column l & 15 of its 16 x 16 block
  double *out = part + ((size_t)seg * gridDim.x + blockIdx.x) * (2u * T * T);
#pragma unroll
  for (int p = 0; p < 2; ++p)
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const uint32_t row = wr + 16u * i + lk + 4u * g, col = wc + 16u * j + li;
          out[(size_t)p * T * T + row * T + col] = acc[p][i][j][g];
        }
}

// grid (pairs of this launch): a tile's segments, in ascending order, onto the call's accumulators
__global__ __launch_bounds__(256) void ts_kin_finish(const double *__restrict__ part, uint32_t nseg, uint32_t mpad, uint32_t ntiles, uint32_t pair0,
                                                     double *__restrict__ num, double *__restrict__ den) {
  constexpr uint32_t T = kKinTile;
  const KinPair pr = kin_pair(pair0 + blockIdx.x, ntiles);
  for (uint32_t e = threadIdx.x; e < 2u * T * T; e += kKinBlock) {
    const uint32_t p = e / (T * T), rem = e % (T * T), row = rem / T, col = rem % T;
    double *dst = (p ? den : num) + (size_t)(pr.ti * T + row) * mpad + pr.tj * T + col;
    double v = *dst;
    for (uint32_t g = 0; g < nseg; ++g) v += part[((size_t)g * gridDim.x + blockIdx.x) * (2u * T * T) + e];
    *dst = v;
  }
}

// x[b][a] = x[a][b] for a < b: the lower triangle is a copy of the upper.  grid (mpad / 256 rounded up, mpad, 2)
__global__ __launch_bounds__(256) void ts_kin_mirror(double *num, double *den, uint32_t mpad) {
  double *x = blockIdx.z ? den : num;
  const uint32_t b = blockIdx.y, a = blockIdx.x * kKinBlock + threadIdx.x;
  if (a < b) x[(size_t)b * mpad + a] = x[(size_t)a * mpad + b];
}

// kin over num: num / (4 den), 0 where den == 0
__global__ __launch_bounds__(256) void ts_kin_form(double *num, const double *den, size_t count) {
  const size_t i = (size_t)blockIdx.x * kKinBlock + threadIdx.x;
  if (i >= count) return;
  const double d = den[i];
  num[i] = d != 0.0 ? num[i] / (4.0 * d) : 0.0;
}

}  // namespace tsamd
