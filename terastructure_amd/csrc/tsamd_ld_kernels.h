// tsamd_ld: structure-adjusted linkage disequilibrium of nearby listed locations over the shard's individuals (gfx950).
//
// With q(n, j) = sum_k Ebeta[j][k] Etheta[n][k], z = (y - 2q) / sqrt(2q (1 - q)) and m = 1 for every stored entry (both 0 where
// the code is 01: ld_terms, tsamd_ld_plan.h), num = Z^T Z and cnt = M^T M over the individuals, for the pairs of list positions
// at most `window` apart: r = num / cnt is the r_S of Mangin et al. 2012 on what the engine holds.  It is tsamd_kinship's
// product in the other direction: rows are locations, the reduction runs over the individuals, and only a band of the matrix is
// formed.  Reads the state, writes none of it.
//
// ts_ld_resid<K> -- the only K-dependent part; every entry is computed once per chunk that reads it.  A workgroup takes
// kLdResidIndivs = 256 individuals (one per thread) and kLdResidBatch = 16 locations.  The 16 x 64 bytes of the 2-bit columns
// are read once, four bytes per thread and coalesced along the individuals -- the direction the columns are stored in -- and
// kept in LDS; the thread gathers its individual's gamma once and normalises it as tsamd_get_theta does (gamma / sum in
// ascending k; K = 1..32 in registers, the run-time-K form divides per use); Ebeta = lambda0 / (lambda0 + lambda1) of the 16
// locations is staged in LDS as ts_kin_resid does.  The thread's 16 z go to an LDS tile [256][17] and its 16 m to a bit mask;
// the workgroup then writes Z and M [individual of the block][location] with the location contiguous: 16 lanes per row of 128
// bytes.  Rows of individuals past the shard's or the block's end (the zero tail of the last k-step) and columns past the
// listed locations (padding to whole tiles) are written as zeros, so every entry of [rows4][lpad] is written by every launch.
//
// ts_ld_syrk -- K-independent, one instantiation: ts_kin_syrk's tile arithmetic (a workgroup of 4 waves owns the 64 x 64 tile of
// BOTH products for its segment's individuals, wave w the 32 x 32 quarter (w >> 1, w & 1) as 2 x 2 blocks of
// v_mfma_f64_16x16x4_f64; operands of 4 k-steps staged through LDS, the next stage requested before the current stage's
// arithmetic; the f64 read-out map) on the band's tile pairs (ld_pair) and on operands whose reduction index is the individual.
// A kernel of its own beside ts_kin_syrk, whose generated code stays as it is.  The count is the second fp64 product, of the
// 0 / 1 masks: exact below 2^53.
//
// ts_ld_finish adds a tile's segments in ascending order onto the chunk's accumulators, block after block; ts_ld_band writes
// the chunk's rows of the band, the doubles as num and the counts as uint32.
//
// Summation order (no floating-point atomics): inside a segment the MFMA accumulates the k-steps in the shard's order; segments
// ascending; blocks ascending.  Two identical calls give identical bits.  A pair's num depends on the chunk, block and segment
// boundaries by rounding only; cnt is exact.
#pragma once
#include "tsamd_device.h"
#include "tsamd_ld_plan.h"

namespace tsamd {

// grid (individual tiles of 256 over rows4, batches of 16 columns over lpad)
template <int KC>
__global__ __launch_bounds__(256) void ts_ld_resid(const LdArgs a) {
  constexpr int KMAX = KC > 0 ? KC : TSAMD_MAX_K;
  constexpr uint32_t NB = kLdResidBatch, NI = kLdResidIndivs, ZLD = NB + 1u;
  static_assert(NI == kLdBlock && NB * (NI / 4u) == 4u * kLdBlock && NB == 16u, "a thread reads four bytes of the 16 x 64 the workgroup needs");
  __shared__ double s_eb[NB * KMAX];
  __shared__ double s_z[NI * ZLD];
  __shared__ uint32_t s_code[NB * (NI / 16u)];  // [location][16 words of 16 individuals]
  __shared__ uint32_t s_mask[NI];
  const uint32_t K = KC > 0 ? (uint32_t)KC : a.K;
  const uint32_t tid = threadIdx.x;
  const uint32_t r0 = blockIdx.x * NI;                     // first row (individual of the block) of this workgroup
  const uint32_t c0 = blockIdx.y * NB;                     // first column
  const uint32_t nl = c0 < a.ncols ? min(NB, a.ncols - c0) : 0u;  // listed locations among its columns; the others are padding
  const uint32_t n = a.ind0 + r0 + tid;                    // the thread's individual
  const bool live = r0 + tid < a.blen && n < a.n_local;

  for (uint32_t e = tid; e < nl * K; e += kLdBlock) {
    const uint32_t j = e / K, k = e - j * K;
    const double2 l = reinterpret_cast<const double2 *>(a.lam)[(size_t)a.locs[c0 + j] * K + k];
    double s = 0.0;  // (as ts_export_loc adds them)
    s += l.x;
    s += l.y;
    s_eb[e] = l.x / s;
  }
  {  // the columns' bytes: word w of location j holds individuals ind0 + r0 + 16 w .. + 15 (ind0 and r0 are multiples of 4).
     // A block that starts on a multiple of 16 individuals -- every block of the default geometry -- reads it as one dword
     // (colstride is a multiple of 4, so an aligned word lies inside the column or past it); otherwise the word may straddle
     // the column's end, and each of its bytes that the column holds is read, the others stay 01
    const uint32_t j = tid >> 4, w = tid & 15u;
    const uint64_t byte0 = (uint64_t)((a.ind0 + r0) >> 2) + 4u * w;
    uint32_t word = 0x55555555u;  // 01: no term
    if (j < nl && byte0 < a.colstride) {
      const uint8_t *src = a.bed + (size_t)a.locs[c0 + j] * a.colstride + byte0;
      if ((byte0 & 3u) == 0u) {
        word = *reinterpret_cast<const uint32_t *>(src);
      } else {
#pragma unroll
        for (uint32_t b = 0; b < 4u; ++b)
          if (byte0 + b < a.colstride) word = (word & ~(0xffu << (8u * b))) | ((uint32_t)src[b] << (8u * b));
      }
    }
    s_code[j * (NI / 16u) + w] = word;
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

  uint32_t mask = 0u;
  for (uint32_t j = 0; j < NB; ++j) {
    double z = 0.0, m = 0.0;
    if (live && j < nl) {
      const uint32_t code = (s_code[j * (NI / 16u) + (tid >> 4)] >> (2u * (tid & 15u))) & 3u;
      double q = 0.0;
      if constexpr (KC > 0) {
#pragma unroll
        for (int k = 0; k < KC; ++k) q = fma(s_eb[j * KC + k], th[k], q);
      } else {
        for (uint32_t k = 0; k < K; ++k) q = fma(s_eb[j * K + k], a.gam[(size_t)k * a.npad + n] / gsum, q);
      }
      ld_terms(q, code, &z, &m);
    }
    s_z[tid * ZLD + j] = z;
    mask |= (m != 0.0 ? 1u : 0u) << j;
  }
  s_mask[tid] = mask;
  __syncthreads();

  // the tile, location contiguous: element e is row e / 16, column e % 16 (c0 + NB <= lpad: lpad is a multiple of 64)
#pragma unroll 4
  for (uint32_t e = tid; e < NI * NB; e += kLdBlock) {
    const uint32_t row = e / NB, col = e % NB;
    if (r0 + row >= a.rows4) break;  // (rows ascend with e)
    const size_t at = (size_t)(r0 + row) * a.lpad + c0 + col;
    a.z[at] = s_z[row * ZLD + col];
    a.m[at] = (double)((s_mask[row] >> col) & 1u);
  }
}

typedef double ld_f64x4 __attribute__((ext_vector_type(4)));

// grid (pairs of this launch, segments).  Z and M are [steps * 4][lpad]; seg_steps k-steps per segment, `steps` in the block;
// rows / nt / ov name the chunk's band of tile pairs (ld_pair).
__global__ __launch_bounds__(256) void ts_ld_syrk(const double *__restrict__ Z, const double *__restrict__ M, uint32_t lpad, uint32_t rows, uint32_t nt,
                                                  uint32_t ov, uint32_t pair0, uint32_t steps, uint32_t seg_steps, double *__restrict__ part) {
  constexpr uint32_t T = kLdTile, ROWS = kLdStageSteps * kLdStep;  // 16 individuals per stage
  constexpr uint32_t LD = T + 16u;                                 // row stride in doubles: the 4 rows of a k-step fall on distinct banks
  constexpr uint32_t PER = 4u * ROWS * T / 2u / kLdBlock;          // double2 loads per thread and stage: 8
  static_assert(T == 64u && kLdBlock == 256u && 2u * kLdBlock == ROWS * T / 2u, "2 x 2 waves of 32 x 32; an array of a stage is two loads per thread");
  __shared__ double sh[4][ROWS][LD];  // z of tile ti, z of tile tj, m of tile ti, m of tile tj: 40 KB

  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const LdPair pr = ld_pair(pair0 + blockIdx.x, rows, nt, ov);
  const uint32_t ti = pr.ti, tj = pr.tj;
  const uint32_t seg = blockIdx.y;
  const uint32_t st_begin = seg * seg_steps, st_end = min(steps, st_begin + seg_steps);
  const uint32_t wr = (wave >> 1) * 32u, wc = (wave & 1u) * 32u;
  const uint32_t lk = lane >> 4, li = lane & 15u;

  ld_f64x4 acc[2][2][2];  // [product][block row][block column]
#pragma unroll
  for (int p = 0; p < 2; ++p)
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) acc[p][i][j] = ld_f64x4{0.0, 0.0, 0.0, 0.0};

  // load u of a thread: array u / 2, then row and double2 column by thread; rows past the segment's end are not loaded (zeros)
  double2 pre[PER];
  auto fetch = [&](uint32_t st0) {
    const uint32_t nrows = min(kLdStageSteps, st_end - st0) * kLdStep;
#pragma unroll
    for (uint32_t u = 0; u < PER; ++u) {
      const uint32_t arr = u >> 1, rem = (u & 1u) * kLdBlock + tid, row = rem / (T / 2u), c2 = rem % (T / 2u);  // (two loads per array)
      const double *src = (arr & 2u) ? M : Z;
      const uint32_t tile = (arr & 1u) ? tj : ti;
      pre[u] = row < nrows ? *reinterpret_cast<const double2 *>(src + (size_t)(st0 * kLdStep + row) * lpad + tile * T + 2u * c2)
                           : double2{0.0, 0.0};
    }
  };
  auto stage = [&]() {
#pragma unroll
    for (uint32_t u = 0; u < PER; ++u) {
      const uint32_t arr = u >> 1, rem = (u & 1u) * kLdBlock + tid, row = rem / (T / 2u), c2 = rem % (T / 2u);
      *reinterpret_cast<double2 *>(&sh[arr][row][2u * c2]) = pre[u];
    }
  };

  if (st_begin < st_end) fetch(st_begin);
  for (uint32_t st0 = st_begin; st0 < st_end; st0 += kLdStageSteps) {
    __syncthreads();  // (the previous stage has been read)
    stage();
    __syncthreads();
    if (st0 + kLdStageSteps < st_end) fetch(st0 + kLdStageSteps);
#pragma unroll
    for (uint32_t kk = 0; kk < kLdStageSteps; ++kk) {  // (k-steps past the segment's end multiply zeros)
      const uint32_t row = kk * kLdStep + lk;
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

// grid (pairs of this launch): a tile's segments, in ascending order, onto the chunk's accumulators [pair][2][T * T]
__global__ __launch_bounds__(256) void ts_ld_finish(const double *__restrict__ part, uint32_t nseg, uint32_t pair0, double *__restrict__ acc) {
  constexpr uint32_t T = kLdTile;
  double *dst = acc + (size_t)(pair0 + blockIdx.x) * (2u * T * T);
  for (uint32_t e = threadIdx.x; e < 2u * T * T; e += kLdBlock) {
    double v = dst[e];
    for (uint32_t g = 0; g < nseg; ++g) v += part[((size_t)g * gridDim.x + blockIdx.x) * (2u * T * T) + e];
    dst[e] = v;
  }
}

// grid (columns of the band / 256 rounded up, the chunk's len rows): row i, column d is the pair of columns (i, i + d) of the
// chunk's Z; 0 where i + d is past the listed locations (ncols: the chunk's and its overlap's)
__global__ __launch_bounds__(256) void ts_ld_band(const double *__restrict__ acc, uint32_t rows, uint32_t nt, uint32_t ov, uint32_t ncols, uint32_t window,
                                                  double *__restrict__ num, uint32_t *__restrict__ cnt) {
  constexpr uint32_t T = kLdTile;
  const uint32_t i = blockIdx.y, d = blockIdx.x * kLdBlock + threadIdx.x;
  if (d > window) return;
  const uint32_t j = i + d;
  double v = 0.0, c = 0.0;
  if (j < ncols) {
    const uint32_t ti = i / T, tj = j / T;  // (tj - ti <= ov, tj < nt: ld_overlap_tiles)
    const double *t = acc + (size_t)(ld_row_first(ti, rows, nt, ov) + (tj - ti)) * (2u * T * T) + (i % T) * T + j % T;
    v = t[0];
    c = t[T * T];
  }
  const size_t at = (size_t)i * (window + 1u) + d;
  num[at] = v;
  cnt[at] = (uint32_t)c;
}

}  // namespace tsamd
