// tsamd_theta_info: the information matrices of theta, individual by individual, over a list of locations (gfx950).
//
// With lambda held fixed the log-likelihood of individual n in theta is sum_j y log q + (2 - y) log(1 - q), q(n, j) = sum_k
// Ebeta[j][k] theta[n][k]; its negative Hessian is H_n = sum_j c(n, j) b_j b_j^T with b_j = Ebeta[j][.], c_obs = y / q^2 +
// (2 - y) / (1 - q)^2 (observed) or c_exp = 2 / (q (1 - q)) (expected) -- info_terms, tsamd_info_plan.h; both 0 where the code is
// 01.  Over a block of individuals that is H = C BB: C (individuals x locations), BB (locations x P = K (K + 1) / 2) the packed
// outer products of the Ebeta rows; the reduction runs over the locations.  Reads the state, writes none of it.
//
// ts_info_coef<K> -- the only K-dependent sweep; every entry is computed once.  A workgroup takes kInfoCoefIndivs = 256
// rows (one per thread) and kInfoCoefBatch = 16 locations.  A contiguous block (ids == NULL) reads the 16 x 64 bytes of the
// 2-bit columns once, four bytes per thread and coalesced along the individuals, into LDS, exactly as ts_ld_resid does (an
// aligned dword where the block starts on a multiple of 16 individuals, otherwise byte by byte up to the column's last byte);
// a gathered block (ids != NULL) reads the byte that holds its individual, as ts_kin_resid does.  The thread gathers its
// individual's gamma once and normalises it as tsamd_get_theta does (gamma / sum in ascending k; K = 1..32 in registers, the
// run-time-K form divides per use); Ebeta = lambda0 / (lambda0 + lambda1) of the 16 locations is staged in LDS as ts_ld_resid
// does.  c_obs and c_exp go to [len4][bpad], the individual contiguous: the product's first operand with the reduction index
// outermost, written coalesced without a transpose.  Rows of locations past the chunk's end (the zero tail of the last k-step)
// and columns of individuals past the block's end (padding to whole tiles) are written as zeros, so every entry of
// [len4][bpad] is written by every launch.
//
// ts_info_outer -- BB[j][p] = Ebeta[j][a] Ebeta[j][b] for the chunk's locations, p = (a <= b) packed; columns P .. ppad and the
// rows of the zero tail are zero.  Run-time K, a workgroup per location and 256 columns.
//
// ts_info_gemm -- K-independent, one instantiation: ts_kin_syrk's tile arithmetic and read-out map with two different operands.
// A workgroup of 4 waves owns the 64 (individuals) x 64 (packed columns) tile of BOTH products for its segment's locations, wave
// w the 32 x 32 quarter (w >> 1, w & 1) as 2 x 2 blocks of v_mfma_f64_16x16x4_f64.  The A operand of lane l is c (obs or exp) of
// location 4 step + (l >> 4) at individual l & 15 of the block row, the B operand BB of the same location at column l & 15 of the
// block column; the two products share B, which is staged once: 3 arrays x 16 rows x 64 doubles per stage against 4 for two
// separate products.  The next stage is requested from memory before the current stage's arithmetic.  A kernel of its own
// beside ts_kin_syrk and ts_ld_syrk, whose generated code stays as it is.
//
// ts_info_finish adds a tile's segments in ascending order onto the block's accumulators, chunk after chunk; ts_info_rows writes
// the block's rows unpadded.
//
// Summation order (no floating-point atomics): inside a segment the MFMA accumulates the k-steps in listed order; segments
// ascending; chunks ascending.  Two identical calls give identical bits, and an individual's row does not depend on the rows
// beside it: the same bits wherever it stands in a list of the same length.
#pragma once
#include "tsamd_device.h"
#include "tsamd_info_plan.h"

namespace tsamd {

// grid (tiles of 256 rows over bpad, batches of 16 locations over len4)
template <int KC>
__global__ __launch_bounds__(256) void ts_info_coef(const InfoArgs a) {
  constexpr int KMAX = KC > 0 ? KC : TSAMD_MAX_K;
  constexpr uint32_t NB = kInfoCoefBatch, NI = kInfoCoefIndivs;
  static_assert(NI == kInfoBlock && NB * (NI / 4u) == 4u * kInfoBlock && NB == 16u, "a thread reads four bytes of the 16 x 64 the workgroup needs");
  __shared__ double s_eb[NB * KMAX];
  __shared__ uint32_t s_code[NB * (NI / 16u)];  // [location][16 words of 16 individuals] (a contiguous block)
  __shared__ uint32_t s_loc[NB];
  const uint32_t K = KC > 0 ? (uint32_t)KC : a.K;
  const uint32_t tid = threadIdx.x;
  const uint32_t r0 = blockIdx.x * NI;                           // first row of this workgroup
  const uint32_t row = r0 + tid;
  const uint32_t c0 = blockIdx.y * NB;                           // first location of the chunk of this workgroup
  const uint32_t nb = min(NB, a.len4 - c0);                      // rows of c it writes ...
  const uint32_t nl = c0 < a.len ? min(nb, a.len - c0) : 0u;     // ... of which listed locations; the others are the zero tail
  const bool gathered = a.ids != nullptr;
  uint32_t n = 0xffffffffu;                                      // the thread's individual (local)
  if (row < a.blen) n = gathered ? a.ids[row] : a.ind0 + row;
  const bool live = n != 0xffffffffu && n < a.n_local;

  if (tid < nl) s_loc[tid] = a.locs[c0 + tid];
  for (uint32_t e = tid; e < nl * K; e += kInfoBlock) {
    const uint32_t j = e / K, k = e - j * K;
    const double2 l = reinterpret_cast<const double2 *>(a.lam)[(size_t)a.locs[c0 + j] * K + k];
    double s = 0.0;  // (as ts_export_loc adds them)
    s += l.x;
    s += l.y;
    s_eb[e] = l.x / s;
  }
  if (!gathered) {
    // the columns' bytes: word w of location j holds individuals ind0 + r0 + 16 w .. + 15 (ind0 and r0 are multiples of 4).
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
  if (row >= a.bpad) return;

  const uint8_t *mybyte = a.bed + (live ? (n >> 2) : 0u);
  const uint32_t shift = 2u * (n & 3u);
  for (uint32_t j = 0; j < nb; ++j) {
    double co = 0.0, ce = 0.0;
    if (live && j < nl) {
      const uint32_t code = gathered ? ((uint32_t)mybyte[(size_t)s_loc[j] * a.colstride] >> shift) & 3u
                                     : (s_code[j * (NI / 16u) + (tid >> 4)] >> (2u * (tid & 15u))) & 3u;
      double q = 0.0;
      if constexpr (KC > 0) {
#pragma unroll
        for (int k = 0; k < KC; ++k) q = fma(s_eb[j * KC + k], th[k], q);
      } else {
        for (uint32_t k = 0; k < K; ++k) q = fma(s_eb[j * K + k], a.gam[(size_t)k * a.npad + n] / gsum, q);
      }
      info_terms(q, code, &co, &ce);
    }
    a.cobs[(size_t)(c0 + j) * a.bpad + row] = co;
    a.cexp[(size_t)(c0 + j) * a.bpad + row] = ce;
  }
}

// grid (ppad / 256 rounded up, len4): row j of BB
__global__ __launch_bounds__(256) void ts_info_outer(const InfoArgs a) {
  __shared__ double s_eb[TSAMD_MAX_K];
  const uint32_t j = blockIdx.y, K = a.K;
  const bool listed = j < a.len;
  if (listed)
    for (uint32_t k = threadIdx.x; k < K; k += kInfoBlock) {
      const double2 l = reinterpret_cast<const double2 *>(a.lam)[(size_t)a.locs[j] * K + k];
      double s = 0.0;  // (as ts_export_loc adds them)
      s += l.x;
      s += l.y;
      s_eb[k] = l.x / s;
    }
  __syncthreads();
  const uint32_t p = blockIdx.x * kInfoBlock + threadIdx.x;
  if (p >= a.ppad) return;
  double v = 0.0;
  if (listed && p < a.P) {
    const InfoAB ab = info_unindex(p, K);
    v = s_eb[ab.a] * s_eb[ab.b];
  }
  a.bb[(size_t)j * a.ppad + p] = v;
}

typedef double info_f64x4 __attribute__((ext_vector_type(4)));

// grid (tiles of this launch, segments).  cobs / cexp are [steps * 4][bpad], bb is [steps * 4][ppad]; seg_steps k-steps per
// segment, `steps` in the chunk; tile t of the block is the individuals' tile t / ptiles and the column tile t % ptiles.
__global__ __launch_bounds__(256) void ts_info_gemm(const double *__restrict__ cobs, const double *__restrict__ cexp, const double *__restrict__ bb,
                                                    uint32_t bpad, uint32_t ppad, uint32_t ptiles, uint32_t tile0, uint32_t steps, uint32_t seg_steps,
                                                    double *__restrict__ part) {
  constexpr uint32_t T = kInfoTile, ROWS = kInfoStageSteps * kInfoStep;  // 16 locations per stage
  constexpr uint32_t LD = T + 16u;                                      // row stride in doubles: the 4 rows of a k-step fall on distinct banks
  constexpr uint32_t PER = 3u * ROWS * T / 2u / kInfoBlock;             // double2 loads per thread and stage: 6
  static_assert(T == 64u && kInfoBlock == 256u && 2u * kInfoBlock == ROWS * T / 2u, "2 x 2 waves of 32 x 32; an array of a stage is two loads per thread");
  __shared__ double sh[3][ROWS][LD];  // c_obs and c_exp of the individuals' tile, BB of the column tile: 30 KB

  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t t = tile0 + blockIdx.x, ti = t / ptiles, tp = t - ti * ptiles;
  const uint32_t seg = blockIdx.y;
  const uint32_t st_begin = seg * seg_steps, st_end = min(steps, st_begin + seg_steps);
  const uint32_t wr = (wave >> 1) * 32u, wc = (wave & 1u) * 32u;
  const uint32_t lk = lane >> 4, li = lane & 15u;

  info_f64x4 acc[2][2][2];  // [product][block row][block column]
#pragma unroll
  for (int p = 0; p < 2; ++p)
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) acc[p][i][j] = info_f64x4{0.0, 0.0, 0.0, 0.0};

  // load u of a thread: array u / 2, then row and double2 column by thread; rows past the segment's end are not loaded (zeros)
  double2 pre[PER];
  auto fetch = [&](uint32_t st0) {
    const uint32_t nrows = min(kInfoStageSteps, st_end - st0) * kInfoStep;
#pragma unroll
    for (uint32_t u = 0; u < PER; ++u) {
      const uint32_t arr = u >> 1, rem = (u & 1u) * kInfoBlock + tid, row = rem / (T / 2u), c2 = rem % (T / 2u);  // (two loads per array)
      const double *src = arr == 0u ? cobs : arr == 1u ? cexp : bb;
      const uint32_t ld = arr == 2u ? ppad : bpad, tile = arr == 2u ? tp : ti;
      pre[u] = row < nrows ? *reinterpret_cast<const double2 *>(src + (size_t)(st0 * kInfoStep + row) * ld + tile * T + 2u * c2) : double2{0.0, 0.0};
    }
  };
  auto stage = [&]() {
#pragma unroll
    for (uint32_t u = 0; u < PER; ++u) {
      const uint32_t arr = u >> 1, rem = (u & 1u) * kInfoBlock + tid, row = rem / (T / 2u), c2 = rem % (T / 2u);
      *reinterpret_cast<double2 *>(&sh[arr][row][2u * c2]) = pre[u];
    }
  };

  if (st_begin < st_end) fetch(st_begin);
  for (uint32_t st0 = st_begin; st0 < st_end; st0 += kInfoStageSteps) {
    __syncthreads();  // (the previous stage has been read)
    stage();
    __syncthreads();
    if (st0 + kInfoStageSteps < st_end) fetch(st0 + kInfoStageSteps);
#pragma unroll
    for (uint32_t kk = 0; kk < kInfoStageSteps; ++kk) {  // (k-steps past the segment's end multiply zeros)
      const uint32_t row = kk * kInfoStep + lk;
      double bv[2];
#pragma unroll
      for (int j = 0; j < 2; ++j) bv[j] = sh[2][row][wc + 16u * j + li];
#pragma unroll
      for (int p = 0; p < 2; ++p) {
        double av[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) av[i] = sh[p][row][wr + 16u * i + li];
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

// grid (tiles of this launch): a tile's segments, in ascending order, onto the block's accumulators [tile][2][T * T]
__global__ __launch_bounds__(256) void ts_info_finish(const double *__restrict__ part, uint32_t nseg, uint32_t tile0, double *__restrict__ acc) {
  constexpr uint32_t T = kInfoTile;
  double *dst = acc + (size_t)(tile0 + blockIdx.x) * (2u * T * T);
  for (uint32_t e = threadIdx.x; e < 2u * T * T; e += kInfoBlock) {
    double v = dst[e];
    for (uint32_t g = 0; g < nseg; ++g) v += part[((size_t)g * gridDim.x + blockIdx.x) * (2u * T * T) + e];
    dst[e] = v;
  }
}

// grid (P / 256 rounded up, the block's blen rows): the rows unpadded, obs and exp [blen][P]
__global__ __launch_bounds__(256) void ts_info_rows(const double *__restrict__ acc, uint32_t P, uint32_t ptiles, double *__restrict__ obs,
                                                    double *__restrict__ exp) {
  constexpr uint32_t T = kInfoTile;
  const uint32_t r = blockIdx.y, p = blockIdx.x * kInfoBlock + threadIdx.x;
  if (p >= P) return;
  const double *t = acc + (size_t)((r / T) * ptiles + p / T) * (2u * T * T) + (r % T) * T + p % T;
  obs[(size_t)r * P + p] = t[0];
  exp[(size_t)r * P + p] = t[T * T];
}

}  // namespace tsamd
