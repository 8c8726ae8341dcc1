// Test probe: evaluates one device primitive of the engine elementwise, so tests/test_gpu_device_math.py can compare it
// with correctly rounded references (tests/golden/device_math_refs.npz).  Compiled by the tests with the library's own
// flags (terastructure_amd.build.FLAGS), so contraction and fma choices match the kernels; never part of libtsamd.so.
//
//   int tsamd_math_probe(int op, int param, const double *in, int n_in, double *out, int n_out)
//
// one thread per output element group; `param` is K (gamma_to_w*) or NV (WaveFold).  Returns a hipError_t (0: ok),
// or -1 for an unknown op / parameter or a size that does not match the op.
#include <utility>

#include "tsamd_resident_kernels.h"

namespace probe {

using namespace tsamd;

enum Op {
  kDigamma = 0,        // in x            -> out psi(x)
  kExpDigammaSplit = 1, // in x           -> out (z, a)
  kExpNonpos = 2,      // in d            -> out exp(d)
  kFastRcp = 3,        // in x            -> out 1/x
  kFastRsqrt = 4,      // in x            -> out 1/sqrt(x)
  kEbeta = 5,          // in (l0, l1)     -> out (Ebeta_0, Ebeta_1) through epilogue_values_reg (eta = 0, eb_used = 1)
  kGammaToW = 6,       // in g[K]         -> out w[K]
  kGammaToWLean = 7,   // in g[K]         -> out w[K]
  kWaveFold = 8,       // in [wave][NV][64 lanes] -> out per thread (fold result, slot)
  kCodes = 9,          // in code         -> out (mom, dad, ok, code_nibble)
};

__global__ void k_scalar(int op, const double *in, double *out, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const double x = in[i < n ? i : n - 1];
  double r0 = 0.0, r1 = 0.0, r2 = 0.0, r3 = 0.0;
  switch (op) {
    case kDigamma: r0 = digamma(x); break;
    case kExpDigammaSplit: exp_digamma_split(x, r0, r1); break;
    case kExpNonpos: r0 = exp_nonpos(x); break;
    case kFastRcp: r0 = fast_rcp(x); break;
    case kFastRsqrt: r0 = fast_rsqrt(x); break;
    case kCodes: {
      bool ok;
      const uint32_t c = (uint32_t)x & 3u;
      code_weights(c, r0, r1, ok);
      r2 = ok ? 1.0 : 0.0;
      r3 = (double)code_nibble(c);
      break;
    }
    default: break;
  }
  if (i < n) {
    const int w = op == kExpDigammaSplit ? 2 : op == kCodes ? 4 : 1;
    out[w * i] = r0;
    if (w > 1) out[w * i + 1] = r1;
    if (w > 2) {
      out[w * i + 2] = r2;
      out[w * i + 3] = r3;
    }
  }
}

// threads 2e and 2e + 1 (neighbouring lanes, as in the kernels) hold the two sides of pair e; every lane of a wave runs
// the cross-lane move, out-of-range threads on a clamped copy of the last pair
__global__ void k_ebeta(const double *in, double *out, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int src = i < n ? i : (n - 2) + (i & 1);
  DevParams p{};
  p.eta0 = 0.0;
  p.eta1 = 0.0;
  double nw, eb_new, diff;
  epilogue_values_reg(p, (uint32_t)i & 1u, in[src], 1.0, 0.0, nw, eb_new, diff);
  if (i < n) out[i] = eb_new;
}

template <int K, bool LEAN>
__global__ void k_gamma_to_w(const double *in, double *out, int rows) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int r = i < rows ? i : rows - 1;
  double g[K], w[K];
#pragma unroll
  for (int k = 0; k < K; ++k) g[k] = in[(size_t)r * K + k];
  if constexpr (LEAN) gamma_to_w_lean<K>(g, w); else gamma_to_w<K>(g, w);
  if (i < rows) {
#pragma unroll
    for (int k = 0; k < K; ++k) out[(size_t)i * K + k] = w[k];
  }
}

template <int NV>
__global__ void k_wave_fold(const double *in, double *out, int waves) {
  using F = WaveFold<NV>;
  const int wave = blockIdx.x * (blockDim.x / 64) + threadIdx.x / 64;
  const uint32_t lane = threadIdx.x % 64u;
  const int wv = wave < waves ? wave : waves - 1;
  double v[F::P];
#pragma unroll
  for (int j = 0; j < F::P; ++j) v[j] = j < NV ? in[((size_t)wv * NV + j) * 64 + lane] : 0.0;
  const double s = F::fold(v, lane);
  if (wave < waves) {
    out[((size_t)wave * 64 + lane) * 2] = s;
    out[((size_t)wave * 64 + lane) * 2 + 1] = (double)F::slot(lane);
  }
}

constexpr int kThreads = 256;

inline int blocks_for(int threads) { return (threads + kThreads - 1) / kThreads; }

template <int K>
int launch_gamma(bool lean, const double *in, double *out, int rows) {
  if (lean)
    hipLaunchKernelGGL((k_gamma_to_w<K, true>), dim3(blocks_for(rows)), dim3(kThreads), 0, 0, in, out, rows);
  else
    hipLaunchKernelGGL((k_gamma_to_w<K, false>), dim3(blocks_for(rows)), dim3(kThreads), 0, 0, in, out, rows);
  return 0;
}

template <int NV>
int launch_fold_one(const double *in, double *out, int waves) {
  hipLaunchKernelGGL((k_wave_fold<NV>), dim3(blocks_for(waves * 64)), dim3(kThreads), 0, 0, in, out, waves);
  return 0;
}

template <int... NV>
int launch_fold(int nv, const double *in, double *out, int waves, std::integer_sequence<int, NV...>) {
  int found = -1;
  ((nv == NV + 1 ? (found = launch_fold_one<NV + 1>(in, out, waves)) : 0), ...);
  return found;
}

}  // namespace probe

extern "C" int tsamd_math_probe(int op, int param, const double *in, int n_in, double *out, int n_out) {
  using namespace probe;
  // elements (threads) and the sizes the op implies
  int n = 0;
  switch (op) {
    case kDigamma: case kExpNonpos: case kFastRcp: case kFastRsqrt: n = n_in; if (n_out != n) return -1; break;
    case kExpDigammaSplit: n = n_in; if (n_out != 2 * n) return -1; break;
    case kCodes: n = n_in; if (n_out != 4 * n) return -1; break;
    case kEbeta: n = n_in; if (n % 2 != 0 || n_out != n) return -1; break;
    case kGammaToW: case kGammaToWLean:
      if (param != 3 && param != 8 && param != 20 && param != 32) return -1;
      if (n_in % param != 0 || n_out != n_in) return -1;
      n = n_in / param;
      break;
    case kWaveFold:
      if (param < 1 || param > 64 || n_in % (64 * param) != 0) return -1;
      n = n_in / (64 * param);  // waves
      if (n_out != 2 * 64 * n) return -1;
      break;
    default: return -1;
  }
  if (n <= 0) return -1;
  double *d_in = nullptr, *d_out = nullptr;
  hipError_t e = hipMalloc(&d_in, sizeof(double) * (size_t)n_in);
  if (e == hipSuccess) e = hipMalloc(&d_out, sizeof(double) * (size_t)n_out);
  if (e == hipSuccess) e = hipMemcpy(d_in, in, sizeof(double) * (size_t)n_in, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemset(d_out, 0, sizeof(double) * (size_t)n_out);
  int rc = 0;
  if (e == hipSuccess) {
    switch (op) {
      case kEbeta: hipLaunchKernelGGL(k_ebeta, dim3(blocks_for(n)), dim3(kThreads), 0, 0, d_in, d_out, n); break;
      case kGammaToW: case kGammaToWLean: {
        const bool lean = op == kGammaToWLean;
        rc = param == 3 ? launch_gamma<3>(lean, d_in, d_out, n) : param == 8 ? launch_gamma<8>(lean, d_in, d_out, n)
             : param == 20 ? launch_gamma<20>(lean, d_in, d_out, n) : launch_gamma<32>(lean, d_in, d_out, n);
        break;
      }
      case kWaveFold: rc = launch_fold(param, d_in, d_out, n, std::make_integer_sequence<int, 64>{}); break;
      default: hipLaunchKernelGGL(k_scalar, dim3(blocks_for(n)), dim3(kThreads), 0, 0, op, d_in, d_out, n); break;
    }
    e = hipGetLastError();
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess && rc == 0) e = hipMemcpy(out, d_out, sizeof(double) * (size_t)n_out, hipMemcpyDeviceToHost);
  }
  if (d_in) (void)hipFree(d_in);
  if (d_out) (void)hipFree(d_out);
  return e != hipSuccess ? (int)e : rc;
}
