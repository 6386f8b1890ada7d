// Test build only (libmjhmc_hip_test.so; the Makefile lists this file for that library alone): the hand-written device
// math of the samplers -- neg_log_unit, sincospi_unit, box_muller (philox.hpp), box_muller_f32 (dense_pot.hpp), the exp
// chains and jump_rate (jump_math.hpp) -- evaluated on caller arrays, one lane per element, and normal_pair on a grid
// of (particle id, pair).  The kernels call the product's own inline functions: what tests/test_gpu_device_math.py
// compares with its long-double references is the code the samplers run.
#ifdef MJHMC_TEST_HOOKS
#include "handles.hpp"
#include "jump_math.hpp"

namespace {

__global__ void device_math_kernel(int which, const double* a, const double* b, int64_t n, double* out0, double* out1) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double x = a[i], y = b ? b[i] : 0.0;
  double r0 = 0.0, r1 = 0.0;
  switch (which) {
    case 0: r0 = neg_log_unit(x); break;
    case 1: sincospi_unit(x, r0, r1); break;
    case 2: box_muller(x, y, r0, r1); break;
    case 3: {
      float z0, z1;
      box_muller_f32((float)x, (float)y, z0, z1);
      r0 = (double)z0;
      r1 = (double)z1;
      break;
    }
    case 4: r0 = exp_normal<true, false>(x); break;
    case 5: r0 = exp_normal<true, true>(x); break;
    case 6: r0 = exp_normal<false, true>(x); break;
    case 7: r0 = exp_any(x); break;
    case 8: r0 = exp_neg(x); break;
    case 9: r0 = exp_neg_k(x, exp_neg_pinned()); break;
    case 10: r0 = jump_rate<false>(x); break;
    default: r0 = jump_rate<true>(x); break;
  }
  out0[i] = r0;
  if (out1) out1[i] = r1;
}

// out[(p * n_pairs + j) * 2 + {0, 1}] = normal_pair(key, first_pid + p, j)
__global__ void normal_pairs_kernel(RngKey key, uint32_t first_pid, int n_pid, int n_pairs, double* out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)n_pid * n_pairs) return;
  const uint32_t p = (uint32_t)(i / n_pairs), j = (uint32_t)(i % n_pairs);
  double z0, z1;
  normal_pair(key, first_pid + p, j, z0, z1);
  out[2 * i] = z0;
  out[2 * i + 1] = z1;
}

constexpr int kDeviceMathFunctions = 12;
constexpr int64_t kProbeMax = int64_t(1) << 24;   // elements per call: test sizes

}  // namespace

extern "C" {

// which: 0 neg_log_unit(a)  1 sincospi_unit(a) -> (sin, cos)  2 box_muller(a, b)  3 box_muller_f32((float)a, (float)b)
// 4, 5, 6 exp_normal<true, false>, <true, true>, <false, true>(a)  7 exp_any(a)  8 exp_neg(a)  9 exp_neg_k(a, pinned)
// 10, 11 jump_rate<false>, <true>(a).  a, out0: n host doubles; b (which 2, 3) and out1 (second result) may be NULL.
int mjhmc_test_device_math(mjhmc_ctx* ctx, int which, const double* a, const double* b, int64_t n, double* out0,
                           double* out1) {
  if (!ctx || !a || !out0 || n < 0 || n > kProbeMax || which < 0 || which >= kDeviceMathFunctions)
    return mjhmc_fail(MJHMC_ERR_INVALID, "bad argument");
  if ((which == 2 || which == 3) && !b) return mjhmc_fail(MJHMC_ERR_INVALID, "this function takes two arguments");
  if (n == 0) return 0;
  HIPCHK(hipSetDevice(ctx->device));
  const size_t bytes = (size_t)n * sizeof(double);
  double* d = nullptr;
  hipError_t rc = hipMalloc(&d, 4 * bytes);
  if (rc != hipSuccess) return mjhmc_fail(MJHMC_ERR_HIP, hipGetErrorString(rc));
  double *d_a = d, *d_b = b ? d + n : nullptr, *d_0 = d + 2 * n, *d_1 = out1 ? d + 3 * n : nullptr;
  rc = hipMemcpy(d_a, a, bytes, hipMemcpyHostToDevice);
  if (rc == hipSuccess && b) rc = hipMemcpy(d_b, b, bytes, hipMemcpyHostToDevice);
  if (rc == hipSuccess) {
    hipLaunchKernelGGL(device_math_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, which, d_a, d_b, n, d_0, d_1);
    rc = hipGetLastError();
  }
  if (rc == hipSuccess) rc = hipMemcpy(out0, d_0, bytes, hipMemcpyDeviceToHost);
  if (rc == hipSuccess && out1) rc = hipMemcpy(out1, d_1, bytes, hipMemcpyDeviceToHost);
  (void)hipFree(d);
  if (rc != hipSuccess) return mjhmc_fail(MJHMC_ERR_HIP, hipGetErrorString(rc));
  return 0;
}

// out: [n_pid][n_pairs][2] host doubles, normal_pair() of RNG tick `tick` of a sampler seeded `seed` for the particle
// ids first_pid .. first_pid + n_pid - 1 (below 2^32) and the pairs 0 .. n_pairs - 1
int mjhmc_test_normal_pairs(mjhmc_ctx* ctx, uint64_t seed, uint64_t tick, int64_t first_pid, int n_pid, int n_pairs,
                            double* out) {
  if (!ctx || !out || n_pid < 1 || n_pairs < 1 || first_pid < 0 || first_pid + n_pid > (int64_t(1) << 32) ||
      (int64_t)n_pid * n_pairs > kProbeMax)
    return mjhmc_fail(MJHMC_ERR_INVALID, "bad argument");
  HIPCHK(hipSetDevice(ctx->device));
  const int64_t n = (int64_t)n_pid * n_pairs;
  const size_t bytes = (size_t)n * 2 * sizeof(double);
  double* d = nullptr;
  hipError_t rc = hipMalloc(&d, bytes);
  if (rc != hipSuccess) return mjhmc_fail(MJHMC_ERR_HIP, hipGetErrorString(rc));
  const RngKey key{(uint32_t)(seed & 0xFFFFFFFFu), (uint32_t)(seed >> 32), (uint32_t)(tick & 0xFFFFFFFFu),
                   (uint32_t)(tick >> 32)};   // sampler_internal.hpp: rng_key()
  hipLaunchKernelGGL(normal_pairs_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, key, (uint32_t)first_pid,
                     n_pid, n_pairs, d);
  rc = hipGetLastError();
  if (rc == hipSuccess) rc = hipMemcpy(out, d, bytes, hipMemcpyDeviceToHost);
  (void)hipFree(d);
  if (rc != hipSuccess) return mjhmc_fail(MJHMC_ERR_HIP, hipGetErrorString(rc));
  return 0;
}

}  // extern "C"
#endif  // MJHMC_TEST_HOOKS
