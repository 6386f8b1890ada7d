// State in and out of the device: re-tiling between the reference's (ndims, nparticles) float64 host layout and the
// particle-major device layout, the pipelined host copies, evaluation dispatch, mjhmc_read / mjhmc_write, and the one-off
// operators mjhmc_eval / mjhmc_leapfrog on a throw-away workspace.
#include <hip/hip_runtime.h>

#include <vector>

#include "sampler_internal.hpp"

// float32-valued float64 rows (Shape::round32)
__global__ void round32_kernel(double* __restrict__ a, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) a[i] = (double)(float)a[i];
}
int round_rows32(mjhmc_sampler* s, void* rows) {
  const int64_t n = s->Npad * (int64_t)s->sh.pitch;
  hipLaunchKernelGGL(round32_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s->stream, (double*)rows, n);
  HIPCHK(hipGetLastError());
  return 0;
}

// src (D, N) float64 row-major  ->  dst [N][pitch] T ; only d < D is written
template <typename T>
__global__ void to_particle_major(const double* __restrict__ src, T* __restrict__ dst, int D, int64_t N, int pitch) {
  __shared__ double tile[32][33];
  const int64_t p0 = (int64_t)blockIdx.x * 32;
  const int d0 = blockIdx.y * 32;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int dd = threadIdx.y + 8 * i;
    const int d = d0 + dd;
    const int64_t p = p0 + threadIdx.x;
    if (d < D && p < N) tile[dd][threadIdx.x] = src[(size_t)d * N + p];
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int pp = threadIdx.y + 8 * i;
    const int64_t p = p0 + pp;
    const int d = d0 + threadIdx.x;
    if (d < D && p < N) dst[(size_t)p * pitch + d] = (T)tile[threadIdx.x][pp];
  }
}

// dst[d*rs + k*cs + off] = src[row(k)][d],  row(k) = idx ? idx[k] : k
template <typename T>
__global__ void to_dim_major(const T* __restrict__ src, const int64_t* __restrict__ idx, double* __restrict__ dst,
                             int D, int64_t ncols, int pitch, int64_t rs, int64_t cs, int64_t off) {
  __shared__ double tile[32][33];
  const int64_t k0 = (int64_t)blockIdx.x * 32;
  const int d0 = blockIdx.y * 32;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int kk = threadIdx.y + 8 * i;
    const int64_t k = k0 + kk;
    const int d = d0 + threadIdx.x;
    if (d < D && k < ncols) {
      const int64_t row = idx ? idx[k] : k;
      tile[kk][threadIdx.x] = (double)src[(size_t)row * pitch + d];
    }
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int dd = threadIdx.y + 8 * i;
    const int d = d0 + dd;
    const int64_t k = k0 + threadIdx.x;
    if (d < D && k < ncols) dst[(size_t)d * rs + (size_t)k * cs + off] = tile[threadIdx.x][dd];
  }
}

template <typename T>
__global__ void widen_vec(const T* __restrict__ src, double* __restrict__ dst, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dst[i] = (double)src[i];
}

// cache_active[i] = !isnan(H_flf[i])
template <typename T>
__global__ void flags_from_hflf(const T* __restrict__ h, uint8_t* __restrict__ out, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = (h[i] == h[i]) ? 1 : 0;
}

template <typename T>
__global__ void narrow_vec(const double* __restrict__ src, T* __restrict__ dst, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dst[i] = (T)src[i];
}

// ---------------------------------------------------------------------------------------------
// upload, download, the pipelined host copies
// ---------------------------------------------------------------------------------------------
int ensure_stage(mjhmc_sampler* s, size_t elems) {
  if (s->stage_elems >= elems) return 0;
  if (s->stage) HIPCHK(hipFree(s->stage));
  s->stage = nullptr;
  s->stage_elems = 0;
  HIPCHK(hipMalloc(&s->stage, elems * sizeof(double)));
  s->stage_elems = elems;
  return 0;
}

int upload_matrix(mjhmc_sampler* s, const double* host, void* dst) {
  TRY(ensure_stage(s, (size_t)s->D * s->N));
  HIPCHK(hipMemcpyAsync(s->stage, host, (size_t)s->D * s->N * sizeof(double), hipMemcpyHostToDevice, s->stream));
  dim3 grid((unsigned)((s->N + 31) / 32), (unsigned)((s->D + 31) / 32)), block(32, 8);
  dispatch_dtype(s->dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL(to_particle_major<T>, grid, block, 0, s->stream, s->stage, (T*)dst, s->D, s->N, s->sh.pitch);
  });
  HIPCHK(hipGetLastError());
  return 0;
}

int ensure_pipe_pair(void* pin[2], hipEvent_t ev[2]) {
  for (int i = 0; i < 2; ++i) {
    if (!pin[i]) HIPCHK(hipHostMalloc(&pin[i], kPipeChunk, hipHostMallocDefault));
    if (!ev[i]) HIPCHK(hipEventCreateWithFlags(&ev[i], hipEventDisableTiming));
  }
  return 0;
}

// small blocks take the direct copy, the others the sampler's pinned pair (pipe_chunks)
int copy_to_host(mjhmc_sampler* s, const void* dev_src, void* host_dst, size_t bytes) {
  if (bytes < 2 * kPipeChunk) {
    HIPCHK(hipMemcpyAsync(host_dst, dev_src, bytes, hipMemcpyDeviceToHost, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));
    return 0;
  }
  TRY(ensure_pipe_pair(s->pipe_pin, s->pipe_ev));
  char* const dst = (char*)host_dst;
  return pipe_chunks(s->stream, s->pipe_pin, s->pipe_ev, dev_src, bytes, [dst](size_t off, const char* pin, size_t lo, size_t hi) {
    std::memcpy(dst + off + lo, pin + lo, hi - lo);
  });
}

int launch_to_dim_major(hipStream_t st, int elem, const void* src, const int64_t* idx, double* dst, int D, int64_t ncols,
                        int pitch, int64_t rs, int64_t cs, int64_t off) {
  dim3 grid((unsigned)((ncols + 31) / 32), (unsigned)((D + 31) / 32)), block(32, 8);
  dispatch_dtype(elem, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL(to_dim_major<T>, grid, block, 0, st, (const T*)src, idx, dst, D, ncols, pitch, rs, cs, off);
  });
  HIPCHK(hipGetLastError());
  return 0;
}

// device particle-major rows -> host float64 with strides (see to_dim_major)
int download_cols(mjhmc_sampler* s, const void* src, const int64_t* dev_idx, int64_t ncols, double* host,
                  size_t host_elems, int64_t rs, int64_t cs, int64_t off, bool copy_out, int elem) {
  TRY(launch_to_dim_major(s->stream, elem < 0 ? s->dtype : elem, src, dev_idx, s->stage, s->D, ncols, s->sh.pitch, rs, cs, off));
  if (copy_out) TRY(copy_to_host(s, s->stage, host, host_elems * sizeof(double)));
  return 0;
}

// ---------------------------------------------------------------------------------------------
// evaluation: E, dE/dX and the kinetic energy through the kernels of the sampler's energy family
// ---------------------------------------------------------------------------------------------
template <typename T>
static int run_eval_t(mjhmc_sampler* s, const void* X, void* Gout, void* Eout, const void* V, void* Vgen, void* EVout) {
  const EvalArgs<T> a{(const T*)X, (T*)Gout, (T*)Eout, (T*)EVout, (const T*)V, (T*)Vgen, s->N, s->first_pid,
                      s->D, s->sh.pitch, s->sh.CH, s->sh.logG, rng_key(s, 0)};
  if constexpr (sizeof(T) == 8) {
    if (s->en->is_user()) return user_launch_eval(s->en, a, s->stream);
  }
  TRY(with_elementwise_energy(s->en->ep.kind, [&](auto en) { en.eval(a, s->en->ep, s->sh.E, s->stream); }));
  HIPCHK(hipGetLastError());
  return 0;
}

template <typename S, bool POT>
static int run_eval_dense(mjhmc_sampler* s, const void* X, void* Gout, void* Eout, const void* V, void* Vgen, void* EVout) {
  DenseEvalArgs<S, POT> a{};
  a.X = (const S*)X;
  a.G = (float*)Gout;  // (SparseImageCode: float32 [Npad][1024])
  a.E = (float*)Eout;
  a.EV = (float*)EVout;
  a.V = (const S*)V;
  a.V_gen = (S*)Vgen;
  a.N = s->N;
  a.ntiles = dense_ntiles(s, s->N, s->Npad);
  a.first_pid = s->first_pid;
  a.key = rng_key(s, 0);
  if constexpr (POT) {
    a.D = s->D;
    pot_launch_eval(a, s->en->pot_model(), s->stream, s->en->pot_gen());
  } else {
    sic_launch_eval(a, s->en->sic_model(), s->stream);
  }
  HIPCHK(hipGetLastError());
  return 0;
}

int run_eval(mjhmc_sampler* s, const void* X, void* Gout, void* Eout, const void* V, void* Vgen, void* EVout) {
  // host energies (E and dE/dX are the caller's, mjhmc_host_set_energy) and wide rows (multi-pass device kernels)
  if (s->en->is_host() || s->sh.wide) return wide_run_eval(s, X, Gout, Eout, V, Vgen, EVout);
  if (s->en->is_pot()) return run_eval_dense<float, true>(s, X, Gout, Eout, V, Vgen, EVout);
  // (the state's type of SparseImageCode: bfloat16, BASELINE.json configs[4], or float32, the reference's TensorFlow float32)
  if (s->en->is_sic()) return s->dtype == MJHMC_BF16 ? run_eval_dense<__bf16, false>(s, X, Gout, Eout, V, Vgen, EVout)
                                                    : run_eval_dense<float, false>(s, X, Gout, Eout, V, Vgen, EVout);
  return s->dtype == MJHMC_F64 ? run_eval_t<double>(s, X, Gout, Eout, V, Vgen, EVout)
                               : run_eval_t<float>(s, X, Gout, Eout, V, Vgen, EVout);
}

// E ([Npad] scalars) and dE/dX (a matrix) of the state matrix X, in the layout and element type the sampler's energy
// family writes: what the energy observables evaluate every recorded slot with (functionals.hip)
int sampler_eval_rows(mjhmc_sampler* s, const void* X, void* Gout, void* Eout) {
  return run_eval(s, X, Gout, Eout, nullptr, nullptr, nullptr);
}

// ---------------------------------------------------------------------------------------------
// the stand-alone leapfrog operator
// ---------------------------------------------------------------------------------------------
// rows buf[0] (X), buf[1] (V) -> buf[2], buf[3], dE/dX buf[4], EX buf[5], EV buf[6]
template <typename T>
static int leap_t(mjhmc_sampler& w, void* const* buf, double eps, int L) {
  const LeapArgs<T> a{(const T*)buf[0], (const T*)buf[1], (T*)buf[2], (T*)buf[3], (T*)buf[4], (T*)buf[5], (T*)buf[6], w.N,
                      w.D, w.sh.pitch, w.sh.CH, w.sh.logG, L, (T)eps, (T)(-eps / 2.)};
  if constexpr (sizeof(T) == 8) {
    if (w.en->is_user()) return user_launch_leap(w.en, a, w.stream);
  }
  TRY(with_elementwise_energy(w.en->ep.kind, [&](auto en) { en.leap(a, w.en->ep, w.sh.E, w.stream); }));
  HIPCHK(hipGetLastError());
  return 0;
}

// the dense energies' leapfrog operator on the same rows
template <typename S, bool POT>
static int leap_dense(mjhmc_sampler& w, void* const* buf, double eps, int L) {
  DenseLeapArgs<S, POT> a{};
  a.X = (const S*)buf[0];
  a.V = (const S*)buf[1];
  a.X_out = (S*)buf[2];
  a.V_out = (S*)buf[3];
  a.G = (float*)buf[4];
  a.EX = (float*)buf[5];
  a.EV = (float*)buf[6];
  a.N = w.N;
  a.ntiles = dense_ntiles(&w, w.N, w.Npad);
  a.L = L;
  a.eps = (float)eps;
  a.chalf = (float)(-eps / 2.);
  if constexpr (POT) {
    a.D = w.D;
    pot_launch_leap(a, w.en->pot_model(), w.stream, w.en->pot_gen());
  } else {
    sic_launch_leap(a, w.en->sic_model(), w.stream);
  }
  HIPCHK(hipGetLastError());
  return 0;
}

// the dtype code of the per-particle scalars (ssize): float64 for float64 state, float32 otherwise (bf16 state included)
static int scalar_dtype(const mjhmc_sampler* s) { return s->dtype == MJHMC_F64 ? MJHMC_F64 : MJHMC_F32; }

int read_vec(mjhmc_sampler* s, const void* dev, void* host, size_t nbytes) {
  // state scalars are stored in the state dtype; the ABI hands out float64
  if (nbytes != (size_t)s->N * sizeof(double)) return fail(MJHMC_ERR_INVALID, "expected N float64");
  if (s->dtype == MJHMC_F64) return copy_to_host(s, dev, host, nbytes);
  TRY(ensure_stage(s, (size_t)s->N));
  hipLaunchKernelGGL(widen_vec<float>, dim3((unsigned)((s->N + 255) / 256)), dim3(256), 0, s->stream,
                     (const float*)dev, s->stage, s->N);
  HIPCHK(hipGetLastError());
  return copy_to_host(s, s->stage, host, nbytes);
}

// A throw-away sampler-shaped workspace keeps one code path for re-tiling and evaluation: mjhmc_eval and mjhmc_leapfrog
// run on it.  It owns its stream, the device rows handed out by rows(), the staging matrix and -- if a result was big
// enough to take that path -- the pinned buffers of copy_to_host.
struct OneOffWorkspace {
  mjhmc_sampler w;
  std::vector<void*> owned;
  int open(mjhmc_energy* e, int dtype, int64_t n) {
    w.ctx = e->ctx;
    w.en = e;
    w.N = n;
    w.Npad = (n + 63) / 64 * 64;
    w.first_pid = 0;
    w.D = e->ep.ndims;
    w.dtype = dtype;
    TRY(shape_for(e, &w.dtype, &w.sh));
    HIPCHK(hipStreamCreateWithFlags(&w.stream, hipStreamNonBlocking));
    return 0;
  }
  int rows(void** p, size_t bytes, bool zeroed) {
    HIPCHK(hipMalloc(p, bytes));
    owned.push_back(*p);
    if (zeroed) HIPCHK(hipMemsetAsync(*p, 0, bytes, w.stream));
    return 0;
  }
  // SPARSE_CODE hands dE/dX out in float32 [Npad][D]; the others in the state's rows
  size_t dEdX_bytes() const { return w.en->is_sic() ? (size_t)w.Npad * w.D * sizeof(float) : mat_bytes(&w); }
  int dEdX_elem() const { return w.en->is_sic() ? (int)MJHMC_F32 : w.dtype; }
  ~OneOffWorkspace() {
    for (void* p : owned) (void)hipFree(p);
    if (w.stage) (void)hipFree(w.stage);
    for (int i = 0; i < 2; ++i) {
      if (w.pipe_pin[i]) (void)hipHostFree(w.pipe_pin[i]);
      if (w.pipe_ev[i]) (void)hipEventDestroy(w.pipe_ev[i]);
    }
    if (w.stream) (void)hipStreamDestroy(w.stream);
  }
};

extern "C" {

int mjhmc_read(mjhmc_sampler* s, int field, void* host_dst, size_t nbytes) {
  if (!s || !host_dst) return fail(MJHMC_ERR_INVALID, "NULL argument");
  HIPCHK(hipSetDevice(s->ctx->device));
  const size_t mat = (size_t)s->D * s->N;
  switch (field) {
    case MJHMC_F_X:
    case MJHMC_F_V:
    case MJHMC_F_DEDX: {
      if (nbytes != mat * sizeof(double)) return fail(MJHMC_ERR_INVALID, "expected (D,N) float64");
      TRY(ensure_stage(s, mat));
      const void* src = field == MJHMC_F_X ? s->Xcur : s->Vbuf[s->vcur];
      int elem = s->dtype;
      if (field == MJHMC_F_DEDX && (s->en->is_pot() || s->en->is_host() || s->sh.wide)) {
        src = s->Gbuf[s->vcur];
      } else if (field == MJHMC_F_DEDX) {   // evaluated now; SparseImageCode writes it as a float32 matrix whatever the state's type
        const bool sic = s->en->is_sic();
        if (!s->scratch) HIPCHK(hipMalloc(&s->scratch, sic ? (size_t)s->Npad * s->D * sizeof(float) : mat_bytes(s)));
        TRY(run_eval(s, s->Xcur, s->scratch, nullptr, nullptr, nullptr, nullptr));
        src = s->scratch;
        if (sic) elem = MJHMC_F32;
      }
      return download_cols(s, src, nullptr, s->N, (double*)host_dst, mat, s->N, 1, 0, true, elem);
    }
    case MJHMC_F_EX: return read_vec(s, s->EX[s->scur], host_dst, nbytes);
    case MJHMC_F_EV: return read_vec(s, s->EV[s->scur], host_dst, nbytes);
    case MJHMC_F_HFLF: return read_vec(s, s->Hflf[s->scur], host_dst, nbytes);
    case MJHMC_F_DWELL:
      if (nbytes != (size_t)s->N * sizeof(double)) return fail(MJHMC_ERR_INVALID, "expected N float64");
      return copy_to_host(s, s->dwell, host_dst, nbytes);
    case MJHMC_F_CACHE: {
      if (nbytes != (size_t)s->N) return fail(MJHMC_ERR_INVALID, "expected N uint8");
      TRY(ensure_stage(s, (size_t)(s->N + 7) / 8));
      uint8_t* flags = (uint8_t*)s->stage;
      dispatch_dtype(scalar_dtype(s), [&](auto tag) {
        using T = typename decltype(tag)::type;
        hipLaunchKernelGGL(flags_from_hflf<T>, dim3((unsigned)((s->N + 255) / 256)), dim3(256), 0, s->stream,
                           (const T*)s->Hflf[s->scur], flags, s->N);
      });
      HIPCHK(hipGetLastError());
      return copy_to_host(s, flags, host_dst, nbytes);
    }
    case MJHMC_F_TRANS:
      if (nbytes != (size_t)s->N) return fail(MJHMC_ERR_INVALID, "expected N uint8");
      return copy_to_host(s, s->trans, host_dst, nbytes);
    default: return fail(MJHMC_ERR_INVALID, "unknown field");
  }
}

int mjhmc_write(mjhmc_sampler* s, int field, const void* host_src, size_t nbytes) {
  if (!s || !host_src) return fail(MJHMC_ERR_INVALID, "NULL argument");
  HIPCHK(hipSetDevice(s->ctx->device));
  const size_t mat = (size_t)s->D * s->N;
  switch (field) {
    case MJHMC_F_X:
    case MJHMC_F_V: {
      if (nbytes != mat * sizeof(double)) return fail(MJHMC_ERR_INVALID, "expected (D,N) float64");
      void* dst = field == MJHMC_F_X ? s->Xcur : s->Vbuf[s->vcur];
      s->undo_valid = false;
      s->list_valid = false;
      if (field == MJHMC_F_X) s->host_energy_set = false;  // MJHMC_E_HOST: E and dE/dX of the new X are the caller's to supply
      TRY(upload_matrix(s, (const double*)host_src, dst));
      if (s->sh.round32) TRY(round_rows32(s, dst));
      TRY(run_eval(s, s->Xcur, s->Gbuf[s->vcur], s->EX[s->scur], s->Vbuf[s->vcur], nullptr, s->EV[s->scur]));
      HIPCHK(hipMemsetAsync(s->Hflf[s->scur], 0xFF, s->Npad * ssize(s), s->stream));
      TRY(drop_spec(s));
      HIPCHK(hipStreamSynchronize(s->stream));
      return 0;
    }
    case MJHMC_F_HFLF: {  // float64 (N); NaN marks a cold cache entry
      if (nbytes != (size_t)s->N * sizeof(double)) return fail(MJHMC_ERR_INVALID, "expected N float64");
      TRY(drop_spec(s));
      s->list_valid = false;
      if (s->dtype == MJHMC_F64) {
        HIPCHK(hipMemcpyAsync(s->Hflf[s->scur], host_src, nbytes, hipMemcpyHostToDevice, s->stream));
      } else {
        TRY(ensure_stage(s, (size_t)s->N));
        HIPCHK(hipMemcpyAsync(s->stage, host_src, nbytes, hipMemcpyHostToDevice, s->stream));
        hipLaunchKernelGGL(narrow_vec<float>, dim3((unsigned)((s->N + 255) / 256)), dim3(256), 0, s->stream,
                           (const double*)s->stage, (float*)s->Hflf[s->scur], s->N);
        HIPCHK(hipGetLastError());
      }
      HIPCHK(hipStreamSynchronize(s->stream));
      return 0;
    }
    default: return fail(MJHMC_ERR_INVALID, "field is not writable");
  }
}

int mjhmc_eval(mjhmc_energy* e, int dtype, const double* X, int64_t n, double* E_out, double* dEdX_out) {
  if (!e || !X || n < 1) return fail(MJHMC_ERR_INVALID, "bad argument");
  TRY(check_state_dtype(e, dtype));
  if (e->is_host()) return fail(MJHMC_ERR_UNSUPPORTED, "a host-evaluated energy has no device evaluation: call the callables");
  HIPCHK(hipSetDevice(e->ctx->device));
  OneOffWorkspace ws;
  mjhmc_sampler& w = ws.w;
  TRY(ws.open(e, dtype, n));
  void *Xd = nullptr, *Gd = nullptr, *Ed = nullptr;
  TRY(ws.rows(&Xd, mat_bytes(&w), true));
  if (dEdX_out) TRY(ws.rows(&Gd, ws.dEdX_bytes(), false));
  if (E_out) TRY(ws.rows(&Ed, w.Npad * ssize(&w), false));
  TRY(upload_matrix(&w, X, Xd));
  if (w.sh.round32) TRY(round_rows32(&w, Xd));
  TRY(run_eval(&w, Xd, Gd, Ed, nullptr, nullptr, nullptr));
  if (E_out) TRY(read_vec(&w, Ed, E_out, (size_t)n * sizeof(double)));
  if (dEdX_out) TRY(download_cols(&w, Gd, nullptr, n, dEdX_out, (size_t)w.D * n, n, 1, 0, true, ws.dEdX_elem()));
  HIPCHK(hipStreamSynchronize(w.stream));
  return 0;
}

int mjhmc_leapfrog(mjhmc_energy* e, int dtype, const double* X, const double* V, int64_t n, double eps, int n_steps,
                   double* X_out, double* V_out, double* EX_out, double* EV_out, double* dEdX_out) {
  if (!e || !X || !V || !X_out || !V_out || n < 1 || n_steps < 0) return fail(MJHMC_ERR_INVALID, "bad argument");
  TRY(check_state_dtype(e, dtype));
  if (e->is_host()) return fail(MJHMC_ERR_UNSUPPORTED, "a host-evaluated energy has no device leapfrog operator");
  HIPCHK(hipSetDevice(e->ctx->device));
  OneOffWorkspace ws;
  mjhmc_sampler& w = ws.w;
  TRY(ws.open(e, dtype, n));
  void* buf[7] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};  // X, V, X', V', G, EX, EV
  const size_t mb = mat_bytes(&w), vb = (size_t)w.Npad * ssize(&w);
  for (int i = 0; i < 4; ++i) TRY(ws.rows(&buf[i], mb, true));
  if (dEdX_out) TRY(ws.rows(&buf[4], ws.dEdX_bytes(), true));
  if (EX_out) TRY(ws.rows(&buf[5], vb, false));
  if (EV_out) TRY(ws.rows(&buf[6], vb, false));
  TRY(upload_matrix(&w, X, buf[0]));
  TRY(upload_matrix(&w, V, buf[1]));
  if (w.sh.round32) {
    TRY(round_rows32(&w, buf[0]));
    TRY(round_rows32(&w, buf[1]));
  }
  if (e->is_pot() && !w.sh.wide) {
    TRY((leap_dense<float, true>(w, buf, eps, n_steps)));
  } else if (e->is_sic()) {
    if (w.dtype == MJHMC_BF16) TRY((leap_dense<__bf16, false>(w, buf, eps, n_steps)));
    else TRY((leap_dense<float, false>(w, buf, eps, n_steps)));
  } else if (w.sh.wide) {
    TRY(wide_leapfrog(&w, (const double*)buf[0], (const double*)buf[1], (double*)buf[2], (double*)buf[3], (double*)buf[4],
                      (double*)buf[5], (double*)buf[6], eps, n_steps));
  } else if (w.dtype == MJHMC_F64) {
    TRY(leap_t<double>(w, buf, eps, n_steps));
  } else {
    TRY(leap_t<float>(w, buf, eps, n_steps));
  }
  const size_t total = (size_t)w.D * n;
  TRY(download_cols(&w, buf[2], nullptr, n, X_out, total, n, 1, 0, true));
  TRY(download_cols(&w, buf[3], nullptr, n, V_out, total, n, 1, 0, true));
  if (dEdX_out) TRY(download_cols(&w, buf[4], nullptr, n, dEdX_out, total, n, 1, 0, true, ws.dEdX_elem()));
  if (EX_out) TRY(read_vec(&w, buf[5], EX_out, (size_t)n * sizeof(double)));
  if (EV_out) TRY(read_vec(&w, buf[6], EV_out, (size_t)n * sizeof(double)));
  HIPCHK(hipStreamSynchronize(w.stream));
  return 0;
}

}  // extern "C"
