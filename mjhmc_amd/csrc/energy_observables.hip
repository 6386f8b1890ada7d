// The device pass of the energy observables (energy_observables.hpp): the instantiations of energy_observables_kernel for
// the (state, gradient) type pairs the energy families write, and their launch.  The handle, its scratch and the
// evaluation that fills it are functionals.hip's (mjhmc_functionals_create_energy).
//   float64 state  -> float64 dE/dX and E   (elementwise and user-expression energies, the wide / multi-pass path,
//                                            ProductOfT and linear models with float64 state)
//   float32 state  -> float32 dE/dX and E   (elementwise energies, ProductOfT and linear models, SparseImageCode)
//   bfloat16 state -> float32 dE/dX and E   (SparseImageCode)
#include "energy_observables.hpp"

#ifdef MJHMC_TEST_HOOKS
#include "handles.hpp"
#include "ring_source.hpp"
#endif

namespace mjhmc {

namespace {

template <int DT, int GT>
void launch(const EnergyObsArgs& a, bool wide, hipStream_t stream) {
  const long long rows_per_block = wide ? 4 : (long long)kFnInFlight * (256 >> a.log_cw);
  const unsigned gx = (unsigned)((a.N + rows_per_block - 1) / rows_per_block);
  if (wide)
    hipLaunchKernelGGL((energy_observables_kernel<DT, GT, true>), dim3(gx), dim3(256), 0, stream, a);
  else
    hipLaunchKernelGGL((energy_observables_kernel<DT, GT, false>), dim3(gx), dim3(256), 0, stream, a);
}

}  // namespace

bool energy_observables_launch(const EnergyObsArgs& a, int state_dtype, bool grad_f32, bool wide, hipStream_t stream) {
  if (state_dtype == 0 && !grad_f32) launch<0, 0>(a, wide, stream);
  else if (state_dtype == 1 && grad_f32) launch<1, 1>(a, wide, stream);
  else if (state_dtype == 2 && grad_f32) launch<2, 1>(a, wide, stream);
  else return false;
  return true;
}

}  // namespace mjhmc

#ifdef MJHMC_TEST_HOOKS
extern "C" {
// test build only: one slot of a derived ring as it lies on the device -- [Npad][pitchK] float64, padding rows and padding
// elements included (mjhmc_functionals_read hands out the K values of the rows p < N only)
int mjhmc_test_functionals_read_raw(mjhmc_functionals* f, int slot, void* host_dst, size_t nbytes) {
  if (!f || !host_dst) return mjhmc_fail(MJHMC_ERR_INVALID, "bad argument");
  const RingSource r = functionals_ring_source(f);
  if (!r.base || slot < 0 || slot >= r.slots || nbytes != r.slot_bytes) return mjhmc_fail(MJHMC_ERR_INVALID, "bad argument");
  mjhmc_sampler* s = functionals_sampler(f);
  HIPCHK(hipSetDevice(s->ctx->device));
  HIPCHK(hipMemcpyAsync(host_dst, r.base + (size_t)slot * r.slot_bytes, nbytes, hipMemcpyDeviceToHost, s->stream));
  HIPCHK(hipStreamSynchronize(s->stream));
  return 0;
}
}  // extern "C"
#endif
