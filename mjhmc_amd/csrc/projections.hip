// The device pass of the linear projections (projections.hpp): the identity-link instantiations of projections_kernel --
// three state types x the two tiles -- and their launch, and the hipRTC build of the kernel around a caller's link
// expression.  The handle, its device copies of A, b and the parameters, and the derived ring are functionals.hip's
// (mjhmc_functionals_create_linear).
#include "projections.hpp"

#include <string>
#include <vector>

#include "../../include/mjhmc_hip.h"
#include "handles.hpp"
#include "user_expr.hpp"

namespace mjhmc {

namespace {

template <int DT>
void launch(const ProjArgs& a, dim3 grid, hipStream_t stream) {
  const ProjIdentity id{nullptr};
  if (proj_lane_values(a.K) == 1)
    hipLaunchKernelGGL((projections_kernel<DT, 1, ProjIdentity>), grid, dim3(256), 0, stream, a, id);
  else
    hipLaunchKernelGGL((projections_kernel<DT, 4, ProjIdentity>), grid, dim3(256), 0, stream, a, id);
}

// the translation unit handed to hipRTC
std::string link_source(const std::string& link) {
  std::string s;
  s += "#include \"projections.hpp\"\n";
  s += "namespace mjhmc {\n";
  s += "// g = link(u, k; p): the caller's expression\n";
  s += "struct UserLink {\n";
  s += "  const double* p;  // parameters, device memory\n";
  s += "  __device__ __forceinline__ double apply(double u, int k) const { (void)u; (void)k; return (double)(" + link + "); }\n";
  s += "};\n";
  s += "}  // namespace mjhmc\n";
  return s;
}

}  // namespace

bool projections_launch(const ProjArgs& a, int state_dtype, hipStream_t stream) {
  const dim3 grid((unsigned)((a.N + kProjRows - 1) / kProjRows), (unsigned)(a.n < 1024 ? a.n : 1024));
  if (state_dtype == 0) launch<0>(a, grid, stream);
  else if (state_dtype == 1) launch<1>(a, grid, stream);
  else if (state_dtype == 2) launch<2>(a, grid, stream);
  else return false;
  return true;
}

int projections_link_compile(const std::string& link, int state_dtype, int K, const std::string& include_dir, const RtcCode** out,
                             std::string* err) {
  bool blank = true;
  for (char ch : link) blank = blank && (ch == ' ' || ch == '\t' || ch == '\n');
  if (blank || link.find(';') != std::string::npos) {
    *err = "the link must be one C expression of u, k and p[m] (it is empty or holds a semicolon)";
    return MJHMC_ERR_INVALID;
  }
  const std::string name = "mjhmc::projections_kernel<" + std::to_string(state_dtype) + ", " + std::to_string(proj_lane_values(K)) +
                           ", mjhmc::UserLink>";
  return rtc_compile_cached(link_source(link), "mjhmc_projections.hip", {name}, include_dir, "the link expression does not compile", out, err);
}

}  // namespace mjhmc

extern "C" {

int mjhmc_projections_check(int n_values, const char* link_expr, const char* include_dir) {
  if (n_values < 1 || n_values > mjhmc::kProjMaxValues)
    return mjhmc_fail(MJHMC_ERR_INVALID, "the number of values K must be in [1, " + std::to_string(mjhmc::kProjMaxValues) +
                                             "], got " + std::to_string(n_values));
  if (!link_expr) return 0;   // the identity is in the library
  if (!include_dir) return mjhmc_fail(MJHMC_ERR_INVALID, "NULL argument");
  const RtcCode* c = nullptr;
  std::string err;
  const int rc = mjhmc::projections_link_compile(link_expr, MJHMC_F64, n_values, include_dir, &c, &err);
  return rc ? mjhmc_fail(rc, err) : 0;
}

}  // extern "C"
