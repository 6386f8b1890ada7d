// Fair sample paths on a uniform time grid (timegrid.hip): the jump process x_p(t) of every chain -- chain p sits in
// state k for its holding time -- sampled at t_j = j * dt into a grid ring of the sample ring's own slot layout.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "autocor.hpp"   // RingView

// One block: n slots of `r` (r.base = the first slot), weights w[k * Npad + p] (device; nullptr = 1).  Per chain p < N, k
// ascending, from the clock T_in[p] and the cursor j_in[p]:
//   Tn = T + w;  while (j < n_grid && (double)j * dt < Tn) { grid[j][p][:] = x[k][p][:]; ++j; }  T = Tn
// and the results go to T_out / j_out (other buffers than T_in / j_in: the lanes of a row read the clock while the row's
// first lane may already have written it).  Two launches on `st`: the check over the n * N weights (w != nullptr; *bad for
// one that is not finite or is negative) and the pass, which returns at its top when *bad is set.
int timegrid_accumulate(hipStream_t st, const RingView& r, int n, const double* w, double dt, int n_grid, void* grid,
                        const double* T_in, const int* j_in, double* T_out, int* j_out, int* bad, std::string& err);

// ext[0] = max_p (n_grid - j[p]), ext[1] = max_p j[p] over p < N (integer atomics: exact); ext must be zero at launch
int timegrid_extent(hipStream_t st, const int* j, int64_t N, int n_grid, int* ext, std::string& err);
