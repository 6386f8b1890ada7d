// Weighted joint histograms of pairs of state dimensions over blocks of ring slots (pairhist.hip): per pair (i, j) a
// [B + 2][B + 2] table of uint64 counts and uint64 masses (weights in units of a power-of-two quantum), the i axis
// fastest, row / column 0 and B + 1 the outer bins of an axis.  Every sum is an integer: the tables do not depend on the
// order of addition.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "autocor.hpp"   // RingView

constexpr int kPairhistMaxPairs = 64;
constexpr int kPairhistMaxBins = 128;
// Dynamic LDS a workgroup gets without a function attribute.  A pair's private tables take (B + 2)^2 * (8 + 4) bytes:
// four pairs at B = 32 (13 872 bytes each), one pair up to B = 71 (63 948 bytes); from B = 72 on (65 712 bytes) the
// pass adds straight into the global tables.
constexpr size_t kPairhistLdsBudget = 65536;
constexpr int kPairhistMaxGroup = 8;    // pairs a workgroup bins at most (small B would fit hundreds)

// launch geometry; the form and the grouping are functions of (B, P) alone, the grid over the particles of N too
struct PairhistPlan {
  int bins = 1;           // B
  int cells = 9;          // (B + 2)^2, the cells of one pair's table
  int n_pairs = 1;        // P
  bool lds = true;        // LDS tables (flushed at the end) or atomics straight into the global tables
  int group = 1;          // pairs a workgroup bins: min(P, kPairhistMaxGroup, kPairhistLdsBudget / (12 cells)); global form: 1
  int gx = 1, gy = 1;     // workgroups over the particles x groups of pairs
  int check_gx = 1, check_gy = 1;   // the weight check's grid (histograms.hpp)
  size_t lds_bytes = 0;   // group * cells * (8 + 4); global form: 0
};

PairhistPlan pairhist_plan(int64_t N, int bins, int n_pairs);

// One block: n slots of `r` (r.base = the first slot), weights w[k * Npad + p] (device; nullptr = 1).  The weight check
// and decision of the 1-D pass (histograms.hpp: histogram_weight_pass), then the pair pass, which adds to count / mass
// [P][B + 2][B + 2] and does nothing when *bad is set.  pairs: int32 [P][2]; range: double [P][4] = lo_i, inv_i, lo_j, inv_j.
int pairhist_accumulate(hipStream_t st, const RingView& r, int n, const double* w, const int32_t* pairs, const double* range,
                        double inv_q, const PairhistPlan& plan, unsigned long long* partial, unsigned long long* count,
                        unsigned long long* mass, unsigned long long* W_units, int* bad, std::string& err);
