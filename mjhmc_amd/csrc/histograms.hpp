// Weighted marginal histograms of blocks of ring slots (histograms.hip): per dimension B bins between lo_d and hi_d plus
// an underflow and an overflow bin, a uint64 count and a uint64 mass (weights in units of a power-of-two quantum) per
// bin.  Every sum is an integer: the tables do not depend on the order of addition.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "autocor.hpp"   // RingView

constexpr int kHistogramMaxBins = 1024;

// launch geometry for one ring shape and bin count; a function of (N, D, pitch, dtype, B) alone
struct HistogramPlan {
  int vec = 2;            // elements in the 16 bytes of a row a lane owns
  int bins = 1;           // B
  int strip = 1;          // dimensions a workgroup bins (a power of two): its [strip][B + 2] tables are in LDS
  int cw = 1, log_cw = 0; // column lanes of a workgroup = max(1, strip / vec); 256 / cw row lanes
  int gx = 1, gy = 1;     // workgroups over the particles x strips
  int check_gx = 1, check_gy = 1;   // the weight check's grid: one partial sum of units per workgroup
  size_t lds_bytes = 0;   // strip * (B + 2) * (8 + 4)
};

HistogramPlan histogram_plan(const RingView& r, int bins);

// flag bits the weight check raises in *bad
constexpr int kHistBadNonfinite = 1;   // a weight that is not finite, or negative
constexpr int kHistBadTooLarge = 2;    // a weight with w / q >= 2^53
constexpr int kHistBadTotal = 4;       // the block would take W_units to 2^63 or beyond

// One block: n slots of `r` (r.base = the first slot), weights w[k * Npad + p] (device; nullptr = 1).  Three launches on
// `st`: the check over the n * N weights (flags in *bad, the block's units per workgroup in `partial`), the decision (adds
// the block's units to *W_units unless a flag is up or the sum would reach 2^63) and the histogram pass, which adds to
// count / mass [D][B + 2] and does nothing when *bad is set.
int histogram_accumulate(hipStream_t st, const RingView& r, int n, const double* w, const double* lo, const double* inv,
                         double inv_q, const HistogramPlan& plan, unsigned long long* partial, unsigned long long* count,
                         unsigned long long* mass, unsigned long long* W_units, int* bad, std::string& err);

// The weight logic of a block on its own, for the passes that share it (pairhist.hip).  histogram_check_grid: the check's
// grid for N particles; `partial` holds check_gx * check_gy values.  histogram_weight_pass: the check (w != nullptr) and the
// decision of histogram_accumulate, two launches on `st`.  histogram_refusal: the error a raised flag becomes -- code
// and message recorded through mjhmc_fail -- for the dwell slots [w_slot0, w_slot0 + n) of the refused block.
void histogram_check_grid(int64_t N, int* check_gx, int* check_gy);
void histogram_weight_pass(hipStream_t st, const double* w, int64_t Npad, int64_t N, int n, double inv_q, int check_gx,
                           int check_gy, unsigned long long* partial, unsigned long long* W_units, int* bad);
int histogram_refusal(int bad, int w_slot0, int n);
