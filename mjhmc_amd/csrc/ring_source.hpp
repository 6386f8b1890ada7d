// Where an accumulator handle (mjhmc_estimator, mjhmc_chainstats, mjhmc_histogram, mjhmc_pairhist) reads its states from: the sampler's
// own sample ring, or the derived ring of a mjhmc_functionals (functionals.hip).  The handles read base pointer, slot
// bytes, slot count, dtype, D, pitch and generation through this descriptor only; particles (N, Npad), stream and
// the dwell ring are the sampler's in both cases.
#pragma once
#include "autocor.hpp"   // RingView
#include "handles.hpp"

struct mjhmc_functionals;

struct RingSource {
  const char* base = nullptr;   // slot 0 (nullptr: no ring yet)
  size_t slot_bytes = 0;
  int slots = 0;
  int dtype = MJHMC_F64;
  int D = 0, pitch = 0, esize = 8;   // esize: bytes of a stored element
  uint64_t gen = 0;             // counts the (re-)allocations of this ring
  const mjhmc_functionals* owner = nullptr;   // nullptr: the sampler's ring
  const char* name() const { return owner ? "derived ring" : "sample ring"; }
};

// functionals.hip
RingSource functionals_ring_source(const mjhmc_functionals* f);
mjhmc_sampler* functionals_sampler(const mjhmc_functionals* f);
void functionals_free_all(mjhmc_sampler* s);

inline RingSource ring_source(const mjhmc_sampler* s, const mjhmc_functionals* f) {
  if (f) return functionals_ring_source(f);
  RingSource r;
  r.base = (const char*)s->ring;
  r.slot_bytes = mat_bytes(s);
  r.slots = s->ring_slots;
  r.dtype = s->dtype;
  r.D = s->D;
  r.pitch = s->sh.pitch;
  r.esize = s->sh.esize;
  r.gen = s->ring_gen;
  return r;
}

inline RingView ring_source_view(const mjhmc_sampler* s, const RingSource& r, int slot0) {
  return RingView{r.base + (size_t)slot0 * r.slot_bytes, r.dtype, s->Npad, s->N, r.D, r.pitch};
}

// the handles of one owner among a sampler's (estimators.hip, chainstats.hip, histograms.hip, pairhist.hip): mjhmc_functionals_destroy
void estimator_free_owned(mjhmc_sampler* s, const mjhmc_functionals* f);
void chainstats_free_owned(mjhmc_sampler* s, const mjhmc_functionals* f);
void histogram_free_owned(mjhmc_sampler* s, const mjhmc_functionals* f);
void pairhist_free_owned(mjhmc_sampler* s, const mjhmc_functionals* f);
