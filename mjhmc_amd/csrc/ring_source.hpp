// The host side the ring statistics share.
//
// RingSource: where an accumulator handle (mjhmc_estimator, mjhmc_chainstats, mjhmc_histogram, mjhmc_pairhist) reads its
// states from: the sampler's own sample ring, or the derived ring of a mjhmc_functionals (functionals.hip).  The handles
// read base pointer, slot bytes, slot count, dtype, D, pitch and generation through this descriptor only; particles (N,
// Npad), stream and the dwell ring are the sampler's in both cases.
//
// RingAccumulator: what those four handles have in common (estimators.hip, chainstats.hip, histograms.hip, pairhist.hip
// derive from it) -- the sampler's one list of them, the argument checks of an accumulate call (acc_begin), the flag
// read-back that ends it (acc_end) and destroy.
//
// pow2ceil / ilog2 and dispatch_dtype: the launch plumbing of every pass over ring rows.
#pragma once
#include <algorithm>

#include "autocor.hpp"   // RingView
#include "handles.hpp"

inline int pow2ceil(int v) {
  int p = 1;
  while (p < v) p <<= 1;
  return p;
}

inline int ilog2(int v) {   // of a power of two (rounds up otherwise)
  int l = 0;
  while ((1 << l) < v) ++l;
  return l;
}

// f(ElemTag<T>()) with T the element type of dtype code `dtype`: `typename decltype(tag)::type` names the kernel instance
template <typename T>
struct ElemTag {
  typedef T type;
};
template <typename F>
inline void dispatch_dtype(int dtype, F&& f) {
  if (dtype == MJHMC_F64)
    f(ElemTag<double>());
  else if (dtype == MJHMC_F32)
    f(ElemTag<float>());
  else
    f(ElemTag<__bf16>());
}

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

// ---------------------------------------------------------------------------------------------------------------------
// What the accumulator handles share
// ---------------------------------------------------------------------------------------------------------------------
struct RingAccumulator {
  mjhmc_sampler* s;
  const mjhmc_functionals* fn;   // whose derived ring the states come from; nullptr: the sampler's own ring
  uint64_t ring_gen;             // that ring at create: plans and buffers are sized for it
  const char* kind;              // "estimator", "pairhist": the handle's name in mjhmc_<kind>_create
  const char* noun;              // "estimator", "pair histogram": what a message calls it
  int* bad = nullptr;            // device flag a pass raises to refuse its block
  int64_t n_states = 0;          // states added so far (mjhmc_chainstats counts per part instead)
  RingAccumulator(const char* kind_, const char* noun_, mjhmc_sampler* s_, const mjhmc_functionals* fn_, const RingSource& src)
      : s(s_), fn(fn_), ring_gen(src.gen), kind(kind_), noun(noun_) {}
  virtual ~RingAccumulator() { free_device({bad}); }   // (a derived handle frees its own buffers the same way)
  static void free_device(std::initializer_list<void*> ptrs) {
    for (void* p : ptrs)
      if (p) (void)hipFree(p);
  }
};

// every handle of a sampler: mjhmc_sampler_destroy, after functionals_free_all
inline void accumulators_free_all(mjhmc_sampler* s) {
  for (RingAccumulator* h : s->accumulators) delete h;
  s->accumulators.clear();
}

// the handles of one owner among a sampler's: mjhmc_functionals_destroy
inline void accumulators_free_owned(mjhmc_sampler* s, const mjhmc_functionals* f) {
  auto& v = s->accumulators;
  const auto mid = std::stable_partition(v.begin(), v.end(), [f](const RingAccumulator* h) { return h->fn != f; });
  std::for_each(mid, v.end(), [](RingAccumulator* h) { delete h; });
  v.erase(mid, v.end());
}

inline int acc_no_ring(const mjhmc_functionals* fn) {
  return mjhmc_fail(MJHMC_ERR_INVALID, fn ? "the functionals have no derived ring yet (call mjhmc_functionals_ring_alloc first)"
                                          : "the sampler has no sample ring yet (call mjhmc_ring_alloc first)");
}

// the end of a create that allocated everything
template <typename H>
inline int acc_created(H* h, H** out) {
  h->s->accumulators.push_back(h);
  *out = h;
  return 0;
}

inline int acc_destroy(RingAccumulator* h) {
  if (!h) return 0;
  mjhmc_sampler* s = h->s;
  (void)hipSetDevice(s->ctx->device);
  if (s->stream) (void)hipStreamSynchronize(s->stream);
  s->accumulators.erase(std::remove(s->accumulators.begin(), s->accumulators.end(), h), s->accumulators.end());
  delete h;
  return 0;
}

// the argument checks of an accumulate call over state slots [x_slot0, x_slot0 + n) and dwell slots [w_slot0, w_slot0 + n)
// (w_slot0 = -1: unit weights); *src is the handle's ring as it is now
inline int acc_begin(const RingAccumulator* h, int x_slot0, int w_slot0, int n, RingSource* src) {
  const mjhmc_sampler* s = h->s;
  *src = ring_source(s, h->fn);
  if (h->ring_gen != src->gen)
    return mjhmc_fail(MJHMC_ERR_INVALID, std::string("the ") + src->name() + " was re-allocated after mjhmc_" + h->kind +
                                             "_create: create a new " + h->noun);
  if (n < 1) return mjhmc_fail(MJHMC_ERR_INVALID, "n must be >= 1");
  if (x_slot0 < 0 || (int64_t)x_slot0 + n > src->slots)
    return mjhmc_fail(MJHMC_ERR_INVALID, "state slots [" + std::to_string(x_slot0) + ", " + std::to_string((int64_t)x_slot0 + n) +
                                             ") are outside the ring of " + std::to_string(src->slots));
  if (w_slot0 < -1 || (w_slot0 >= 0 && (int64_t)w_slot0 + n > s->ring_slots))
    return mjhmc_fail(MJHMC_ERR_INVALID, "dwell slots [" + std::to_string(w_slot0) + ", " + std::to_string((int64_t)w_slot0 + n) +
                                             ") are outside the ring of " + std::to_string(s->ring_slots) +
                                             " (-1 asks for unit weights)");
  return 0;
}

// the block's weights, or nullptr for unit weights
inline const double* acc_weights(const RingAccumulator* h, int w_slot0) {
  return w_slot0 >= 0 ? h->s->dwell_ring + (size_t)w_slot0 * h->s->Npad : nullptr;
}

// the flag of the passes just launched, read back (one synchronisation) and cleared when it is up
inline int acc_take_flag(RingAccumulator* h, int* bad) {
  mjhmc_sampler* s = h->s;
  *bad = 0;
  HIPCHK(hipMemcpyAsync(bad, h->bad, sizeof(int), hipMemcpyDeviceToHost, s->stream));
  HIPCHK(hipStreamSynchronize(s->stream));
  if (*bad) HIPCHK(hipMemsetAsync(h->bad, 0, sizeof(int), s->stream));
  return 0;
}

// the end of an accumulate call: on_bad(flag) words the refusal of a block that raised the flag (it added nothing)
template <typename OnBad>
inline int acc_end(RingAccumulator* h, int n, OnBad on_bad) {
  int bad = 0;
  TRY(acc_take_flag(h, &bad));
  if (bad) return on_bad(bad);
  h->n_states += (int64_t)n * h->s->N;
  return 0;
}

// the refusal of the moment and chain passes
inline int acc_nonfinite_dwell(int w_slot0, int n) {
  return mjhmc_fail(MJHMC_ERR_NONFINITE, "a dwelling time in dwell slots [" + std::to_string(w_slot0) + ", " +
                                             std::to_string(w_slot0 + n) +
                                             ") is not finite (a state whose total jump rate is zero): nothing of this block was added");
}
