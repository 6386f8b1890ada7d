// The tile traffic of the row-form kernels: 64 rows between HBM and the lanes that own them, through LDS.
#pragma once
#ifndef __HIPCC_RTC__  // hipRTC pre-includes the device runtime and has no header search path to it
#include <hip/hip_runtime.h>
#endif
#include <stdint.h>

namespace mjhmc {

// order the wavefront's LDS traffic: the tile is written by one set of lanes and read by another.  LDS operations of a wave
// execute in order; what is needed is that the compiler keeps them in order and that the writes have landed -- NOT a
// fence: a release fence also waits for the wave's global stores (vmcnt(0): the X rows' way to HBM, 2-5 us, in front of
// the V rows' pass through the tile).
__device__ __forceinline__ void wave_lds_fence() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_wave_barrier();
}

// The tile traffic of the row-form kernels: 64 rows between HBM (row order: chunk q = i * 64 + lane of the tile's 64 * CH
// chunks, (row, col) = (q / CH, q % CH)) and the lanes that own them, through tile[64 * 16] (slot row * 16 + (col ^ (row & 15))).
// FULL: every row has all its chunks (ndims 31, 32 / 15, 16): no predicate anywhere, and i = P * m + k walks rows
// 16 m + RPI * k + lane / RC, so a row-order slot is one of P per-lane bases + m * 256.
template <typename T, int E, int LOGG, bool FULL>
struct RowTile {
  static_assert(sizeof(T) == 8, "float64 rows");
  static constexpr int G = 1 << LOGG, C = E / 2, RC = C * G;   // RC: chunks of a full row
  static_assert(RC == 8 || RC == 16, "rows of 8 or 16 chunks");
  static constexpr int RPI = 64 / RC, P = 16 / RPI;
  using V = double2;
  // the chunks on their way between HBM and the tile: ONE vector value, not an array (an array of 16 chunks indexed from
  // unrolled loops was left in scratch memory -- 512 bytes written and read back per wave and matrix)
  using Stage = double __attribute__((ext_vector_type(2 * RC)));
  V* tile;
  int CH, pitch;
  int64_t N;

  // Every phase forms its own addresses from an opaque copy of the lane index: formed once, the compiler carries 16 + 16 LDS
  // and 2 x 16 global addresses across the trajectory loop in scratch memory -- and each reload in the store phase is a
  // vmcnt(0) wait, i.e. it waits for the previous STORE to reach memory (16 round trips per matrix).
  static __device__ __forceinline__ int fresh_lane() {
    int l = threadIdx.x & 63;   // (the relay kernel's workgroups have four waves)
    asm volatile("" : "+v"(l));
    return l;
  }
  struct Walk {   // short rows: (row, col) stepped, not divided
    int row, col, drow, dcol, CH;
    __device__ __forceinline__ void step() {
      col += dcol;
      row += drow;
      if (col >= CH) {
        col -= CH;
        row += 1;
      }
    }
  };
  __device__ __forceinline__ Walk walk0(int l) const {
    Walk w;
    w.CH = CH;
    w.row = l / CH;
    w.col = l - w.row * CH;
    w.drow = 64 / CH;
    w.dcol = 64 - w.drow * CH;
    return w;
  }
  // HBM rows -> registers, still in row order.  All loads are issued before anything waits; the passes a short row does
  // not need re-read the tile's last chunk and are dropped.
  __device__ __forceinline__ void fetch(const T* M, int64_t base, Stage& t) const {
    const int l = fresh_lane();
    const char* tb = reinterpret_cast<const char*>(M + (size_t)base * pitch);
    const uint32_t last_chunk = (uint32_t)(64 * CH - 1) * 16u;
#pragma unroll
    for (int i = 0; i < RC; ++i) {
      uint32_t off = (uint32_t)(i * 64 + l) * 16u;
      if (!FULL) off = min(off, last_chunk);
      const V q = *reinterpret_cast<const V*>(tb + off);
      t[2 * i] = q.x;
      t[2 * i + 1] = q.y;
    }
  }
  // the listed particles' rows (p_lane: the particle whose row this lane will own), RC lanes per row
  __device__ __forceinline__ void fetch_listed(const T* M, int p_lane, Stage& t) const {
    const int l = fresh_lane();
    Walk w = walk0(l);
#pragma unroll
    for (int i = 0; i < RC; ++i) {
      const int pr = __shfl(p_lane, FULL ? w.row : min(w.row, 63));
      const V q = *reinterpret_cast<const V*>(M + (size_t)pr * pitch + w.col * 2);
      t[2 * i] = q.x;
      t[2 * i + 1] = q.y;
      w.step();
    }
  }
  // ... through the tile into the lane that owns the row: r[j] = what lane j of the particle's group holds elsewhere
  __device__ __forceinline__ void to_rows(const Stage& t, T (&r)[G][E]) const {
    const int l = fresh_lane();
    if constexpr (FULL) {
      const int h = l / RC, col = l % RC;
#pragma unroll
      for (int k = 0; k < P; ++k) {
        const int rk = RPI * k + h, slot = rk * 16 + (col ^ rk);
#pragma unroll
        for (int m = 0; m < RC / P; ++m) tile[slot + m * 256] = V{t[2 * (P * m + k)], t[2 * (P * m + k) + 1]};
      }
    } else {
      Walk w = walk0(l);
#pragma unroll
      for (int i = 0; i < RC; ++i) {
        if (i < CH) tile[w.row * 16 + (w.col ^ (w.row & 15))] = V{t[2 * i], t[2 * i + 1]};
        w.step();
      }
    }
    wave_lds_fence();
    read_own(r);
    wave_lds_fence();
  }
  // the lane's own row of the tile <-> registers
  __device__ __forceinline__ void read_own(T (&r)[G][E]) const {
    const int l = fresh_lane();
    const int mine = l * 16, key = l & 15;
#pragma unroll
    for (int c = 0; c < RC; ++c) {
      V q = tile[mine + (c ^ key)];
      if (!FULL && c >= CH) q = V{0, 0};
      r[c % G][(c / G) * 2] = q.x;
      r[c % G][(c / G) * 2 + 1] = q.y;
    }
  }
  __device__ __forceinline__ void write_own(const T (&r)[G][E]) const {
    const int l = fresh_lane();
    const int mine = l * 16, key = l & 15;
#pragma unroll
    for (int c = 0; c < RC; ++c) tile[mine + (c ^ key)] = V{r[c % G][(c / G) * 2], r[c % G][(c / G) * 2 + 1]};
  }
  // registers -> the tile -> registers in row order (from_rows), then HBM (store).  Both matrices of a state go through
  // the tile before the first store is issued: a wait for anything older than a store (a reloaded spill on some path of
  // the compiler's, say) is then a wait for that store's round trip to memory.
  __device__ __forceinline__ void from_rows(const T (&r)[G][E], Stage& t) const {
    write_own(r);
    wave_lds_fence();
    const int l = fresh_lane();
    if constexpr (FULL) {
      const int h = l / RC, col = l % RC;
#pragma unroll
      for (int k = 0; k < P; ++k) {
        const int rk = RPI * k + h, slot = rk * 16 + (col ^ rk);
#pragma unroll
        for (int m = 0; m < RC / P; ++m) {
          const V q = tile[slot + m * 256];
          t[2 * (P * m + k)] = q.x;
          t[2 * (P * m + k) + 1] = q.y;
        }
      }
    } else {
      Walk w = walk0(l);
#pragma unroll
      for (int i = 0; i < RC; ++i) {
        const V q = tile[min(w.row, 63) * 16 + (w.col ^ (w.row & 15))];
        t[2 * i] = q.x;
        t[2 * i + 1] = q.y;
        w.step();
      }
    }
    wave_lds_fence();
  }
  __device__ __forceinline__ void store(T* M, int64_t base, const Stage& t) const {
    const int l = fresh_lane();
    char* tb = reinterpret_cast<char*>(M + (size_t)base * pitch);
    const int live_rows = (int)min((int64_t)64, N - base);   // < 64 in the batch's last tile only
    if (FULL && live_rows == 64) {
#pragma unroll
      for (int i = 0; i < RC; ++i) *reinterpret_cast<V*>(tb + (uint32_t)(i * 64 + l) * 16u) = V{t[2 * i], t[2 * i + 1]};
    } else {
      Walk w = walk0(l);
#pragma unroll
      for (int i = 0; i < RC; ++i) {
        if ((FULL || i < CH) && w.row < live_rows) *reinterpret_cast<V*>(tb + (uint32_t)(i * 64 + l) * 16u) = V{t[2 * i], t[2 * i + 1]};
        w.step();
      }
    }
  }
};

}  // namespace mjhmc
