// check_sink.h -- how the checking kernels (check.hip, selfcheck.hip) append failure records to
// a CheckSink: one atomic add per wave, ordinary 16-byte vector stores.  Device code only.
#pragma once
#include "check.h"

namespace h2g {

// a wave's view of the sink: wave-uniform (every lane active at a push sees the same values;
// a wave's lowest lane takes part in all of its pushes, since rows grow with the lane)
struct WaveSink {
  unsigned long long pending = 0;  // failures counted since the buffer filled up
  bool full = false;
};

// called by all active lanes of the wave together; `fail` lanes record {kind, index, row}
static __device__ __forceinline__ void sink_push(const CheckSink& s, WaveSink& w, bool fail, uint32_t kind,
                                                 uint32_t index, uint32_t row) {
  const unsigned long long m = __ballot(fail);
  if (!m) return;
  const unsigned long long cnt = (unsigned long long)__popcll(m);
  if (w.full) {
    w.pending += cnt;
    return;
  }
  const int lane = threadIdx.x & 63;
  const int leader = __ffsll(m) - 1;
  unsigned long long base = 0;
  if (lane == leader) base = atomicAdd(s.total, cnt);
  base = __shfl(base, leader);
  if (fail) {
    const unsigned long long at = base + (unsigned long long)__popcll(m & ((1ull << lane) - 1));
    if (at < s.cap) s.rec[at] = make_uint4(kind, index, row, 0u);
  }
  if (base + cnt >= s.cap) w.full = true;
}

// once per wave, after its last push, by all lanes that reach the end of the kernel
static __device__ __forceinline__ void sink_flush(const CheckSink& s, const WaveSink& w) {
  if ((threadIdx.x & 63) == 0 && w.pending) atomicAdd(s.total, w.pending);
}

}  // namespace h2g
