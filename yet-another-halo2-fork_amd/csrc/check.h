// check.h -- kernels of h2g_check_witness (check.hip): which gates, lookups, shuffles and
// copy constraints a witness leaves unsatisfied, restating MockProver::verify
// (halo2_frontend/src/dev.rs:742-1166) on the device.
#pragma once
#include "prover_kernels.h"

namespace h2g {

// Failure records {kind, index, row, 0} (the layout of h2g_check_failure) appended to
// rec[0 .. cap); *total counts every failure, also those past cap.
struct CheckSink {
  uint4* rec = nullptr;
  unsigned long long* total = nullptr;
  uint64_t cap = 0;
};

// gates (dev.rs:849-925): every gate's program segment at all n rows, rotations mod n;
// a nonzero value at row < u is kind 1, at row >= u kind 2
struct GateCheckArgs {
  const int4* prog = nullptr;
  const int2* segs = nullptr;  // device array: one program segment per gate
  int ngates = 0, n_slots = 0;
  const Fr* consts = nullptr;
  const Fr* const* load_col = nullptr;  // Lagrange columns
  const int* load_rot = nullptr;
  uint64_t n = 0, u = 0;
  CheckSink sink;
};
hipError_t check_gates(const GateCheckArgs& a, hipStream_t st);

// lookups (dev.rs:957-1052): kind 3 for every row r < u whose compressed input in[r] is not
// among the sorted canonical table values t[0 .. u)
hipError_t check_lookup_members(const Fr* in, const CanonKey* t, size_t u, uint32_t index, const CheckSink& sink,
                                hipStream_t st);
// shuffles (dev.rs:1054-1112): *flag |= 1 when the two sorted sides differ anywhere
hipError_t check_sorted_equal(const CanonKey* a, const CanonKey* b, size_t u, uint32_t* flag, hipStream_t st);

// copies (dev.rs:1114-1142): kind 5 for every copy (ltype, lindex, lrow, rtype, rindex, rrow)
// whose two cells differ; cols: the advice, fixed (from off_fixed) and instance (from
// off_instance) Lagrange columns.  The caller has checked every column and row index.
hipError_t check_copies(const Fr* const* cols, int off_fixed, int off_instance, const int32_t* copies, uint32_t count,
                        const CheckSink& sink, hipStream_t st);

}  // namespace h2g
