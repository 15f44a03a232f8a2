// Deterministic mode (include/sibrar_hip.h: sbr_set_deterministic; reference call site utilities/utils.py:22-27).
// A process-wide flag: while it is on, no entry point launches a kernel that adds floats or doubles with atomics in arrival order.
// An entry point with such a path either takes its fixed-order form or fails with "<entry point>: no deterministic form".
// Both modes count the arrival-order launches they make (sbr_nondeterministic_launches): the counter is how a test tells that a
// training really stayed on fixed-order paths instead of agreeing with itself by luck.
#pragma once
#include "common.h"

bool sbr_det_on();
void sbr_note_arrival_order();                     // one more launch that accumulates floats in arrival order

// "no deterministic form" unless the flag is off; then counts the arrival-order launch the caller is about to make
#define SBR_ARRIVAL_ORDER(entry)                                                    \
  do {                                                                              \
    SBR_REQUIRE(!sbr_det_on(), "%s: no deterministic form (sbr_set_deterministic is on)", entry); \
    sbr_note_arrival_order();                                                       \
  } while (0)

// Scratch of the fixed-order forms, owned by the library: one grow-only block per device and purpose, handed to the launches of ONE
// entry-point call and free again when they have run — calls on one stream (or one captured step) follow each other, so they share it;
// deterministic work on two streams of a device at the same time is not supported. An outgrown block is retired, never freed: captured
// steps keep its address. Growing needs an allocation, which a capturing stream cannot make: nullptr + error then (run one plain step
// first, as for every other persistent buffer of the step).
#define SBR_SCRATCH_COLRED 0
#define SBR_SCRATCH_SCATTER 1
#define SBR_SCRATCH_LOSS 2
void* sbr_det_scratch(int purpose, size_t bytes, hipStream_t s, const char* entry);

// fixed-slot column reduction, second half: replica 1 of the column-reduction workspace ws ([KD totals][SBR_COLRED_REP][KD]) receives
// the sum over slots [nslots][KD] in slot order (the other replicas are zero: the workspace contract), so that the usual finishing
// kernel of the caller runs unchanged behind it
int sbr_det_fold_slots(const double* slots, int nslots, int KD, double* ws, hipStream_t s, const char* entry);

// out[0] = sum of partials[0 .. n) in a fixed pattern (one workgroup)
int sbr_det_sum_partials(const double* partials, int n, double* out, hipStream_t s, const char* entry);

// dW[rows[j], :] += dOut[ii(j), :] with every destination row owned by one wave that adds its source rows in ascending j
int sbr_det_scatter_add_rows(const float* dOut, long ldo, const int* in_idx, const int* rows, float* dW, long ldw, long n, int D,
                             hipStream_t s, const char* entry);
