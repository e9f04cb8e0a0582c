// Decisions of the evaluation path that are pure arithmetic: which kernels a var-len batch runs on, and
// how big the temporaries of a two-stage plan start.  No HIP, no engine state: tests/host_engine_policy
// compiles this header alone with g++.
#pragma once
#include <algorithm>
#include <cstdint>

namespace gdv::engine {

// Status bits of the optimistic var-len kernels (gdv_device_lib.hpp): a NULL row carried bytes under a
// flat output; the ASCII assumption of the wave pre-pass broke; the exact variant did see bytes >= 0x80.
constexpr uint32_t kNotFlat = 16u, kNotAscii = 32u, kSawUtf8 = 64u;

// Var-len paths: 0 = the optimistic kernels, 1 = the wave shape's exact variant, 2 = the scanner-shaped
// (general) kernel.
//
// The path a batch STARTS on.  `hint` is where the last synchronous batch left the Projector.  Plans
// without an optimistic kernel, and every plan under GDV_NO_OPTFLAT, run on 2.  A plan without an exact
// variant takes 2 for 1.  `general_batches` counts the batches that would have started on 2: every 16th of
// them (count & 15 == 15) tries the optimistic kernels again.  Callers that never retry pass 0.
inline int VarlenStartPath(int hint, bool has_optimistic, bool has_exact, bool no_optflat, uint32_t general_batches) {
  if (!has_optimistic) return 2;
  int path = no_optflat ? 2 : hint;
  if (path == 1 && !has_exact) path = 2;
  if (path == 2 && !no_optflat && (general_batches & 15u) == 15u) path = 0;
  return path;
}

// The path AFTER a launch on `path` (0 or 1) left `err_bits`; the same path back = the batch is done.
// From 0: NOTASCII alone -> the exact variant where the plan has one; NOTASCII or NOTFLAT otherwise -> 2.
// From 1: NOTFLAT -> 2 (the exact variant's kSawUtf8 note decides where the NEXT batch starts, not this one).
inline int VarlenNextPath(int path, uint32_t err_bits, bool has_exact) {
  if (path == 0) {
    if ((err_bits & kNotAscii) && !(err_bits & kNotFlat) && has_exact) return 1;
    if (err_bits & (kNotAscii | kNotFlat)) return 2;
    return 0;
  }
  if (path == 1 && (err_bits & kNotFlat)) return 2;
  return path;
}

// First-stage temporaries of a two-stage plan: the largest first guess (int32 offsets address one byte less
// than 2 GiB; 64 bytes of slack for the padding behind the bytes) ...
constexpr int64_t kStageGuessMax = (int64_t{1} << 31) - 64;

// ... and the capacity one temporary starts with: the blanket `guess`, or, once a batch of this plan has
// run (hint_x16: bytes per row x 16 it produced), that ratio + 25 % + 4096, never more than the guess.
// A short buffer costs one retry.
inline int64_t StageCapacity(int64_t guess, int64_t hint_x16, int64_t rows) {
  if (hint_x16 <= 0) return guess;
  return std::min<int64_t>(guess, (hint_x16 * rows / 16) * 5 / 4 + 4096);
}

}  // namespace gdv::engine
