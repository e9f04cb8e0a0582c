// The engine's pure decisions (gandiva_amd/csrc/gdv_engine_policy.h) behind a C interface, for
// tests/test_engine_policy.py: g++ alone builds it, nothing here needs HIP or a GPU.
#include "../../gandiva_amd/csrc/gdv_engine_policy.h"

extern "C" {

int host_varlen_start_path(int hint, int has_optimistic, int has_exact, int no_optflat, unsigned general_batches) {
  return gdv::engine::VarlenStartPath(hint, has_optimistic != 0, has_exact != 0, no_optflat != 0, general_batches);
}

int host_varlen_next_path(int path, unsigned err_bits, int has_exact) {
  return gdv::engine::VarlenNextPath(path, err_bits, has_exact != 0);
}

long long host_stage_capacity(long long guess, long long hint_x16, long long rows) {
  return gdv::engine::StageCapacity(guess, hint_x16, rows);
}

long long host_stage_guess_max() { return gdv::engine::kStageGuessMax; }

unsigned host_status_bits() { return gdv::engine::kNotFlat | gdv::engine::kNotAscii << 8 | gdv::engine::kSawUtf8 << 16; }

}  // extern "C"
