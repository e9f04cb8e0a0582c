// Tier 0 (round 6): a post-fix program for the ahead-of-time interpreter kernel (gdv_tier0.hip) — what a Projector /
// Filter evaluates with while hipRTC compiles its specialised kernel.  Built at Make from the same expression trees, over
// the same argument block as the generated kernel.  Covers every registry signature whose parameters and result are
// fixed-width and not decimal, that cannot raise and is not a hash: arithmetic (add / subtract / multiply, negative, abs,
// greatest, least, integer mod, bitwise), the comparisons, the null handling (isnull ... isnumeric, istrue ..., nvl,
// is_[not_]distinct_from), the numeric and the fixed-width date casts, the float64 math, every date / time function
// (extract*, date_trunc_*, last_day, timestampadd / diff, date_add / sub, datediff, to_timestamp / to_time), IN over
// fixed-width values, if / else, AND / OR and literals — in row mode and, for projectors, over a selection vector.
// Outside: functions that can raise (divide, float mod, two-argument log), hashes, decimal128, var-len plans and the
// rows_word / cast_x86_indefinite options: those plans have no tier 0 and wait for their compilation as before.
#pragma once
#include <cstdint>

namespace gdv {
namespace tier0 {

enum TypeKind : int { kTBool = 0, kTI8, kTU8, kTI16, kTU16, kTI32, kTU32, kTI64, kTU64, kTF32, kTF64 };
enum Op : int {
  kLoad = 1, kLit, kAdd, kSub, kMul, kCmp, kCast, kNot, kIsNull, kIsNotNull, kAnd2, kOr2, kIf, kOut, kFilterOut,
  // the rest of the fixed-width registry
  kCall1,     // a | b << 8 = function id (gdv_tier0_fns.inc): one operand, validity unchanged
  kCall2,     // a | b << 8 = function id: two operands, validity words ANDed
  kGen1,      // a = Gen1, b = type
  kGen2,      // a = Gen2, b = type
  kBoolTest,  // a = BoolTest: reads the operand's validity per lane, never null
  kDistinct,  // a = 1: is_not_distinct_from, b = operand type: reads both validities per lane, never null
  kNvl,       // b = type: validity by ballot
  kIn         // a = first literal slot, b = number of slots, c = type: the operand's zero-extended bit image among them
};
enum Cmp : int { kEq = 0, kNe, kLt, kLe, kGt, kGe };
// type-generic functions: the type is an operand of the instruction
enum Gen1 : int { kNegative = 0, kAbs, kBitNot };
enum Gen2 : int { kGreatest = 0, kLeast, kBitAnd, kBitOr, kBitXor };
enum BoolTest : int { kIsTrue = 0, kIsFalse, kIsNotTrue, kIsNotFalse };
// function ids of kCall1 / kCall2: the position in gdv_tier0_fns.inc
enum Fn : int {
#define GDV_T0_F1(sym, R, A) kFn_##sym,
#define GDV_T0_F2(sym, R, A, B) kFn_##sym,
#include "gdv_tier0_fns.inc"
#undef GDV_T0_F1
#undef GDV_T0_F2
  kNumFns
};

constexpr int kMaxDepth = 12;     // operand stack entries (LDS: 4 waves x 12 x 64 x 8 bytes = 24 KiB per workgroup)
constexpr int kMaxCode = 256;     // instructions: op | a << 8 | b << 16 | c << 24
constexpr int kMaxLits = 92;      // literals and IN-list values together: what the 4 KiB of kernel arguments leave room for
constexpr int kMaxBlock = 2048;   // bytes of the argument block (ArgLayout::total())
// where the interpreter reads the generated kernels' argument block (gdv_planner.h: ArgLayout; gdv_tier0.cc asserts the match)
constexpr int kBlockN = 0, kBlockSel = 16, kBlockMask = 24, kBlockCounts = 32, kBlockAux2 = 56, kBlockHeader = 64,
              kBlockInStride = 64, kBlockOutStride = 32;

// passed BY VALUE (kernel arguments: 3832 bytes + the 256 hidden ones the compiler appends, of the 4 KiB a launch may carry) — no
// allocation, no upload
struct Args {
  uint8_t block[kMaxBlock] __attribute__((aligned(8)));  // the generated kernel's own argument block (ArgLayout)
  uint32_t code[kMaxCode];
  uint64_t lits[kMaxLits];
  int32_t ncode, n_in, filter, subtiles;
  int32_t selw;      // selection-mode projector: bytes per index of the selection vector (2 / 4 / 8); 0: row mode
  int32_t extended;  // the program holds an op past kFilterOut: picks the kernel instantiation (gdv_tier0.hip)
};
static_assert(sizeof(Args) + 256 <= 4096, "tier-0 arguments + the hidden kernel arguments must fit the 4 KiB of a launch");

}  // namespace tier0
}  // namespace gdv

// ---- host side (gdv_tier0.cc): the program of a plan, or "this plan has no tier 0" ----------------------------------
#ifndef __HIP_DEVICE_COMPILE__
#include <hip/hip_runtime_api.h>

#include <string>
#include <vector>

#include "gdv_node.h"
#include "gdv_planner.h"

namespace gdv {

// Builds the program for `exprs` (projector outputs in order) or for a filter's condition (filter = true: exprs holds the
// one condition) over the argument block layout and input slots of `plan`.  False — with the reason in *why — when a
// node, a type or the plan's shape is outside what the interpreter takes; the caller then has no tier 0 for this plan.
bool BuildTier0Program(const Schema& schema, const std::vector<ExpressionPtr>& exprs, bool filter, const KernelPlan& plan,
                       tier0::Args* out, std::string* why);

// the program as text, one instruction per line (diagnostics, tests)
std::string DescribeTier0Program(const tier0::Args& prog);
// evaluations that ran on tier 0 (process-wide)
int64_t Tier0Launches();
void CountTier0Launch();

// gdv_tier0.hip
hipError_t LaunchTier0(const tier0::Args& args, int64_t rows, int num_cus, hipStream_t stream);

}  // namespace gdv
#endif
