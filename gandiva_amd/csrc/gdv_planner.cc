#include "gdv_planner_internal.h"

#include <algorithm>
#include <cstdlib>

namespace gdv {

using namespace planner;

thread_local bool planner::tl_ablation = false;  // (the one definition: gdv_planner_internal.h declares it)

// ------------------------------------------------------------------ options

CodegenOptions CodegenOptions::FromEnv() {
  CodegenOptions o;
  if (const char* s = std::getenv("GDV_U")) {
    // powers of two only: the index-emission kernel walks 64-word groups (gdv_kernels.hip)
    int u = std::max(1, std::min(16, atoi(s)));
    while (u & (u - 1)) u &= u - 1;
    o.subtiles = u;
    o.subtiles_forced = true;
  }
  if (const char* s = std::getenv("GDV_WAVES")) {
    o.waves = std::max(1, std::min(16, atoi(s)));
    o.waves_forced = true;
  }
  if (const char* s = std::getenv("GDV_NT")) o.nontemporal = atoi(s) != 0;
  if (const char* s = std::getenv("GDV_NTLOAD")) o.nt_loads = atoi(s) != 0;
  if (const char* s = std::getenv("GDV_NO_LDS_MIRROR")) o.lds_mirror = atoi(s) == 0;
  o.no_inline_string_args = std::getenv("GDV_NO_INLINE_STRING_ARGS") != nullptr;
  o.no_wave_shape = std::getenv("GDV_NO_WAVE_SHAPE") != nullptr;
  o.wave_bytefree_only = std::getenv("GDV_WAVE_BYTEFREE_ONLY") != nullptr;
  o.ablation = std::getenv("GDV_ABLATION") != nullptr;
  o.runtime_needles = std::getenv("GDV_RUNTIME_NEEDLES") != nullptr;
  o.prepass_rolled = std::getenv("GDV_PREPASS_ROLLED") != nullptr;
  o.no_sel_wave = std::getenv("GDV_NO_SEL_WAVE") != nullptr;
  if (const char* s = std::getenv("GDV_PREPASS_AHEAD")) o.prepass_ahead = atoi(s) != 0;
  if (const char* s = std::getenv("GDV_CAST_X86_INDEFINITE")) o.cast_x86_indefinite = atoi(s) != 0;
  if (const char* s = std::getenv("GDV_UTF8_CASE")) o.utf8_case = atoi(s) != 0;
  if (const char* s = std::getenv("GDV_SWEEP_GROUP")) o.sweep_group = std::max(1, std::min(8, atoi(s)));
  if (const char* s = std::getenv("GDV_FP_EXPERIMENT")) o.fp_experiment = atoi(s);
  if (const char* s = std::getenv("GDV_FP_K")) o.fp_rounds = std::max(1, std::min(8, atoi(s)));
  if (const char* s = std::getenv("GDV_FP_WINDOW")) o.fp_window_bytes = std::max(0, std::min(16384, atoi(s)));
  return o;
}

std::string CodegenOptions::Key() const {
  return "u" + std::to_string(subtiles) + "w" + std::to_string(waves) + (nontemporal ? "nt" : "") +
         (nt_loads ? "ntl" : "") + (lds_mirror ? "" : "nm") + (subtiles_forced ? "U" : "") + (waves_forced ? "W" : "") +
         (no_inline_string_args ? "ni" : "") + (no_wave_shape ? "nw" : "") + (wave_bytefree_only ? "bf" : "") +
         (ablation ? "abl" : "") + (runtime_needles ? "rn" : "") + (prepass_rolled ? "pr" : "") + (rows_word ? "rw" : "") + (no_sel_wave ? "nsw" : "") + (prepass_ahead ? "" : "npa") + (fp_experiment ? "fx" + std::to_string(fp_experiment) : "") + (fp_rounds != 3 ? "k" + std::to_string(fp_rounds) : "") +
         (fp_window_bytes != 9984 ? "fw" + std::to_string(fp_window_bytes) : "") + (cast_x86_indefinite ? "xi" : "") + (sweep_group != 1 ? "sg" + std::to_string(sweep_group) : "") + (utf8_case ? "uc" : "");
}

namespace {

enum class StringShape { kScanner, kWaveMain, kWavePrepass, kWaveMainExact, kWavePrepassExact };

// Is the value of `n` — and its validity — computable without reading a single var-len BYTE once
// every string is assumed ASCII?  (offsets, validity bitmaps, fixed-width values and literals are
// free.)  Outputs with that property let a plan take the wave shape: their byte totals come from a
// pre-pass over the offsets.
bool ByteFree(const Node& n, bool utf8_case) {
  static const std::set<std::string> over_strings = {
      "substr", "substring", "left", "right", "upper", "lower", "octet_length", "bit_length", "char_length",
      "length", "lengthUtf8", "castVARCHAR", "concat", "concatOperator", "reverse", "initcap", "lpad", "rpad", "isnull", "hashSHA256", "sha256",
      "hashSHA1", "sha1", "sha", "hashMD5", "md5", "repeat",
      "mask", "mask_first_n", "mask_last_n", "mask_show_first_n", "mask_show_last_n",  // (the length is the text's)
      "hex", "to_hex", "unhex", "from_hex", "base64",  // (unbase64 reads the row's last word for the padding)
      "isnotnull"};
  switch (n.kind()) {
    case NodeKind::kField:
    case NodeKind::kLiteral:
      return true;
    case NodeKind::kFunction: {
      auto& fn = static_cast<const FunctionNode&>(n);
      bool takes_strings = false;
      for (auto& c : fn.children()) {
        if (!ByteFree(*c, utf8_case)) return false;
        takes_strings |= c->return_type().is_varlen();
      }
      if (utf8_case && (fn.name() == "upper" || fn.name() == "lower")) return false;  // the length follows from the bytes
      return !takes_strings || over_strings.count(fn.name()) != 0;
    }
    case NodeKind::kIf: {
      auto& i = static_cast<const IfNode&>(n);
      return ByteFree(*i.condition(), utf8_case) && ByteFree(*i.then_node(), utf8_case) && ByteFree(*i.else_node(), utf8_case);
    }
    case NodeKind::kBoolean:
      for (auto& c : static_cast<const BooleanNode&>(n).children())
        if (!ByteFree(*c, utf8_case)) return false;
      return true;
    case NodeKind::kIn: {
      auto& in = static_cast<const InNode&>(n);
      return !in.value_type().is_varlen() && ByteFree(*in.eval(), utf8_case);
    }
  }
  return false;
}

// Can one argument block serve both kernels?  (the same inputs, literals and constants bound, in the same order)
bool SameBindings(const KernelPlan& a, const KernelPlan& b) {
  return a.input_fields == b.input_fields && a.input_needs_values == b.input_needs_values &&
         a.input_needs_validity == b.input_needs_validity && a.literals == b.literals && a.const_block == b.const_block;
}

// One shape of a projector's kernel.  kWavePrepass generates only the expressions listed in
// `only` (the scanned var-len outputs of the main kernel, in that order = segment order).
Status PlanProjectorShape(const Schema& schema, const std::vector<ExpressionPtr>& exprs, SelectionMode mode,
                          const CodegenOptions& opts, StringShape shape, const std::vector<int>* only,
                          KernelPlan* plan, std::vector<VarlenOut>* varlen_outs, int compact_from) {
  plan->kind = KernelKind::kProject;
  plan->mode = mode;
  plan->opts = opts;
  plan->compact_from = compact_from;
  CodeGen cg(schema, mode, opts);
  cg.compact_from_ = compact_from;
  cg.exact_ascii_ = shape == StringShape::kWaveMainExact || shape == StringShape::kWavePrepassExact;
  if (shape == StringShape::kWaveMainExact) shape = StringShape::kWaveMain;
  if (shape == StringShape::kWavePrepassExact) shape = StringShape::kWavePrepass;
  cg.no_hooks_ = shape == StringShape::kWavePrepass;
  cg.bake_needles_ = shape != StringShape::kScanner && !opts.runtime_needles;
  cg.replace_hits_ = shape != StringShape::kScanner && opts.lds_mirror && mode == SelectionMode::kNone;
  WordAccumulators accs;
  std::ostringstream after_loop, before_loop, in_pass, after_rows;
  std::vector<std::string> strings;
  int num_staged = 0, num_scanned = 0;
  const bool wave = shape != StringShape::kScanner;
  const bool prepass = shape == StringShape::kWavePrepass;
  if (!prepass)
    for (auto& e : exprs) plan->has_varlen_output |= e->result().type.is_varlen();
  // 64 lengths below 2^25 cannot wrap the 32-bit scan; otherwise the total is taken on 16-bit
  // halves and saturates (the host rejects outputs of 2 GiB or more)
  auto tile_total = [](const std::string& ln, const std::string& inc) {
    return "(__builtin_expect(__ballot(" + ln + " >= (1 << 25)) != 0, 0) ? gdv_tile_total(" + ln +
           ") : (gdv_uint32)gdv_wave_last(" + inc + "))";
  };
  for (size_t e = 0; e < exprs.size(); e++) {
    if (only != nullptr && std::find(only->begin(), only->end(), static_cast<int>(e)) == only->end()) continue;
    Val v;
    cg.Stmt("// @expr_" + std::to_string(e));
    GDV_RETURN_NOT_OK(cg.Gen(*exprs[e]->root(), "", &v));
    const DataType& t = exprs[e]->result().type;
    if (!prepass) plan->output_types.push_back(t);
    strings.push_back(exprs[e]->ToString());
    const std::string E = std::to_string(e);
    if (t.is_varlen()) {
      // The row's bytes are one view, or the pieces of a concat written back to back; lengths are
      // prefix-summed inside the wave on the DPP data path.
      const std::string ok = cg.Tmp("bool", CodeGen::AndFull("live", cg.LaneValid(v)));
      VarlenOut vo;
      vo.e = static_cast<int>(e);
      const bool flat_cand = v.pieces.empty() && v.col_slot >= 0 && !cg.selection();
      const bool has_window = !flat_cand && num_staged < 3;  // LDS staging windows per wave
      std::vector<std::pair<std::string, std::string>> pieces = v.pieces;
      if (pieces.empty()) pieces.emplace_back(v.v, "");
      std::string total;
      std::vector<std::string> pv;
      auto emit_pieces = [&] {
        for (size_t q = 0; q < pieces.size(); q++) {
          const std::string name = "pv" + E + "_" + std::to_string(q);
          pv.push_back(name);
          cg.Stmt("gdv_str " + name + " = " + pieces[q].first + ";");
          cg.Stmt("if (!(" + CodeGen::AndFull(ok, pieces[q].second) + ")) " + name + ".len = 0;");
          total += (q ? " + " : "") + name + ".len";
        }
      };
      if (prepass) {
        // lengths only: one byte total per wave tile -> counts[segment][wave tile]
        emit_pieces();
        const std::string S = std::to_string(num_scanned++);
        // (lengths add up per lane across the sub-tiles; ONE wave reduction per tile.  Exact whenever
        // the tile stays below 2^31 bytes — the main kernel's running total then agrees — and at
        // least 2^31-1 otherwise, which the host rejects)
        in_pass << "  gdv_int32 run" << E << " = 0;  // this lane's bytes over the sub-tiles (saturates at 2^31-1)\n";
        cg.Stmt("run" + E + " = gdv_sat_add31(run" + E + ", " + total + ");");
        after_rows << "  { const gdv_uint32 t = gdv_tile_total(run" << E << ");\n"
                   << "    if (lane == 0) A.counts[" << S << " * seg_stride + wt] = t > 0x7fffffffu ? 0x7fffffffu : t; }\n";
        cg.varlen_outs_.push_back(vo);
        continue;
      }
      if (wave && flat_cand) {
        // the output IS the (mapped) input span: offsets = the input's, rebased; bytes leave from the
        // byte sweep.  Only wrong if a NULL row carries bytes: NOTFLAT, the host re-runs (general kernel).
        vo.flat_slot = v.col_slot;
        vo.flat_map = v.col_map;
        const std::string K = std::to_string(v.col_slot);
        const int vidx = static_cast<int>(cg.varlen_outs_.size());
        before_loop << "  gdv_uint64 fb" << E << " = 0;  // rows that drop bytes of the input span (nulls with a length)\n";
        cg.Stmt("if (live) outo" + E + "[row] = oa" + K + "[u] - so0_" + K + ";");
        cg.Stmt("fb" + E + " |= __ballot(!" + ok + " && ob" + K + "[u] > oa" + K + "[u]);");
        after_rows << "  if (fb" << E << " != 0 && lane == 0) gdv_raise_bits(A.err, GDV_ERR_NOTFLAT);\n"
                   << "  if (last_tile && lane == 0) {  // closing offset + byte total of a flat output\n"
                   << "    outo" << E << "[n] = sp1" << K << " - so0_" << K << ";\n"
                   << "    ((gdv_uint64*)A.counts)[" << vidx << "] = (gdv_uint64)(sp1" << K << " - so0_" << K << ");\n"
                   << "  }\n";
        cg.varlen_outs_.push_back(vo);
      } else if (wave) {
        // scanned output: the wave tile's base comes from the pre-pass + scan (one scalar load), so
        // bytes can leave as soon as they are staged.  The LDS window STREAMS: when the next
        // sub-tile's rows would not fit behind what is staged, the staged bytes are flushed
        // (coalesced, to their final place) and the window starts over at that sub-tile — outputs
        // of up to GDV_OUT_WIN / 64 bytes per row on average (32 at 4 sub-tiles, 64 at 8) never
        // touch the per-row direct copy, whatever the tile's total is (rounds 1-2 and the scanner
        // shape: a tile above 8 bytes per row takes a second row pass with scattered stores — what
        // made upper(concat(s, '-', s)) cost 4.1 ms at 5 * 10^7 rows).  A single sub-tile wider than
        // the whole window is copied row by row, in place.
        emit_pieces();
        const std::string S = std::to_string(num_scanned++);
        vo.segment = num_scanned - 1;
        before_loop << "  const gdv_int64 base" << E << " = (gdv_int64)A.mask[" << S << " * seg_stride + wt];\n"
                    << "  gdv_int32 run" << E << " = 0;   // bytes this wave tile has produced so far (saturates at 2^31-1)\n"
                    << "  gdv_int32 wb" << E << " = 0;    // tile-relative position of the window's first byte\n";
        cg.Stmt("const gdv_int32 ln" + E + "_u = " + total + ";");
        cg.Stmt("const gdv_int32 inc" + E + " = gdv_wave_scan_incl(ln" + E + "_u);");
        cg.Stmt("const gdv_int32 loc" + E + " = run" + E + " + inc" + E + " - ln" + E + "_u;  // where the row's bytes start inside the wave tile");
        cg.Stmt("const gdv_int32 sub0_" + E + " = run" + E + ";");
        cg.Stmt("{ const gdv_uint32 t = " + tile_total("ln" + E + "_u", "inc" + E) + ";");
        cg.Stmt("  run" + E + " = gdv_sat_add31(run" + E + ", (gdv_int32)(t > 0x7fffffffu ? 0x7fffffffu : t)); }");
        cg.Stmt("if (live) outo" + E + "[row] = (gdv_int32)(base" + E + " + loc" + E + ");");
        if (cg.selection())
          // the slot count may live in device memory (GDV_ROWS reads it): the host cannot know where the closing
          // offset belongs, so the wave tile that holds the last slot writes it
          after_rows << "  if (last_tile && lane == 0) outo" << E << "[n] = (gdv_int32)(base" << E << " + run" << E << ");\n";
        // nothing at or past the caller's capacity is written (the grand total says what was needed)
        cg.Stmt("const bool fit" + E + " = run" + E + " < 0x7fffffff && base" + E + " + run" + E + " <= A.out[" + E + "].cap;");
        if (has_window) {
          vo.window = num_staged++;
          vo.reads_views = !v.opaque;  // (concat results: their pieces are mostly views of columns)
          before_loop << "  gdv_uint8* const win" << E << " = lds_out + " << vo.window << " * (GDV_OUT_WIN + 16);\n";
          cg.Stmt("if (run" + E + " - wb" + E + " > GDV_OUT_WIN) {  // wave-uniform: the window is full");
          cg.Stmt("  if (fit" + E + " && sub0_" + E + " > wb" + E + ") gdv_flush_out(outd" + E + " + base" + E + " + wb" + E + ", win" + E + ", sub0_" + E +
                  " - wb" + E + ", lane);");
          cg.Stmt("  wb" + E + " = sub0_" + E + ";");
          cg.Stmt("}");
          cg.Stmt("if (run" + E + " - wb" + E + " <= GDV_OUT_WIN) {");
          cg.Stmt("  gdv_int32 at = loc" + E + " - wb" + E + ";");
          for (auto& name : pv) {
            cg.Stmt("  if (" + AblNot(4) + name + ".len > 0) GDV_STAGE_COPY((gdv_lds_u8*)(win" + E + " + at), " + name + ");");
            cg.Stmt("  at += " + name + ".len;");
          }
          cg.Stmt("} else if (fit" + E + ") {  // this sub-tile alone is wider than the window: row by row, in place");
        } else {
          cg.Stmt("if (fit" + E + ") {  // (no LDS window left for this output: row by row, in place)");
        }
        cg.Stmt("  gdv_uint8* at = outd" + E + " + base" + E + " + loc" + E + ";");
        for (auto& name : pv) {
          cg.Stmt("  if (" + name + ".len > 0) " + cg.CopyFn() + "(at, " + name + ");");
          cg.Stmt("  at += " + name + ".len;");
        }
        if (has_window) {
          cg.Stmt("  wb" + E + " = run" + E + ";  // nothing of it is staged");
          cg.Stmt("}");
          after_rows << "  if (run" << E << " > wb" << E << " && run" << E << " < 0x7fffffff && base" << E << " + run" << E << " <= A.out[" << E
                     << "].cap" << AblAnd(16) << ")\n"
                     << "    gdv_flush_out(outd" << E << " + base" << E << " + wb" << E << ", win" << E << ", run" << E << " - wb" << E << ", lane);\n";
        } else {
          cg.Stmt("}");
        }
        cg.varlen_outs_.push_back(vo);
      } else {
        emit_pieces();
        before_loop << "  gdv_int32 lc" << E << "[GDV_U] = {};  // where each row's bytes start inside the wave tile\n"
                    << "  gdv_int32 run" << E << " = 0;  // bytes this wave tile produces (saturates at 2^31-1)\n"
                    << "  bool dir" << E << " = false;  // second row pass: copy straight to HBM at dbase" << E << "\n"
                    << "  gdv_int64 dbase" << E << " = 0;\n";
        if (flat_cand) {
          vo.flat_slot = v.col_slot;
          vo.flat_map = v.col_map;
          const std::string K = std::to_string(v.col_slot);
          before_loop << "  gdv_uint64 fb" << E << " = 0;  // rows that drop bytes of the input span (nulls with a length)\n";
          // optimistic flat variant of the kernel (compile-time): the bytes are copied after the
          // sweep and the offsets are the input's, rebased: nothing of this output is scanned
          cg.Stmt("if (optflat) {");
          cg.Stmt("  if (pass == 0) {");
          cg.Stmt("    if (live) outo" + E + "[row] = oa" + K + "[u] - so0_" + K + ";");
          cg.Stmt("    fb" + E + " |= __ballot(!" + ok + " && ob" + K + "[u] > oa" + K + "[u]);");
          cg.Stmt("  }");
          cg.Stmt("} else {");
        }
        cg.Stmt("const gdv_int32 ln" + E + "_u = " + total + ";");
        cg.Stmt("if (pass == 0) {");
        cg.Stmt("  const gdv_int32 inc = gdv_wave_scan_incl(ln" + E + "_u);");
        cg.Stmt("  lc" + E + "[0] = run" + E + " + inc - ln" + E + "_u;");
        // 64 lengths below 2^25 cannot wrap the 32-bit scan; otherwise the total is taken on
        // 16-bit halves and saturates (the host rejects outputs of 2 GiB or more)
        cg.Stmt("  const gdv_uint32 t = __builtin_expect(__ballot(ln" + E + "_u >= (1 << 25)) != 0, 0) ? gdv_tile_total(ln" + E +
                "_u) : (gdv_uint32)gdv_wave_last(inc);");
        cg.Stmt("  run" + E + " = gdv_sat_add31(run" + E + ", (gdv_int32)(t > 0x7fffffffu ? 0x7fffffffu : t));");
        if (flat_cand) {
          const std::string K = std::to_string(v.col_slot);
          cg.Stmt("  fb" + E + " |= __ballot(!" + ok + " && ob" + K + "[u] > oa" + K + "[u]);");
        }
        if (has_window) {
          vo.window = num_staged++;
          before_loop << "  gdv_uint8* const win" << E << " = lds_out + " << vo.window << " * (GDV_OUT_WIN + 16);\n";
          // stage while the view is at hand (rows that fall outside the window are skipped: the
          // tile then takes the second, direct pass)
          cg.Stmt("  gdv_int32 at = lc" + E + "[0];");
          for (auto& name : pv) {
            cg.Stmt("  if (" + AblNot(4) + name + ".len > 0 && at + " + name + ".len <= GDV_OUT_WIN) GDV_STAGE_COPY((gdv_lds_u8*)(win" + E +
                    " + at), " + name + ");");
            cg.Stmt("  at += " + name + ".len;");
          }
        }
        cg.Stmt("} else if (dir" + E + ") {");
        cg.Stmt("  gdv_uint8* at = outd" + E + " + dbase" + E + " + lc" + E + "[0];");
        for (auto& name : pv) {
          cg.Stmt("  if (" + name + ".len > 0) " + cg.CopyFn() + "(at, " + name + ");");
          cg.Stmt("  at += " + name + ".len;");
        }
        cg.Stmt("}");
        if (flat_cand) cg.Stmt("}");
        cg.varlen_outs_.push_back(vo);
      }
    } else if (t.id == kBool) {
      std::string acc = accs.Get(cg, "__ballot(" + CodeGen::AndExpr("live", v.v) + ")");
      after_loop << WordStore(acc, "((gdv_uint64*)A.out[" + E + "].data)");
    } else {
      cg.Stmt("GDV_OUT(" + E + ", (" + t.CType() + ")" + v.v + ");");
    }
    if (prepass) continue;
    // validity word of the 64 rows of this sub-tile
    std::string word;
    if (cg.selection()) {
      word = "__ballot(" + CodeGen::AndExpr("live", cg.LaneValid(v)) + ")";
    } else {
      word = "(" + cg.WordExpr(v.vcols) + " & livemask)";
      if (!v.vlane.empty()) word = "(" + word + " & __ballot(live && " + v.vlane + "))";
    }
    after_loop << WordStore(accs.Get(cg, word), "A.out[" + E + "].valid");
  }
  // Loads in flight: aim for >= 8 KiB of input values per wave tile (64 lanes x GDV_U rows x
  // input bytes/row), within a budget of 512 input bytes per lane.  Wide plans (C2: 32 B/row,
  // ten outputs) stay at 4 — measured optimum, more sub-tiles cost occupancy — narrow plans
  // (C1: 12 B/row) go to 16 (+3 % measured).
  bool string_plan = plan->has_varlen_output || wave;
  for (size_t k = 0; k < cg.input_fields_.size(); k++)
    string_plan |= schema[cg.input_fields_[k]].type.is_varlen() && cg.needs_values_[k];
  if (string_plan) {
    // workgroup tile = 4 waves x 4 sub-tiles x 64 rows.  Sub-tiles cost registers, not code (the
    // row loop is rolled): 8 were better while the kernel carried 130 VGPRs either way; with the
    // branch-free range test and the compile-time flat variant 4 sub-tiles fit 95 VGPRs (5 waves
    // per SIMD) and win: 1.70 vs 1.83 ms (profiles/r02_c5_tuning.txt)
    if (!plan->opts.subtiles_forced) {
      if (shape == StringShape::kScanner) plan->opts.subtiles = 4;
      if (shape == StringShape::kWaveMain) {
        // wave shape: a tile costs a fixed prologue (scalar loads, sweep set-up, ends of the span,
        // flush), so 8 sub-tiles per wave beat 4 (C5: 1.15 vs 1.29 ms, profiles/r03_c5_tuning.txt)
        // — as long as the wave's LDS (staging windows of 8 B per row, the match bitmaps and the
        // mirror of ONE sub-tile's span) leaves room for six workgroups per CU
        const int windows = num_staged, hooks = static_cast<int>(cg.contains_hooks_.size());
        // LDS mirror (and with it the per-sub-tile sweep): the first swept var-len input, when some
        // staged output's copies would read it
        cg.mirror_slot_ = -1;
        bool readers = cg.replace_hook_ >= 0 && !cg.selection();  // (rows of a swept replace() are copied from the mirror)
        for (auto& vo : cg.varlen_outs_) readers |= vo.window >= 0 && vo.reads_views;
        for (size_t k = 0; opts.lds_mirror && readers && !cg.selection() && k < cg.input_fields_.size() && cg.mirror_slot_ < 0; k++) {
          if (!(schema[cg.input_fields_[k]].type.is_varlen() && cg.needs_values_[k])) continue;
          bool swept = cg.ascii_slots_.count(static_cast<int>(k)) != 0;
          for (auto& h : cg.contains_hooks_) swept |= h.slot == static_cast<int>(k);
          for (auto& vo : cg.varlen_outs_) swept |= vo.flat_slot == static_cast<int>(k);
          if (swept) cg.mirror_slot_ = static_cast<int>(k);
        }
        // (the mirror must hold the column whose matches the bitmap marks)
        if (opts.lds_mirror && cg.replace_hook_ >= 0) cg.mirror_slot_ = cg.contains_hooks_[cg.replace_hook_].slot;
        const int lds_u8 = windows * (8 * 64 * 8 + 16) +
                           (cg.mirror_slot_ >= 0 ? hooks * (2048 / 64 + 4) * 8 + 2048 + 32 : hooks * ((8 * 64 * 32) / 64 + 4) * 8);
        plan->opts.subtiles = lds_u8 <= 6656 ? 8 : 4;
      }
      // (kWavePrepass: the caller passes the main kernel's tile)
      if (shape == StringShape::kWavePrepass)  // a pre-pass sweeps only for a replace() that counts its matches in the bitmap
        cg.mirror_slot_ = cg.replace_hook_ >= 0 ? cg.contains_hooks_[cg.replace_hook_].slot : -1;
    }
    if (!plan->opts.waves_forced) plan->opts.waves = 4;
    if (varlen_outs != nullptr) *varlen_outs = cg.varlen_outs_;
    if (wave)
      return AssembleStringsWave(cg, plan, strings, accs, before_loop.str(), in_pass.str(), after_rows.str(),
                                 after_loop.str(), prepass ? WaveKind::kPrepass : WaveKind::kMain,
                                 /*has_direct_pass=*/false);
    return AssembleStrings(cg, plan, strings, accs, before_loop.str(), after_loop.str());
  }
  if (wave) return Status::CodeGenError("internal: wave shape asked for a plan without var-len columns");
  if (!plan->opts.subtiles_forced) {
    int in_bytes = 0;
    bool any_varlen = false;
    for (size_t k = 0; k < cg.input_fields_.size(); k++) {
      const DataType& t = schema[cg.input_fields_[k]].type;
      any_varlen |= t.is_varlen();
      if (cg.needs_values_[k]) in_bytes += std::max(1, t.byte_width());
    }
    if (!any_varlen && in_bytes > 0) {
      int u = 4;
      while (u < 16 && 64 * u * in_bytes < 8192 && 2 * u * in_bytes <= 512) u <<= 1;
      // Round 6: SIXTEEN sub-tiles per wave wherever the loaded values fit the registers (in_bytes x 16 <= 512: 128 VGPRs) and
      // no element is wider than 8 bytes.  A wave then reads and writes 64 x 16 consecutive elements of every stream — 4-8 KiB
      // per stream and wave instead of 1-2 — and the DRAM sees longer runs per stream between the 14 interleaved ones:
      // C2 4.75-4.82 ms against 4.96-5.10 (U = 4) on one box, 4.78-4.90 against 4.96-5.14 on another; C1 0.733-0.735 against
      // 0.776-0.780 (U = 4) and 0.81-0.85 (U = 8, what the rule above chose for it); decimal128 columns (C4): no difference,
      // they stay at 4 (profiles/r06_tile_shape.txt).  Occupancy drops to two or three waves per SIMD: it does not matter here.
      int max_width = 0;
      for (size_t k = 0; k < cg.input_fields_.size(); k++)
        if (cg.needs_values_[k]) max_width = std::max(max_width, schema[cg.input_fields_[k]].type.byte_width());
      for (auto& e : exprs) max_width = std::max(max_width, e->result().type.byte_width());
      if (in_bytes * 16 <= 512 && max_width <= 8) u = 16;
      plan->opts.subtiles = u;
      // ... and ONE workgroup per CU for such a plan when it reads at least twice what it writes (row mode): with sixteen
      // sub-tiles a wave has 16 x in_bytes x 64 bytes in flight, four waves keep a CU's share of the HBM busy, and every further
      // resident workgroup only interleaves more read streams at the DRAM — C1 0.705-0.711 ms against 0.743-0.757 at eight per
      // CU (and 0.745-0.754 at two) in three alternations on one box, 0.673-0.709 against 0.706-0.738 in four on another; write-dominated plans (C2) and 4-sub-tile plans (C4)
      // measure the same at 1 / 2 / 8 and keep the default (profiles/r06_grid_density.txt)
      int out_bytes = 0;
      for (auto& e : exprs) out_bytes += std::max(1, e->result().type.byte_width());
      if (u == 16 && mode == SelectionMode::kNone && in_bytes >= 2 * out_bytes) plan->grid_blocks_per_cu = 1;
    }
  }
  return Assemble(cg, plan, strings, accs, before_loop.str(), after_loop.str());
}

}  // namespace

Status PlanProjector(const Schema& schema, const std::vector<ExpressionPtr>& exprs,
                     SelectionMode mode, const CodegenOptions& opts, KernelPlan* plan, int compact_from) {
  AblationScope ablation_scope(opts.ablation);
  if (exprs.empty()) return Status::Invalid("Expressions cannot be empty");
  for (auto& e : exprs) {
    if (!e) return Status::Invalid("Expression cannot be null");
    GDV_RETURN_NOT_OK(ValidateExpression(schema, *e));
  }
  // Wave shape (pre-pass + scan + independent wave tiles): row mode and at least one var-len
  // output.  Outputs whose length follows from the offsets under the ASCII assumption (ByteFree)
  // cost a pre-pass over the offsets only; the others make the pre-pass read the bytes a first
  // time — still faster than the scanner shape, whose hand-off, occupancy and second row pass for
  // outputs above 8 bytes per row cost more (replace at 5 * 10^7 rows: 3.3 ms there).  Selection-
  // mode plans — and the re-run of a batch that breaks an assumption — take the scanner shape.
  // Round 5: selection-mode plans take the wave shape too (rows = slots, gathered through the selection vector;
  // no byte sweep, no optimistic assumption: the row functions run their general paths in the pre-pass and in the
  // main kernel alike) — rounds 2-4 sent them to the scanner shape.  GDV_NO_SEL_WAVE=1: as before.
  bool wave_ok = (mode == SelectionMode::kNone || !opts.no_sel_wave) && !opts.no_wave_shape;
  bool any_varlen_out = false;
  const bool bytefree_only = opts.wave_bytefree_only;
  for (auto& e : exprs) {
    if (!e->result().type.is_varlen()) continue;
    any_varlen_out = true;
    if (bytefree_only) wave_ok = wave_ok && ByteFree(*e->root(), opts.utf8_case);
  }
  if (!(wave_ok && any_varlen_out))
    return PlanProjectorShape(schema, exprs, mode, opts, StringShape::kScanner, nullptr, plan, nullptr, compact_from);

  KernelPlan fast, slow;
  std::vector<VarlenOut> vouts;
  GDV_RETURN_NOT_OK(PlanProjectorShape(schema, exprs, mode, opts, StringShape::kWaveMain, nullptr, &fast, &vouts, compact_from));
  GDV_RETURN_NOT_OK(PlanProjectorShape(schema, exprs, mode, opts, StringShape::kScanner, nullptr, &slow, nullptr, compact_from));
  // one argument block serves both kernels: the two generations must have bound the same inputs,
  // literals and constants (they run the same tree walk; checked, not assumed)
  if (!SameBindings(fast, slow)) {
    *plan = slow;
    return Status::OK();
  }
  std::vector<int> scanned;
  for (auto& vo : vouts)
    if (vo.flat_slot < 0) scanned.push_back(vo.e);
  if (static_cast<int>(scanned.size()) > kMaxWaveSegments) {
    *plan = slow;
    return Status::OK();
  }
  *plan = fast;
  plan->can_raise = fast.can_raise || slow.can_raise;
  // the fallback: the scanner-shaped kernel with every output on the general path
  plan->kernel_name_general = slow.has_flat_output ? slow.kernel_name_general : slow.kernel_name;
  plan->source_general = slow.has_flat_output ? slow.source_general : slow.source;
  plan->general_subtiles = slow.opts.subtiles;
  plan->general_waves = slow.opts.waves;
  plan->wave_segments.clear();
  for (auto& vo : vouts) plan->wave_segments.push_back(vo.flat_slot < 0 ? vo.segment : -1);
  if (!scanned.empty()) {
    auto pre = std::make_shared<KernelPlan>();
    CodegenOptions popts = fast.opts;  // same tile: a wave tile of the pre-pass IS a wave tile of the main kernel
    GDV_RETURN_NOT_OK(PlanProjectorShape(schema, exprs, mode, popts, StringShape::kWavePrepass, &scanned, pre.get(), nullptr, compact_from));
    if (pre->opts.subtiles != fast.opts.subtiles) {
      *plan = slow;
      return Status::OK();
    }
    plan->prepass = pre;
    plan->ir = fast.source + pre->source;  // (the main kernel first: its name is the plan's)
  }
  // The exact variant (round 4): only where some function consults the ASCII flag — i.e. where the
  // optimistic kernels can raise NOTASCII at all.  Same tree walk, same inputs / literals / constants
  // (checked): the host hands it the optimistic kernels' argument blocks.
  // (selection-mode plans: a batch that breaks the assumption takes the scanner-shaped general kernel)
  if (mode == SelectionMode::kNone && fast.source.find("GDV_ERR_NOTASCII") != std::string::npos) {
    auto ex = std::make_shared<KernelPlan>();
    std::vector<VarlenOut> evouts;
    Status st = PlanProjectorShape(schema, exprs, mode, fast.opts, StringShape::kWaveMainExact, nullptr, ex.get(), &evouts, compact_from);
    bool ok = st.ok() && ex->opts.subtiles == fast.opts.subtiles && ex->opts.waves == fast.opts.waves &&
              SameBindings(*ex, fast) && evouts.size() == vouts.size();
    for (size_t i = 0; ok && i < vouts.size(); i++)
      ok = evouts[i].flat_slot == vouts[i].flat_slot && evouts[i].segment == vouts[i].segment;
    if (ok && plan->prepass) {
      auto epre = std::make_shared<KernelPlan>();
      st = PlanProjectorShape(schema, exprs, mode, fast.opts, StringShape::kWavePrepassExact, &scanned, epre.get(), nullptr, compact_from);
      const KernelPlan& p0 = *plan->prepass;
      ok = st.ok() && epre->opts.subtiles == fast.opts.subtiles && SameBindings(*epre, p0) && epre->layout.total() == p0.layout.total();
      ex->prepass = epre;
    }
    if (ok) {
      plan->exact = ex;
      plan->can_raise = plan->can_raise || ex->can_raise;
    }
  }
  return Status::OK();
}

Status PlanFilter(const Schema& schema, const ExpressionPtr& condition,
                  const CodegenOptions& opts, KernelPlan* plan) {
  AblationScope ablation_scope(opts.ablation);
  if (!condition) return Status::Invalid("Condition cannot be null");
  GDV_RETURN_NOT_OK(ValidateExpression(schema, *condition));
  if (condition->root()->return_type().id != kBool)
    return Status::ValidationError("Filter condition must be of type boolean");
  plan->kind = KernelKind::kFilter;
  plan->mode = SelectionMode::kNone;
  plan->opts = opts;
  CodeGen cg(schema, SelectionMode::kNone, opts);
  WordAccumulators accs;
  Val v;
  cg.Stmt("// @expr_0 (filter condition)");
  GDV_RETURN_NOT_OK(cg.Gen(*condition->root(), "", &v));
  // a null predicate does not select the row
  std::string pass = CodeGen::AndExpr(cg.LaneValid(v), v.v);
  cg.Stmt("const gdv_uint64 fm = __ballot(" + CodeGen::AndExpr("live", pass) + ");");
  cg.Stmt("fcount += (gdv_uint32)__popcll(fm);");
  std::string acc = accs.Get(cg, "fm");
  // A predicate kernel keeps nothing but its input values live, so it can afford many more
  // loads in flight per wave than a projection: measured on C3 (2 x int64, 10^9 rows) the
  // predicate pass goes from 5.2 TB/s at GDV_U = 4 to 5.9 TB/s at 16 (profiles/r01_c3_sweep).
  // Budget: <= 512 bytes of input values per lane, i.e. <= 128 VGPRs of loads.
  if (!plan->opts.subtiles_forced) {
    int in_bytes = 0;
    for (size_t k = 0; k < cg.input_fields_.size(); k++)
      if (cg.needs_values_[k]) in_bytes += std::max(4, schema[cg.input_fields_[k]].type.byte_width());
    int u = 16;
    while (u > 4 && u * std::max(in_bytes, 1) > 512) u >>= 1;
    plan->opts.subtiles = u;
    // (Round 6: ONE workgroup per CU — what the read skeleton prefers — measured 2.64-2.70 ms per Filter::Evaluate against
    // 2.69-2.80 at eight per CU in five alternations on one box and 2.97-2.98 against 2.92-2.94 in four on another: the grid
    // stays at the engine's default, profiles/r06_grid_density.txt)
  }
  std::ostringstream after;
  // the match words are written once and read by the index-emission kernel much later: non-temporal
  // (C3, same box: 2.74 / 2.99 ms plain vs 2.69 / 2.67 ms; validity words of projections measured
  // the other way round — C2 4.90 vs 5.0-5.1 ms — and stay plain)
  after << WordStore(acc, "A.mask", true);
  // one selected-row count per wave tile feeds the offsets scan (gdv_kernels.hip)
  after << "  if (lane == 0) A.counts[wbase / GDV_U] = fcount;\n";
  bool string_plan = false;
  for (size_t k = 0; k < cg.input_fields_.size(); k++)
    string_plan |= schema[cg.input_fields_[k]].type.is_varlen() && cg.needs_values_[k];
  if (string_plan) {
    // the index-emission kernel walks groups of 64 match words: sub-tiles stay a power of two
    plan->opts.subtiles = 4;
    if (!plan->opts.waves_forced) plan->opts.waves = 4;
    return AssembleStrings(cg, plan, {condition->ToString()}, accs, "  gdv_uint32 fcount = 0;\n", after.str());
  }
  return Assemble(cg, plan, {condition->ToString()}, accs, "  gdv_uint32 fcount = 0;\n",
                  after.str());
}

Status PlanFilterProject(const Schema& schema, const ExpressionPtr& condition, const std::vector<ExpressionPtr>& exprs,
                         SelectionMode index_mode, const CodegenOptions& opts, KernelPlan* plan, bool with_small) {
  if (!condition) return Status::Invalid("Condition cannot be null");
  if (exprs.empty()) return Status::Invalid("Expressions cannot be empty");
  GDV_RETURN_NOT_OK(ValidateExpression(schema, *condition));
  if (condition->root()->return_type().id != kBool)
    return Status::ValidationError("Filter condition must be of type boolean");
  for (auto& e : exprs) {
    if (!e) return Status::Invalid("Expression cannot be null");
    GDV_RETURN_NOT_OK(ValidateExpression(schema, *e));
    if (e->result().type.is_varlen())
      return Status::CodeGenError("fused filter-project: var-len outputs take the filter + projector chain");
  }
  // the direct shape always exists; the windowed one is the main kernel wherever its window fits
  auto direct = std::make_shared<KernelPlan>();
  GDV_RETURN_NOT_OK(PlanFilterProjectShape(schema, condition, exprs, index_mode, opts, FpShape::kDirect, direct.get()));
  if (opts.fp_window_bytes > 0) {
    KernelPlan windowed;
    Status st = PlanFilterProjectShape(schema, condition, exprs, index_mode, opts, FpShape::kWindow, &windowed);
    // the engine launches either kernel with the windowed plan's argument block: the direct plan's literals and
    // constant block must be a prefix of it (they are: the windowed body generates the same trees first, then the
    // tail's copies) — if that ever stops holding, the plan keeps the direct shape alone
    const bool prefix = st.ok() && direct->literals.size() <= windowed.literals.size() &&
                        std::equal(direct->literals.begin(), direct->literals.end(), windowed.literals.begin()) &&
                        windowed.const_block.compare(0, direct->const_block.size(), direct->const_block) == 0 &&
                        direct->input_fields == windowed.input_fields && direct->opts.subtiles == windowed.opts.subtiles &&
                        direct->opts.waves == windowed.opts.waves;
    if (st.ok() && prefix) {
      *plan = std::move(windowed);
      plan->exact = direct;
      // the small shape (one workgroup per batch) is the windowed body again: the same rule, with equality — text
      // only here, compiled when a list of small batches first asks for it
      if (with_small) {
        auto small = std::make_shared<KernelPlan>();
        st = PlanFilterProjectShape(schema, condition, exprs, index_mode, opts, FpShape::kSmall, small.get());
        if (!st.ok() && st.code != kCodeGenError) return st;
        if (st.ok() && small->literals == plan->literals && small->const_block == plan->const_block &&
            small->input_fields == plan->input_fields && small->opts.subtiles == plan->opts.subtiles &&
            small->opts.waves == plan->opts.waves && small->layout.total() == plan->layout.total() &&
            small->fp_rounds == plan->fp_rounds && small->fp_window_rows == plan->fp_window_rows)
          plan->small = small;
      }
      return Status::OK();
    }
    if (!st.ok() && st.code != kCodeGenError) return st;
  }
  *plan = std::move(*direct);
  return Status::OK();
}

}  // namespace gdv
