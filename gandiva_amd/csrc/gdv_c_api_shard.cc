// C ABI, device selection and the one-call sharded paths: one host thread per shard, each on its own device context and stream.
#include "gdv_c_api_internal.h"

#include <thread>

using namespace gdv;
using namespace gdv::capi;

namespace {
void ShardBounds(int64_t num_rows, int num_shards, int shard, int64_t* lo, int64_t* hi) {
  (void)gdv_shard_bounds(num_rows, num_shards, shard, lo, hi);
}
// body(shard, stream) runs on device devices[shard]; returns the first failing shard's status
template <typename Fn>
int RunShards(int n, const int32_t* devices, Fn&& body) {
  DeviceScope scope;  // (shard 0 selects its device on the calling thread)
  std::vector<Status> st(static_cast<size_t>(n));
  auto work = [&](int s) {
    try {
      Status sel = Runtime::SelectDevice(devices[s]);
      if (!sel.ok()) { st[s] = sel; return; }
      Runtime& rt = Runtime::Get();
      Status dev = rt.EnsureDevice();
      if (!dev.ok()) { st[s] = dev; return; }
      hipStream_t stream = nullptr;
      Status a = rt.AcquireStream(&stream);
      if (!a.ok()) { st[s] = a; return; }
      st[s] = body(s, stream);
      (void)hipStreamSynchronize(stream);
      rt.ReleaseStream(stream);
    } catch (const std::bad_alloc&) {
      st[s] = Status::OutOfMemory("host allocation failed");
    } catch (const std::exception& e) {
      st[s] = Status::ExecutionError(std::string("internal error: ") + e.what());
    }
  };
  std::vector<std::thread> threads;
  threads.reserve(n > 1 ? n - 1 : 0);
  int started = 1;  // (shard 0 runs on the calling thread)
  try {
    for (int s = 1; s < n; s++, started++) threads.emplace_back(work, s);
  } catch (const std::exception&) {
    // the process is out of threads: the shards that got none run here, one after the other (a joinable std::thread
    // must never be destroyed — the ones that did start are joined below whatever happens)
  }
  work(0);
  for (int s = started; s < n; s++) work(s);
  for (auto& t : threads) t.join();
  for (int s = 0; s < n; s++)
    if (!st[s].ok())
      return Fail(Status(st[s].code, "shard " + std::to_string(s) + " (device " + std::to_string(devices[s]) + "): " + st[s].msg));
  return GDV_OK;
}
}  // namespace

extern "C" {

// ---------------------------------------------------------------- device helpers
int gdv_device_count(void) { return Runtime::DeviceCount(); }
int gdv_physical_device_count(void) { return Runtime::PhysicalDeviceCount(); }
int gdv_set_virtual_devices(int n) {
  if (n < 0 || n > Runtime::kMaxDevices) return Fail(Status::Invalid("bad virtual device count"));
  Runtime::SetVirtualDevices(n);
  return GDV_OK;
}
int gdv_set_device(int device) { return Check(Runtime::SelectDevice(device)); }
int gdv_get_device(void) { return Runtime::SelectedDevice(); }
int gdv_shard_bounds(int64_t num_rows, int num_shards, int shard, int64_t* lo, int64_t* hi) {
  if (num_rows < 0 || num_shards < 1 || shard < 0 || shard >= num_shards || !lo || !hi)
    return Fail(Status::Invalid("bad shard arguments"));
  // near-equal shards on 1024-row boundaries (one workgroup tile = one 128-byte line of every
  // validity bitmap); the last shard takes the ragged tail — gandiva_amd/shard.py: shard_bounds
  const int64_t align = 1024;
  const int64_t tiles = (num_rows + align - 1) / align;
  const int64_t per = tiles / num_shards, extra = tiles % num_shards;
  const int64_t lo_tile = shard * per + std::min<int64_t>(shard, extra);
  const int64_t hi_tile = lo_tile + per + (shard < extra ? 1 : 0);
  *lo = std::min(lo_tile * align, num_rows);
  *hi = std::min(hi_tile * align, num_rows);
  return GDV_OK;
}


int gdv_projector_evaluate_sharded(const gdv_projector_t* p, int64_t num_rows, int num_cols, int num_outs,
                                   gdv_shard_t* shards, int num_shards, uint32_t flags) {
  return Guarded([&]() -> int {
  (void)flags;
  if (!p) return Fail(Status::Invalid("null projector"));
  if (num_shards < 1 || !shards || num_rows < 0) return Fail(Status::Invalid("bad shard list"));
  if (p->p->plan().mode != SelectionMode::kNone) return Fail(Status::Invalid("sharded evaluation takes row-mode projectors"));
  std::vector<int32_t> devices(num_shards);
  for (int s = 0; s < num_shards; s++) {
    devices[s] = shards[s].device;
    if ((num_cols > 0 && !shards[s].cols) || !shards[s].outs) return Fail(Status::Invalid("shard without columns / outputs"));
  }
  return RunShards(num_shards, devices.data(), [&](int s, hipStream_t stream) -> Status {
    int64_t lo = 0, hi = 0;
    ShardBounds(num_rows, num_shards, s, &lo, &hi);
    if (hi == lo) return Status::OK();
    std::vector<ColumnBuffers> c = ToColumns(shards[s].cols, num_cols);
    std::vector<OutputBuffers> o = ToOutputs(shards[s].outs, num_outs);
    Status st = p->p->Evaluate(hi - lo, c.data(), num_cols, nullptr, o.data(), num_outs, MemKind::kDevice, stream, 0);
    WriteBackDataSizes(shards[s].outs, o, num_outs);
    return st;
  });
  });
}

int gdv_filter_evaluate_sharded(const gdv_filter_t* f, int64_t num_rows, int num_cols, int selection_mode,
                                gdv_shard_t* shards, int num_shards, uint32_t flags, int64_t* total_selected) {
  return Guarded([&]() -> int {
  if (!f) return Fail(Status::Invalid("null filter"));
  if (num_shards < 1 || !shards || num_rows < 0) return Fail(Status::Invalid("bad shard list"));
  SelectionMode mode;
  if (!ToSelectionMode(selection_mode, &mode) || mode == SelectionMode::kNone) return Fail(Status::Invalid("bad selection mode"));
  std::vector<int32_t> devices(num_shards);
  for (int s = 0; s < num_shards; s++) {
    devices[s] = shards[s].device;
    shards[s].num_selected = 0;
    if ((num_cols > 0 && !shards[s].cols) || !shards[s].out_indices) return Fail(Status::Invalid("shard without columns / indices"));
  }
  const bool global = (flags & GDV_SHARD_GLOBAL_INDICES) != 0;
  int rc = RunShards(num_shards, devices.data(), [&](int s, hipStream_t stream) -> Status {
    int64_t lo = 0, hi = 0;
    ShardBounds(num_rows, num_shards, s, &lo, &hi);
    if (hi == lo) return Status::OK();
    std::vector<ColumnBuffers> c = ToColumns(shards[s].cols, num_cols);
    return f->f->Evaluate(hi - lo, c.data(), num_cols, mode, shards[s].out_indices, shards[s].max_slots,
                          &shards[s].num_selected, MemKind::kDevice, stream, 0, nullptr, global ? lo : 0);
  });
  if (rc != GDV_OK) return rc;
  if (total_selected) {
    *total_selected = 0;
    for (int s = 0; s < num_shards; s++) *total_selected += shards[s].num_selected;
  }
  return GDV_OK;
  });
}

int gdv_filter_gather_sharded(const gdv_shard_t* shards, int num_shards, int selection_mode, int dst_device,
                              void* dst_indices, int64_t dst_slots) {
  return Guarded([&]() -> int {
  SelectionMode mode;
  if (!ToSelectionMode(selection_mode, &mode) || mode == SelectionMode::kNone) return Fail(Status::Invalid("bad selection mode"));
  if (num_shards < 1 || !shards || !dst_indices) return Fail(Status::Invalid("bad shard list"));
  const int w = IndexWidth(mode);
  int64_t total = 0;
  for (int s = 0; s < num_shards; s++) total += shards[s].num_selected;
  if (total > dst_slots) return Fail(Status::Invalid("gathered selection vector needs " + std::to_string(total) + " slots"));
  DeviceScope scope;
  Status st = scope.Select(dst_device);
  if (!st.ok()) return Fail(st);
  Runtime& dst = Runtime::Get();
  st = dst.EnsureDevice();
  hipStream_t stream = nullptr;
  if (st.ok()) st = dst.AcquireStream(&stream);
  if (st.ok()) {
    int64_t at = 0;
    for (int s = 0; s < num_shards && st.ok(); s++) {
      const int64_t n = shards[s].num_selected;
      if (n > 0) {
        // (virtual devices share a physical one: the copy is then an ordinary device-to-device one)
        const int src_phys = Runtime::ForDevice(shards[s].device).physical();
        hipError_t e = src_phys == dst.physical()
                           ? hipMemcpyAsync(static_cast<char*>(dst_indices) + at * w, shards[s].out_indices, n * w, hipMemcpyDeviceToDevice, stream)
                           : hipMemcpyPeerAsync(static_cast<char*>(dst_indices) + at * w, dst.physical(), shards[s].out_indices, src_phys, n * w, stream);
        if (e != hipSuccess) st = Status::ExecutionError(std::string("gather: ") + hipGetErrorString(e));
      }
      at += n;
    }
    if (hipStreamSynchronize(stream) != hipSuccess && st.ok()) st = Status::ExecutionError("gather: stream synchronisation failed");
    dst.ReleaseStream(stream);
  }
  return Check(st);
  });
}

int gdv_projector_evaluate_host_sharded(const gdv_projector_t* p, int64_t num_rows, const gdv_column_t* cols, int num_cols,
                                        gdv_out_column_t* outs, int num_outs, const int32_t* devices, int num_devices) {
  return Guarded([&]() -> int {
  if (!p) return Fail(Status::Invalid("null projector"));
  if (num_cols > 0 && !cols) return Fail(Status::Invalid("null column array"));
  if (!outs || !devices || num_devices < 1) return Fail(Status::Invalid("outputs and a device list are required"));
  if (p->p->plan().mode != SelectionMode::kNone) return Fail(Status::Invalid("sharded evaluation takes row-mode projectors"));
  if (num_outs != p->p->num_outputs()) return Fail(Status::Invalid("number of outputs does not match the projector"));
  bool varlen_out = false;
  for (int i = 0; i < num_outs; i++) varlen_out |= p->p->output_type(i).is_varlen();
  // var-len outputs: byte positions depend on the shards before -> one device; tiny batches: not worth the threads
  const int n = (varlen_out || num_rows < 2048) ? 1 : num_devices;
  if (n == 1) {
    DeviceScope scope;
    Status sel = scope.Select(devices[0]);
    if (!sel.ok()) return Fail(sel);
    return ProjectorEvaluate(p, num_rows, cols, num_cols, nullptr, nullptr, outs, num_outs, GDV_MEM_HOST, nullptr, 0);
  }
  for (int i = 0; i < num_outs; i++) {
    const DataType& t = p->p->output_type(i);
    const int64_t vneed = (num_rows + 7) / 8, dneed = t.id == kBool ? (num_rows + 7) / 8 : Projector::DataBytes(t, num_rows);
    if (!outs[i].validity || !outs[i].data || outs[i].validity_size < vneed || outs[i].data_size < dneed)
      return Fail(Status::Invalid("output buffer " + std::to_string(i) + " too small"));
  }
  return RunShards(n, devices, [&](int s, hipStream_t stream) -> Status {
    int64_t lo = 0, hi = 0;
    ShardBounds(num_rows, n, s, &lo, &hi);
    if (hi == lo) return Status::OK();
    // a slice of the caller's batch: array offset + lo (var-len columns keep their whole byte buffer)
    std::vector<ColumnBuffers> c = ToColumns(cols, num_cols);
    for (auto& col : c) col.offset += lo;
    std::vector<OutputBuffers> o(num_outs);
    for (int i = 0; i < num_outs; i++) {
      const DataType& t = p->p->output_type(i);
      // lo is a multiple of 1024: whole bytes of every bitmap
      o[i].validity = static_cast<char*>(outs[i].validity) + lo / 8;
      o[i].validity_size = (hi - lo + 7) / 8;
      if (t.id == kBool) {
        o[i].data = static_cast<char*>(outs[i].data) + lo / 8;
        o[i].data_size = (hi - lo + 7) / 8;
      } else {
        o[i].data = static_cast<char*>(outs[i].data) + lo * t.byte_width();
        o[i].data_size = (hi - lo) * t.byte_width();
      }
    }
    return p->p->Evaluate(hi - lo, c.data(), num_cols, nullptr, o.data(), num_outs, MemKind::kHost, stream, 0);
  });
  });
}

int gdv_filter_evaluate_host_sharded(const gdv_filter_t* f, int64_t num_rows, const gdv_column_t* cols, int num_cols,
                                     int selection_mode, void* out_indices, int64_t max_slots, int64_t* num_selected,
                                     const int32_t* devices, int num_devices) {
  return Guarded([&]() -> int {
  if (!f) return Fail(Status::Invalid("null filter"));
  if (num_cols > 0 && !cols) return Fail(Status::Invalid("null column array"));
  if (!out_indices || !num_selected || !devices || num_devices < 1) return Fail(Status::Invalid("Selection vector cannot be null"));
  SelectionMode mode;
  if (!ToSelectionMode(selection_mode, &mode) || mode == SelectionMode::kNone) return Fail(Status::Invalid("bad selection mode"));
  if (max_slots < num_rows)
    return Fail(Status::Invalid("Selection vector too small: max slots " + std::to_string(max_slots) + " < rows " + std::to_string(num_rows)));
  const int n = num_rows < 2048 ? 1 : num_devices;
  const int w = IndexWidth(mode);
  std::vector<int64_t> counts(n, 0);
  int rc = RunShards(n, devices, [&](int s, hipStream_t stream) -> Status {
    int64_t lo = 0, hi = 0;
    ShardBounds(num_rows, n, s, &lo, &hi);
    if (hi == lo) return Status::OK();
    std::vector<ColumnBuffers> c = ToColumns(cols, num_cols);
    for (auto& col : c) col.offset += lo;
    // shard s can select at most hi - lo rows: its part of the vector is [lo, hi), closed up below
    return f->f->Evaluate(hi - lo, c.data(), num_cols, mode, static_cast<char*>(out_indices) + lo * w, hi - lo, &counts[s],
                          MemKind::kHost, stream, 0, nullptr, lo);
  });
  if (rc != GDV_OK) return rc;
  int64_t at = 0;
  for (int s = 0; s < n; s++) {
    int64_t lo = 0, hi = 0;
    ShardBounds(num_rows, n, s, &lo, &hi);
    if (counts[s] > 0 && at != lo)
      std::memmove(static_cast<char*>(out_indices) + at * w, static_cast<char*>(out_indices) + lo * w, static_cast<size_t>(counts[s]) * w);
    at += counts[s];
  }
  *num_selected = at;
  return GDV_OK;
  });
}

}  // extern "C"
