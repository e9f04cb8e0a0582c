// gandiva/device_memory.h — NOT part of the reference's API (its buffers are the CPU's own): an addition of this
// backend, like host_memory.h and sharded.h.  An arrow::Device / arrow::MemoryManager pair over the HBM of one GPU, so
// that a C++ (or pyarrow) caller can hold a RecordBatch whose buffers are device-resident and hand it to
// Projector::Evaluate / Filter::Evaluate / FilterProject::Evaluate / the shard overloads of sharded.h: such a batch is
// evaluated in place, its outputs are allocated from the same manager, nothing crosses the host link.
//
//     auto mm = gandiva::HipDevice::Make(0).ValueOrDie()->hip_memory_manager();
//     auto dbatch = gandiva::CopyBatchTo(*batch, mm).ValueOrDie();          // host -> HBM, once
//     projector->Evaluate(*dbatch, nullptr, &out);                          // out[i]->data()->buffers: !is_cpu()
//     auto host = out[0]->CopyTo(arrow::default_cpu_memory_manager());      // only when the host wants to look
//
// Memory comes from the library's device pool (include/gandiva_amd.h: gdv_device_pool_*): a buffer that is dropped goes
// back to the pool and is handed out again for the next request of its size, and ReserveSet gives the placement-probed
// set of output columns for Projector::Evaluate(batch, ArrayDataVector).
#pragma once
#include <cstdint>
#include <memory>
#include <string>
#include <vector>

#include "arrow/buffer.h"
#include "arrow/device.h"
#include "arrow/record_batch.h"
#include "gandiva/arrow.h"
#include "gandiva/selection_vector.h"

namespace gandiva {

class HipMemoryManager;

// One object per library device number (gdv_set_device's numbering: virtual devices count).  Make() touches no GPU; the
// objects live as long as the process.
class HipDevice : public arrow::Device {
 public:
  static arrow::Result<std::shared_ptr<HipDevice>> Make(int device_id);
  const char* type_name() const override { return "gandiva::HipDevice"; }
  std::string ToString() const override;
  bool Equals(const arrow::Device& other) const override;
  int64_t device_id() const override { return id_; }
  arrow::DeviceAllocationType device_type() const override { return arrow::DeviceAllocationType::kROCM; }
  // the same manager on every call
  std::shared_ptr<arrow::MemoryManager> default_memory_manager() override;
  std::shared_ptr<HipMemoryManager> hip_memory_manager();

 private:
  explicit HipDevice(int id) : arrow::Device(/*is_cpu=*/false), id_(id) {}
  int id_;
  std::shared_ptr<HipMemoryManager> mm_;
};

// Owns one device pool, created on its device with the first allocation.  Every entry point selects the manager's
// device for the duration of the call and restores the calling thread's device afterwards.  Thread-safe.
class HipMemoryManager : public arrow::MemoryManager {
 public:
  // A mutable, non-CPU buffer of `size` bytes; capacity() is `size` rounded up to a multiple of 64 bytes (the kernels
  // store validity in whole 8-byte words).  The buffer keeps the manager alive and goes back to the pool when dropped.
  arrow::Result<std::unique_ptr<arrow::Buffer>> AllocateBuffer(int64_t size) override;
  arrow::Result<std::shared_ptr<arrow::io::RandomAccessFile>> GetBufferReader(std::shared_ptr<arrow::Buffer> buf) override;
  arrow::Result<std::shared_ptr<arrow::io::OutputStream>> GetBufferWriter(std::shared_ptr<arrow::Buffer> buf) override;

  // `count` buffers of `bytes` each, placed by gdv_device_pool_reserve_set: the output columns of a projection, to be
  // reused across batches through Projector::Evaluate(batch, ArrayDataVector).
  arrow::Result<std::vector<std::shared_ptr<arrow::Buffer>>> ReserveSet(int count, int64_t bytes, int candidates = 4);
  // buffers that were dropped go back to the driver
  Status Trim();
  // bytes the pool holds (handed out + retained); *in_use: the handed-out part
  int64_t bytes_allocated(int64_t* in_use = nullptr) const;
  int device_id() const { return id_; }

 protected:
  // CPU <-> this device over gdv_memcpy_h2d / gdv_memcpy_d2h.  The C ABI has no device-to-device copy: between two
  // HipMemoryManagers these return nullptr ("not supported") and Arrow's own MemoryManager::CopyBuffer goes through
  // the host.
  arrow::Result<std::shared_ptr<arrow::Buffer>> CopyBufferFrom(const std::shared_ptr<arrow::Buffer>& buf,
                                                               const std::shared_ptr<arrow::MemoryManager>& from) override;
  arrow::Result<std::shared_ptr<arrow::Buffer>> CopyBufferTo(const std::shared_ptr<arrow::Buffer>& buf,
                                                             const std::shared_ptr<arrow::MemoryManager>& to) override;
  arrow::Result<std::unique_ptr<arrow::Buffer>> CopyNonOwnedFrom(const arrow::Buffer& buf,
                                                                 const std::shared_ptr<arrow::MemoryManager>& from) override;
  arrow::Result<std::unique_ptr<arrow::Buffer>> CopyNonOwnedTo(const arrow::Buffer& buf,
                                                               const std::shared_ptr<arrow::MemoryManager>& to) override;

 private:
  friend class HipDevice;
  struct Impl;
  HipMemoryManager(const std::shared_ptr<arrow::Device>& device, int id);
  int id_;
  Impl* impl_;  // never deleted: the managers live as long as the process and make no HIP call at exit
};

// RecordBatch::CopyTo under a name that says what it does: every buffer of `batch` copied into `to`'s memory
// (a HipMemoryManager: host -> HBM; arrow::default_cpu_memory_manager(): HBM -> host).
arrow::Result<std::shared_ptr<arrow::RecordBatch>> CopyBatchTo(const arrow::RecordBatch& batch,
                                                               const std::shared_ptr<arrow::MemoryManager>& to);

// A SelectionVector over `max_slots` indices in `mm`'s memory, for Filter::Evaluate / FilterProject::Evaluate over
// batches that live there.
arrow::Result<std::shared_ptr<SelectionVector>> MakeDeviceSelectionVector(SelectionVector::Mode mode, int64_t max_slots,
                                                                          const std::shared_ptr<HipMemoryManager>& mm);

}  // namespace gandiva
