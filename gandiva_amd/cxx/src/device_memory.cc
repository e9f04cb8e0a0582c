// gandiva/device_memory.h over the C ABI's device pool (gdv_device_pool_*), gdv_memcpy_h2d / _d2h and
// gdv_set_device / gdv_get_device.  Host logic only: no kernel is launched from here.
#include "gandiva/device_memory.h"

#include <mutex>

#include "arrow/api.h"
#include "device_scope.h"
#include "gandiva_amd.h"

namespace gandiva {

namespace {

Status LastError(int rc) {
  std::string msg = gdv_last_error();
  size_t colon = msg.find(": ");
  if (colon != std::string::npos) msg = msg.substr(colon + 2);
  return Status(static_cast<arrow::StatusCode>(rc), msg);
}
#define GDV_DEV_RETURN_NOT_OK(rc)             \
  do {                                        \
    int _rc = (rc);                           \
    if (_rc != GDV_OK) return LastError(_rc); \
  } while (0)

constexpr int kMaxDevices = 64;
constexpr int64_t kAlign = 64;
alignas(64) const uint8_t kZeros[kAlign] = {};

int64_t RoundUp(int64_t size) { return std::max<int64_t>((size + kAlign - 1) / kAlign * kAlign, kAlign); }

}  // namespace

struct HipMemoryManager::Impl {
  std::mutex mu;
  gdv_device_pool_t* pool = nullptr;  // created with the manager's device selected (a pool belongs to that device)
  // called under a DeviceScope of the manager's device
  Status Pool(gdv_device_pool_t** out) {
    std::lock_guard<std::mutex> g(mu);
    if (pool == nullptr) GDV_DEV_RETURN_NOT_OK(gdv_device_pool_create(&pool));
    *out = pool;
    return Status::OK();
  }
};

namespace {

// The block goes back to the pool with the buffer; the manager (and so the pool) outlives it.
class HipBuffer : public arrow::MutableBuffer {
 public:
  HipBuffer(void* ptr, int64_t size, int64_t capacity, std::shared_ptr<arrow::MemoryManager> mm, gdv_device_pool_t* pool)
      : arrow::MutableBuffer(static_cast<uint8_t*>(ptr), size, std::move(mm)), pool_(pool) {
    capacity_ = capacity;
  }
  ~HipBuffer() override { (void)gdv_device_pool_free(pool_, const_cast<uint8_t*>(data_)); }  // (host bookkeeping only)

 private:
  gdv_device_pool_t* pool_;
};

}  // namespace

// ------------------------------------------------------------------ HipDevice

arrow::Result<std::shared_ptr<HipDevice>> HipDevice::Make(int device_id) {
  if (device_id < 0 || device_id >= kMaxDevices)
    return Status::Invalid("device ", device_id, " out of range (0 .. ", kMaxDevices - 1, ")");
  // never destroyed: buffers anywhere in the process may still point at a manager when static destructors run,
  // and the HIP runtime must not be called from them
  static std::mutex* mu = new std::mutex;
  static std::vector<std::shared_ptr<HipDevice>>* devices = new std::vector<std::shared_ptr<HipDevice>>(kMaxDevices);
  std::lock_guard<std::mutex> g(*mu);
  auto& slot = (*devices)[device_id];
  if (!slot) {
    slot = std::shared_ptr<HipDevice>(new HipDevice(device_id));
    slot->mm_ = std::shared_ptr<HipMemoryManager>(new HipMemoryManager(slot, device_id));
  }
  return slot;
}

std::string HipDevice::ToString() const { return "HipDevice(device_number=" + std::to_string(id_) + ")"; }

bool HipDevice::Equals(const arrow::Device& other) const {
  auto o = dynamic_cast<const HipDevice*>(&other);
  return o != nullptr && o->id_ == id_;
}

std::shared_ptr<arrow::MemoryManager> HipDevice::default_memory_manager() { return mm_; }
std::shared_ptr<HipMemoryManager> HipDevice::hip_memory_manager() { return mm_; }

// ------------------------------------------------------------------ HipMemoryManager

HipMemoryManager::HipMemoryManager(const std::shared_ptr<arrow::Device>& device, int id)
    : arrow::MemoryManager(device), id_(id), impl_(new Impl) {}

arrow::Result<std::unique_ptr<arrow::Buffer>> HipMemoryManager::AllocateBuffer(int64_t size) {
  if (size < 0) return Status::Invalid("negative allocation size");
  internal::DeviceScope scope(id_);
  ARROW_RETURN_NOT_OK(scope.status());
  gdv_device_pool_t* pool = nullptr;
  ARROW_RETURN_NOT_OK(impl_->Pool(&pool));
  const int64_t capacity = RoundUp(size);
  void* p = nullptr;
  GDV_DEV_RETURN_NOT_OK(gdv_device_pool_alloc(pool, capacity, &p));
  return std::unique_ptr<arrow::Buffer>(new HipBuffer(p, size, capacity, shared_from_this(), pool));
}

arrow::Result<std::shared_ptr<arrow::io::RandomAccessFile>> HipMemoryManager::GetBufferReader(std::shared_ptr<arrow::Buffer>) {
  return Status::NotImplemented("HipMemoryManager has no buffer reader: copy the buffer to the CPU");
}
arrow::Result<std::shared_ptr<arrow::io::OutputStream>> HipMemoryManager::GetBufferWriter(std::shared_ptr<arrow::Buffer>) {
  return Status::NotImplemented("HipMemoryManager has no buffer writer: copy a CPU buffer to the device");
}

arrow::Result<std::vector<std::shared_ptr<arrow::Buffer>>> HipMemoryManager::ReserveSet(int count, int64_t bytes, int candidates) {
  if (count < 1 || count > 32) return Status::Invalid("ReserveSet takes 1 .. 32 buffers, got ", count);
  if (bytes < 0) return Status::Invalid("negative allocation size");
  internal::DeviceScope scope(id_);
  ARROW_RETURN_NOT_OK(scope.status());
  gdv_device_pool_t* pool = nullptr;
  ARROW_RETURN_NOT_OK(impl_->Pool(&pool));
  const int64_t capacity = RoundUp(bytes);
  std::vector<void*> ptrs(count, nullptr);
  GDV_DEV_RETURN_NOT_OK(gdv_device_pool_reserve_set(pool, count, capacity, candidates, ptrs.data(), nullptr, nullptr, nullptr));
  std::vector<std::shared_ptr<arrow::Buffer>> out;
  for (void* p : ptrs) out.push_back(std::make_shared<HipBuffer>(p, bytes, capacity, shared_from_this(), pool));
  return out;
}

Status HipMemoryManager::Trim() {
  internal::DeviceScope scope(id_);
  ARROW_RETURN_NOT_OK(scope.status());
  std::lock_guard<std::mutex> g(impl_->mu);
  if (impl_->pool != nullptr) GDV_DEV_RETURN_NOT_OK(gdv_device_pool_trim(impl_->pool));
  return Status::OK();
}

int64_t HipMemoryManager::bytes_allocated(int64_t* in_use) const {
  std::lock_guard<std::mutex> g(impl_->mu);
  if (in_use) *in_use = 0;
  return impl_->pool != nullptr ? gdv_device_pool_bytes(impl_->pool, in_use) : 0;
}

arrow::Result<std::unique_ptr<arrow::Buffer>> HipMemoryManager::CopyNonOwnedFrom(const arrow::Buffer& buf,
                                                                                 const std::shared_ptr<arrow::MemoryManager>& from) {
  if (!from->is_cpu()) return nullptr;
  ARROW_ASSIGN_OR_RAISE(auto dst, AllocateBuffer(buf.size()));
  internal::DeviceScope scope(id_);
  ARROW_RETURN_NOT_OK(scope.status());
  uint8_t* d = reinterpret_cast<uint8_t*>(dst->address());
  if (buf.size() > 0) GDV_DEV_RETURN_NOT_OK(gdv_memcpy_h2d(d, buf.data(), buf.size()));
  // the padding is read with the last word of a bitmap and the last 16-byte piece of a byte buffer: zeroed, as Arrow's
  // own allocations are (the pool hands out recycled blocks)
  const int64_t pad = dst->capacity() - buf.size();
  if (pad > 0) GDV_DEV_RETURN_NOT_OK(gdv_memcpy_h2d(d + buf.size(), kZeros, pad));
  return dst;
}

arrow::Result<std::shared_ptr<arrow::Buffer>> HipMemoryManager::CopyBufferFrom(const std::shared_ptr<arrow::Buffer>& buf,
                                                                               const std::shared_ptr<arrow::MemoryManager>& from) {
  ARROW_ASSIGN_OR_RAISE(auto dst, CopyNonOwnedFrom(*buf, from));
  return std::shared_ptr<arrow::Buffer>(std::move(dst));
}

arrow::Result<std::unique_ptr<arrow::Buffer>> HipMemoryManager::CopyNonOwnedTo(const arrow::Buffer& buf,
                                                                               const std::shared_ptr<arrow::MemoryManager>& to) {
  if (!to->is_cpu()) return nullptr;
  ARROW_ASSIGN_OR_RAISE(auto dst, to->AllocateBuffer(buf.size()));
  if (buf.size() > 0) {
    internal::DeviceScope scope(id_);
    ARROW_RETURN_NOT_OK(scope.status());
    GDV_DEV_RETURN_NOT_OK(gdv_memcpy_d2h(dst->mutable_data(), reinterpret_cast<const void*>(buf.address()), buf.size()));
  }
  return dst;
}

arrow::Result<std::shared_ptr<arrow::Buffer>> HipMemoryManager::CopyBufferTo(const std::shared_ptr<arrow::Buffer>& buf,
                                                                             const std::shared_ptr<arrow::MemoryManager>& to) {
  ARROW_ASSIGN_OR_RAISE(auto dst, CopyNonOwnedTo(*buf, to));
  return std::shared_ptr<arrow::Buffer>(std::move(dst));
}

// ------------------------------------------------------------------ helpers

arrow::Result<std::shared_ptr<arrow::RecordBatch>> CopyBatchTo(const arrow::RecordBatch& batch,
                                                               const std::shared_ptr<arrow::MemoryManager>& to) {
  if (!to) return Status::Invalid("memory manager cannot be null");
  return batch.CopyTo(to);
}

arrow::Result<std::shared_ptr<SelectionVector>> MakeDeviceSelectionVector(SelectionVector::Mode mode, int64_t max_slots,
                                                                          const std::shared_ptr<HipMemoryManager>& mm) {
  if (!mm) return Status::Invalid("memory manager cannot be null");
  if (max_slots < 0) return Status::Invalid("max_slots cannot be negative");
  if (mode == SelectionVector::MODE_NONE) return Status::Invalid("selection vector mode cannot be NONE");
  if (mode == SelectionVector::MODE_UINT16 && max_slots > 65536)
    return Status::Invalid("max_slots cannot exceed 65536 for a 16-bit selection vector");
  const int w = mode == SelectionVector::MODE_UINT16 ? 2 : mode == SelectionVector::MODE_UINT32 ? 4 : 8;
  ARROW_ASSIGN_OR_RAISE(auto buf, mm->AllocateBuffer(std::max<int64_t>(max_slots, 1) * w));
  std::shared_ptr<SelectionVector> out;
  ARROW_RETURN_NOT_OK(SelectionVector::Make(mode, max_slots, std::shared_ptr<arrow::Buffer>(std::move(buf)), &out));
  return out;
}

}  // namespace gandiva
