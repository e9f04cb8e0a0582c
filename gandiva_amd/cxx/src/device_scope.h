// Private to libgandiva.so: the calling thread's library device (gdv_set_device) switched for one call.
#pragma once
#include "gandiva/arrow.h"
#include "gandiva_amd.h"

namespace gandiva {
namespace internal {

// Selects `device` (a negative number: nothing) and puts the caller's device back when it goes out of scope.
class DeviceScope {
 public:
  explicit DeviceScope(int device) {
    if (device < 0) return;
    prev_ = gdv_get_device();
    if (prev_ == device) return;
    const int rc = gdv_set_device(device);
    if (rc != GDV_OK) {
      status_ = Status(static_cast<arrow::StatusCode>(rc), gdv_last_error());
      return;
    }
    switched_ = true;
  }
  ~DeviceScope() {
    if (switched_) (void)gdv_set_device(prev_);
  }
  DeviceScope(const DeviceScope&) = delete;
  DeviceScope& operator=(const DeviceScope&) = delete;
  const Status& status() const { return status_; }

 private:
  int prev_ = 0;
  bool switched_ = false;
  Status status_;
};

}  // namespace internal
}  // namespace gandiva
