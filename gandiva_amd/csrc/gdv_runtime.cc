// Device contexts and which one a thread uses, the probe, loading and launching kernels (the other units of gdv_runtime.h:
// gdv_code_cache.cc, gdv_device_memory.cc, gdv_host_registry.cc).
#include "gdv_runtime.h"

#include <algorithm>
#include <cstdlib>

namespace gdv {

namespace {
std::mutex g_contexts_mu;
Runtime* g_contexts[Runtime::kMaxDevices] = {};
int g_virtual_devices = 0;
thread_local int tl_selected_device = -1;

int PhysicalCountUncached() {
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) {
    (void)hipGetLastError();
    return 0;
  }
  return count;
}
}  // namespace

int Runtime::PhysicalDeviceCount() {
  static const int count = PhysicalCountUncached();
  return count;
}

int Runtime::DeviceCount() {
  int v = 0;
  {
    std::lock_guard<std::mutex> g(g_contexts_mu);
    v = g_virtual_devices;
  }
  if (v == 0) {  // GDV_VIRTUAL_DEVICES: read once per process
    static const int from_env = [] { const char* e = std::getenv("GDV_VIRTUAL_DEVICES"); return e ? atoi(e) : 0; }();
    v = from_env;
  }
  const int phys = PhysicalDeviceCount();
  if (phys == 0) return 0;
  return std::min<int>(kMaxDevices, std::max(phys, v));
}

void Runtime::SetVirtualDevices(int n) {
  std::lock_guard<std::mutex> g(g_contexts_mu);
  g_virtual_devices = std::max(0, std::min<int>(n, kMaxDevices));
}

Runtime& Runtime::ForDevice(int id) {
  if (id < 0 || id >= kMaxDevices) id = 0;
  std::lock_guard<std::mutex> g(g_contexts_mu);
  // never destroyed: cached Projectors / Filters (process-wide LRUs) own pooled device blocks and
  // hand them back during static destruction, in an order the contexts must outlive
  if (g_contexts[id] == nullptr) g_contexts[id] = new Runtime(id);
  return *g_contexts[id];
}

int Runtime::SelectedDevice() {
  if (tl_selected_device >= 0) return tl_selected_device;
  int dev = 0;
  if (PhysicalDeviceCount() > 0 && hipGetDevice(&dev) != hipSuccess) {
    (void)hipGetLastError();
    dev = 0;
  }
  return dev;
}

Runtime& Runtime::Get() { return ForDevice(SelectedDevice()); }

Status Runtime::SelectDevice(int id) {
  const int n = DeviceCount();
  if (n == 0) return Status::ExecutionError("no HIP device available");
  if (id < 0 || id >= n)
    return Status::Invalid("device " + std::to_string(id) + " out of range (" + std::to_string(n) + " devices)");
  tl_selected_device = id;
  return ForDevice(id).EnsureDevice();
}

void Runtime::Probe() {
  if (probed_) return;
  probed_ = true;
  const int count = PhysicalDeviceCount();
  if (count <= 0) {
    has_device_ = false;
    if (const char* a = std::getenv("GDV_ARCH")) arch_ = a;
    return;
  }
  has_device_ = true;
  physical_ = id_ % count;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, physical_) == hipSuccess) {
    num_cus_ = prop.multiProcessorCount;
    std::string a = prop.gcnArchName;  // e.g. "gfx950:sramecc+:xnack-"
    size_t colon = a.find(':');
    arch_ = colon == std::string::npos ? a : a.substr(0, colon);
  }
}

bool Runtime::has_device() {
  std::lock_guard<std::mutex> g(mu_);
  Probe();
  return has_device_;
}

Status Runtime::EnsureDevice() {
  if (!has_device())
    return Status::ExecutionError(
        "no HIP device available: gandiva_amd evaluates on the GPU only (there is no CPU "
        "fallback)");
  // Code objects, the buffer pool and the all-ones word of this context live on physical_:
  // make it the calling thread's HIP device (a thread that never chose one starts on device 0).
  int dev = -1;
  if (hipGetDevice(&dev) != hipSuccess || dev != physical_) {
    hipError_t e = hipSetDevice(physical_);
    if (e != hipSuccess)
      return Status::ExecutionError("could not make HIP device " + std::to_string(physical_) +
                                    " current on the calling thread: " + hipGetErrorString(e));
  }
  return Status::OK();
}

int Runtime::num_cus() {
  std::lock_guard<std::mutex> g(mu_);
  Probe();
  return num_cus_;
}

const std::string& Runtime::arch() {
  std::lock_guard<std::mutex> g(mu_);
  Probe();
  return arch_;
}

static hipError_t LoadModule(const std::vector<char>& code, const std::string& name, CompiledKernel* k) {
  hipError_t e = hipModuleLoadData(&k->module, code.data());
  if (e == hipSuccess && !k->small_only) e = hipModuleGetFunction(&k->function, k->module, name.c_str());
  return e;
}

static hipFunction_t OptionalEntry(const CompiledKernel& k, const std::string& entry) {  // nullptr: the module has none
  hipFunction_t f = nullptr;
  if (hipModuleGetFunction(&f, k.module, entry.c_str()) == hipSuccess) return f;
  (void)hipGetLastError();
  return nullptr;
}

Status Runtime::GetKernel(const std::string& source, const std::string& kernel_name,
                          const CompiledKernel** out) {
  GDV_RETURN_NOT_OK(EnsureDevice());
  {
    std::lock_guard<std::mutex> g(mu_);
    auto it = kernels_.find(kernel_name);
    if (it != kernels_.end()) {
      *out = it->second.get();
      return Status::OK();
    }
  }
  std::vector<char> code;
  bool from_cache = false;
  GDV_RETURN_NOT_OK(CompileToCodeObject(source, kernel_name, &code, &from_cache));
  auto k = std::make_unique<CompiledKernel>();
  k->name = kernel_name;
  // (the small shape of a fused filter-project: a code object with the <name>_small / <name>_small1 entries alone)
  k->small_only = source.find(" " + kernel_name + "(") == std::string::npos && source.find(kernel_name + "_small(") != std::string::npos;
  hipError_t le = LoadModule(code, kernel_name, k.get());
  if (le != hipSuccess && from_cache) {
    // a cached code object that does not load (truncated, built by another toolchain): drop
    // the file and compile afresh instead of failing every Make from now on
    (void)hipGetLastError();
    if (k->module != nullptr) (void)hipModuleUnload(k->module);
    k->module = nullptr;
    GDV_RETURN_NOT_OK(CompileToCodeObject(source, kernel_name, &code, nullptr, true));
    le = LoadModule(code, kernel_name, k.get());
  }
  if (le != hipSuccess)
    return Status::ExecutionError(std::string("loading the compiled kernel failed: ") + hipGetErrorString(le));
  if (source.find(kernel_name + "_many(") != std::string::npos) k->function_many = OptionalEntry(*k, kernel_name + "_many");
  if (source.find(kernel_name + "_small(") != std::string::npos) k->function_small = OptionalEntry(*k, kernel_name + "_small");
  if (k->function_small != nullptr) k->function_small1 = OptionalEntry(*k, kernel_name + "_small1");
  std::lock_guard<std::mutex> g(mu_);
  auto& slot = kernels_[kernel_name];
  if (!slot) slot = std::move(k);
  *out = slot.get();
  return Status::OK();
}

Status Runtime::AllOnesWord(const uint64_t** ptr) {
  GDV_RETURN_NOT_OK(EnsureDevice());
  std::lock_guard<std::mutex> g(mu_);
  if (all_ones_ == nullptr) {
    void* p = nullptr;
    GDV_HIP_RETURN_NOT_OK(hipMalloc(&p, 256));
    GDV_HIP_RETURN_NOT_OK(hipMemset(p, 0xff, 256));
    all_ones_ = static_cast<uint64_t*>(p);
  }
  *ptr = all_ones_;
  return Status::OK();
}

Status Runtime::LaunchMany(const CompiledKernel& k, int64_t grid_x, int64_t batches, int block,
                           const void* table_device, hipStream_t stream, bool small) {
  hipFunction_t fn = small ? k.function_small : k.function_many;
  if (fn == nullptr) return Status::ExecutionError("kernel has no multi-batch entry point");
  void* params[] = {&table_device};
  GDV_HIP_RETURN_NOT_OK(hipModuleLaunchKernel(fn, static_cast<unsigned>(grid_x),
                                              static_cast<unsigned>(batches), 1, static_cast<unsigned>(block), 1, 1,
                                              0, stream, params, nullptr));
  return Status::OK();
}

Status Runtime::Launch(const CompiledKernel& k, int64_t grid, int block, const void* args,
                       size_t arg_bytes, hipStream_t stream, hipFunction_t entry) {
  void* config[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, const_cast<void*>(args),
                    HIP_LAUNCH_PARAM_BUFFER_SIZE, &arg_bytes, HIP_LAUNCH_PARAM_END};
  GDV_HIP_RETURN_NOT_OK(hipModuleLaunchKernel(entry != nullptr ? entry : k.function, static_cast<unsigned>(grid), 1, 1,
                                              static_cast<unsigned>(block), 1, 1, 0, stream,
                                              nullptr, config));
  return Status::OK();
}

}  // namespace gdv
