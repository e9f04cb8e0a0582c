// C ABI, device and host memory: properties, alloc/free, the pool, copies, registered host memory, HBM ceiling probes.
#include "gdv_c_api_internal.h"

#include "gdv_kernels.h"

using namespace gdv;
using namespace gdv::capi;

extern "C" {

int gdv_device_num_cus(void) { return Runtime::Get().num_cus(); }
const char* gdv_device_arch(void) { return Runtime::Get().arch().c_str(); }
int gdv_device_alloc(int64_t bytes, void** ptr) {
  if (!ptr || bytes < 0) return Fail(Status::Invalid("bad argument"));
  return Check(Runtime::Get().Alloc(static_cast<size_t>(bytes ? bytes : 1), ptr));
}
int gdv_device_free(void* ptr) { Runtime::Get().Free(ptr); return GDV_OK; }
int gdv_device_pool_create(gdv_device_pool_t** out) {
  return Guarded([&]() -> int {
    if (!out) return Fail(Status::Invalid("null output pointer"));
    Status st = Runtime::Get().EnsureDevice();
    if (!st.ok()) return Fail(st);
    *out = new gdv_device_pool();
    return GDV_OK;
  });
}
void gdv_device_pool_destroy(gdv_device_pool_t* pool) { delete pool; }
int gdv_device_pool_reserve_set(gdv_device_pool_t* pool, int count, int64_t bytes, int candidates, void** ptrs, double* rates,
                                int* tried, int* kept) {
  return Guarded([&]() -> int {
    if (!pool) return Fail(Status::Invalid("null pool"));
    return Check(pool->pool.ReserveSet(count, bytes, candidates, ptrs, rates, tried, kept));
  });
}
int gdv_device_pool_alloc(gdv_device_pool_t* pool, int64_t bytes, void** ptr) {
  return Guarded([&]() -> int {
    if (!pool) return Fail(Status::Invalid("null pool"));
    return Check(pool->pool.Alloc(bytes, ptr));
  });
}
int gdv_device_pool_free(gdv_device_pool_t* pool, void* ptr) {
  return Guarded([&]() -> int {
    if (!pool) return Fail(Status::Invalid("null pool"));
    return Check(pool->pool.Free(ptr));
  });
}
int gdv_device_pool_trim(gdv_device_pool_t* pool) {
  return Guarded([&]() -> int {
    if (!pool) return Fail(Status::Invalid("null pool"));
    return Check(pool->pool.Trim());
  });
}
int64_t gdv_device_pool_bytes(const gdv_device_pool_t* pool, int64_t* in_use) { return pool ? pool->pool.bytes_held(in_use) : 0; }
int gdv_memcpy_h2d(void* dst, const void* src, int64_t bytes) {
  hipError_t e = hipMemcpy(dst, src, static_cast<size_t>(bytes), hipMemcpyHostToDevice);
  return e == hipSuccess ? GDV_OK : Fail(Status::ExecutionError(hipGetErrorString(e)));
}
int gdv_memcpy_d2h(void* dst, const void* src, int64_t bytes) {
  hipError_t e = hipMemcpy(dst, src, static_cast<size_t>(bytes), hipMemcpyDeviceToHost);
  return e == hipSuccess ? GDV_OK : Fail(Status::ExecutionError(hipGetErrorString(e)));
}
int gdv_host_register(void* ptr, int64_t bytes) {
  return Guarded([&]() -> int {
  if (bytes < 0) return Fail(Status::Invalid("bad argument"));
  return Check(HostRegistry::Get().Register(ptr, static_cast<size_t>(bytes)));
  });
}
int gdv_host_unregister(void* ptr) {
  return Guarded([&]() -> int { return Check(HostRegistry::Get().Unregister(ptr)); });
}
int gdv_host_alloc(int64_t bytes, void** ptr) {
  return Guarded([&]() -> int {
  if (bytes < 0) return Fail(Status::Invalid("bad argument"));
  return Check(HostRegistry::Get().Alloc(static_cast<size_t>(bytes), ptr));
  });
}
int gdv_host_free(void* ptr) {
  return Guarded([&]() -> int { return Check(HostRegistry::Get().Free(ptr)); });
}
int64_t gdv_host_staged_bytes(void) { return HostRegistry::StagedBytes().load(std::memory_order_relaxed); }
int gdv_device_hbm_ceilings(int64_t bytes, double* read_gbs, double* write_gbs, double* copy_gbs) {
  return Guarded([&]() -> int {
  if (bytes < (1 << 20) || !read_gbs || !write_gbs || !copy_gbs) return Fail(Status::Invalid("bad argument"));
  bytes &= ~int64_t{4095};
  Runtime& rt = Runtime::Get();
  Status st = rt.EnsureDevice();
  if (!st.ok()) return Fail(st);
  DeviceBuffer a, b;
  st = a.Allocate(static_cast<size_t>(bytes));
  if (st.ok()) st = b.Allocate(static_cast<size_t>(bytes));
  if (!st.ok()) return Fail(st);
  hipError_t e = hipMemset(a.get(), 1, static_cast<size_t>(bytes));
  if (e == hipSuccess) e = hipMemset(b.get(), 2, static_cast<size_t>(bytes));
  if (e == hipSuccess)
    e = MeasureHbmCeilings(a.get(), b.get(), static_cast<size_t>(bytes), rt.num_cus() * 16, read_gbs, write_gbs, copy_gbs);
  if (e == hipSuccess) e = hipDeviceSynchronize();
  return e == hipSuccess ? GDV_OK : Fail(Status::ExecutionError(hipGetErrorString(e)));
  });
}
int gdv_device_stream_ceiling(int64_t bytes_per_stream, int num_read, int num_write, double* gbs, int* workgroups_per_cu,
                              int* nontemporal) {
  return Guarded([&]() -> int {
  if (bytes_per_stream < (1 << 20) || !gbs || num_read < 0 || num_write < 0 || num_read + num_write < 1 ||
      num_read > 10 || num_write > 10)
    return Fail(Status::Invalid("bad argument"));
  bytes_per_stream &= ~int64_t{8191};
  Runtime& rt = Runtime::Get();
  Status st = rt.EnsureDevice();
  if (!st.ok()) return Fail(st);
  std::vector<DeviceBuffer> bufs(num_read + num_write);
  std::vector<void*> ptrs;
  for (auto& b : bufs) {
    st = b.Allocate(static_cast<size_t>(bytes_per_stream));
    if (!st.ok()) return Fail(st);
    hipError_t e = hipMemset(b.get(), 1, static_cast<size_t>(bytes_per_stream));
    if (e != hipSuccess) return Fail(Status::ExecutionError(hipGetErrorString(e)));
    ptrs.push_back(b.get());
  }
  int wg = 0, nt = 0;
  hipError_t e = MeasureStreamCeiling(ptrs.data(), num_read, num_write, static_cast<size_t>(bytes_per_stream / 8), rt.num_cus(),
                                      gbs, &wg, &nt);
  return StreamCeilingResult(e, wg, nt, workgroups_per_cu, nontemporal);
  });
}
int gdv_device_stream_ceiling_on(void* const* streams, int num_read, int num_write, int64_t elems, double* gbs,
                                 int* workgroups_per_cu, int* nontemporal) {
  return Guarded([&]() -> int {
  if (!streams || !gbs || elems < 1024 || num_read < 0 || num_write < 0 || num_read + num_write < 1 || num_read > 10 ||
      num_write > 10)
    return Fail(Status::Invalid("bad argument"));
  for (int i = 0; i < num_read + num_write; i++)
    if (streams[i] == nullptr) return Fail(Status::Invalid("null stream"));
  Runtime& rt = Runtime::Get();
  Status st = rt.EnsureDevice();
  if (!st.ok()) return Fail(st);
  int wg = 0, nt = 0;
  hipError_t e = MeasureStreamCeiling(streams, num_read, num_write, static_cast<size_t>(elems), rt.num_cus(), gbs, &wg, &nt);
  return StreamCeilingResult(e, wg, nt, workgroups_per_cu, nontemporal);
  });
}
int gdv_device_synchronize(void) {
  hipError_t e = hipDeviceSynchronize();
  return e == hipSuccess ? GDV_OK : Fail(Status::ExecutionError(hipGetErrorString(e)));
}

}  // extern "C"
