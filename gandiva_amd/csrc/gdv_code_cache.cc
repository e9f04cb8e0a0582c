// Code objects: the cache directory, the in-memory and on-disk cache, the hipRTC compilation, and the background compiler of
// tier 0 with its ordering at process exit (declared in gdv_runtime.h).
#include <dlfcn.h>
#include <sys/syscall.h>
#include <hip/hiprtc.h>
#include <sys/stat.h>
#include <unistd.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <condition_variable>
#include <deque>
#include <mutex>
#include <set>
#include <thread>

#include "gdv_runtime.h"

namespace gdv {

static bool DirWritable(const std::string& d) {
  mkdir(d.c_str(), 0755);
  return access(d.c_str(), W_OK) == 0;
}

// A cache directory outside the installation is trusted only if it is ours and nobody else
// can write to it: code objects found there are loaded and run against the caller's HBM.
static bool PrivateDir(const std::string& d) {
  mkdir(d.c_str(), 0700);
  struct stat st;
  if (lstat(d.c_str(), &st) != 0 || !S_ISDIR(st.st_mode)) return false;
  if (st.st_uid != geteuid() || (st.st_mode & (S_IWGRP | S_IWOTH)) != 0) return false;
  return access(d.c_str(), W_OK) == 0;
}

std::string Runtime::cache_dir() {
  if (const char* e = std::getenv("GANDIVA_AMD_CACHE_DIR")) {
    std::string d = e;
    if (DirWritable(d)) return d;
  }
  // in-tree cache next to the shared library: travels with the repo snapshot
  Dl_info info;
  if (dladdr(reinterpret_cast<const void*>(&gdv_device_lib_src), &info) && info.dli_fname) {
    std::string so = info.dli_fname;
    size_t slash = so.rfind('/');
    std::string d = (slash == std::string::npos ? std::string(".") : so.substr(0, slash)) +
                    "/_kcache";
    if (DirWritable(d)) return d;
  }
  // per-user cache: $XDG_CACHE_HOME or ~/.cache, created 0700 and verified; as a last
  // resort a per-uid directory under /tmp with the same checks.  "" = no disk cache.
  std::string base;
  if (const char* x = std::getenv("XDG_CACHE_HOME")) base = x;
  else if (const char* h = std::getenv("HOME")) base = std::string(h) + "/.cache";
  if (!base.empty()) {
    mkdir(base.c_str(), 0700);
    std::string d = base + "/gandiva_amd_kcache";
    if (PrivateDir(d)) return d;
  }
  std::string d = "/tmp/gandiva_amd_kcache_" + std::to_string(static_cast<long>(geteuid()));
  if (PrivateDir(d)) return d;
  return "";
}

static uint64_t Fnv(const char* s, size_t n) {
  uint64_t h = 1469598103934665603ull;
  for (size_t i = 0; i < n; i++) {
    h ^= static_cast<unsigned char>(s[i]);
    h *= 1099511628211ull;
  }
  return h;
}

namespace {
// (never destroyed: the background compiler thread may still be inside CompileToCodeObject while the process's statics are
// torn down — it is joined by ~BackgroundCompiler, which can run AFTER these would have been destroyed)
std::mutex& CodeCacheMutex() { static std::mutex* m = new std::mutex; return *m; }
std::map<std::string, std::vector<char>>& CodeCache() { static auto* c = new std::map<std::string, std::vector<char>>; return *c; }
std::set<std::string>& FailedCompilations() { static auto* s = new std::set<std::string>; return *s; }
std::string LibraryHashTag() {  // the on-disk cache is keyed by the hash of the whole device library as well
  static const uint64_t lib_hash = Fnv(gdv_device_lib_src, strlen(gdv_device_lib_src));
  char tag[40];
  snprintf(tag, sizeof(tag), "%016llx", static_cast<unsigned long long>(lib_hash));
  return tag;
}
std::string CodeObjectPath(const std::string& dir, const std::string& kernel_name, const std::string& arch) {
  return dir + "/" + kernel_name + "." + LibraryHashTag() + "." + arch + ".hsaco";
}
bool CachedInMemory(const std::string& mem_key, std::vector<char>* code) {
  std::lock_guard<std::mutex> g(CodeCacheMutex());
  auto it = CodeCache().find(mem_key);
  if (it == CodeCache().end()) return false;
  *code = it->second;
  return true;
}

// The process's one background compiler thread (tier 0): compilations are serialised anyway (CompileToCodeObject), a
// queue keeps Make from waiting for them.  Joined at exit: a detached thread inside hipRTC while the statics of the
// process are torn down is a crash.
class BackgroundCompiler {
 public:
  // hipRTC loads its compiler (libamd_comgr) with dlopen on first use, i.e. from the worker thread, AFTER this object
  // exists: comgr's static destructors would then run BEFORE this object's at exit — while the worker may still be
  // compiling inside it (SIGSEGV at exit of any process that ends within a few hundred milliseconds of a Make; found by
  // tests/test_tier0.py and the C++ acceptance binary).  Loading comgr here, in the constructor, registers its
  // teardown first: this object's destructor — which stops the queue and JOINS the worker — runs before it.
  BackgroundCompiler() {
    for (const char* name : {"libamd_comgr.so.3", "libamd_comgr.so"}) (void)dlopen(name, RTLD_NOW | RTLD_GLOBAL);
  }
  static BackgroundCompiler& Get() { static BackgroundCompiler b; return b; }
  // stop accepting work, forget what is queued, wait for the compilation in flight (gdv_shutdown; also the destructor)
  void Shutdown() {
    { std::lock_guard<std::mutex> g(mu_); stop_ = true; jobs_.clear(); }
    cv_.notify_all();
    // (one joiner at a time: gdv_shutdown() on an embedder's thread may race exit() on the main thread; the loser of the
    // race returns only once the worker has ended, as a lone caller would)
    std::lock_guard<std::mutex> j(join_mu_);
    if (worker_.joinable()) worker_.join();
  }
  bool Push(std::string source, std::string name) {  // false: shut down — the caller compiles on its own thread
    std::lock_guard<std::mutex> g(mu_);
    if (stop_) return false;
    for (auto& j : jobs_) if (j.second == name) return true;
    jobs_.emplace_back(std::move(source), std::move(name));
    if (!started_) { started_ = true; worker_ = std::thread([this] { Run(); }); }
    cv_.notify_one();
    return true;
  }
  ~BackgroundCompiler() { Shutdown(); }

 private:
  void Run() {
    for (;;) {
      std::pair<std::string, std::string> job;
      {
        std::unique_lock<std::mutex> g(mu_);
        cv_.wait(g, [this] { return stop_ || !jobs_.empty(); });
        if (stop_) return;
        job = std::move(jobs_.front());
        jobs_.pop_front();
      }
      std::vector<char> code;
      Status st = Runtime::ForDevice(0).CompileToCodeObject(job.first, job.second, &code);
      if (!st.ok()) {
        std::lock_guard<std::mutex> g(CodeCacheMutex());
        FailedCompilations().insert(job.second);
      }
      // (the compiler's function-local statics that THIS compilation constructed are torn down, at exit, after a handler
      // registered now — see ExitHook)
      (void)std::atexit(&BackgroundCompiler::ExitHook);
    }
  }
 public:
  static void ExitHook() { Get().Shutdown(); }
 private:
  std::mutex mu_, join_mu_;
  std::condition_variable cv_;
  std::deque<std::pair<std::string, std::string>> jobs_;
  std::thread worker_;
  bool started_ = false, stop_ = false;
};
}  // namespace

int Runtime::CodeObjectState(const std::string& kernel_name, bool memory_only) {
  const std::string a = arch();
  {
    std::lock_guard<std::mutex> g(CodeCacheMutex());
    if (CodeCache().count(kernel_name + "." + a)) return 1;
    if (FailedCompilations().count(kernel_name)) return -1;
  }
  if (memory_only || std::getenv("GDV_NO_DISK_CACHE") != nullptr) return 0;
  const std::string dir = cache_dir();
  if (dir.empty()) return 0;
  return access(CodeObjectPath(dir, kernel_name, a).c_str(), R_OK) == 0 ? 1 : 0;
}

// Process exit with a compilation in flight.  exit() runs the exit handlers newest first, and the compiler (LLVM inside
// libamd_comgr) registers the destructors of its function-local statics as it first executes them, i.e. DURING compilations:
// they are newer than anything this library registered before, so at exit they are torn down first — under a worker that is
// still compiling (round 6, found with a cold code-object cache: the C++ acceptance binary, which finishes on tier 0 within a
// second of its first Make, crashed or hung in its exit).  Three layers:
//  * exit() destroys the CALLING thread's thread_local objects before it runs any handler: a guard object on every thread that
//    queues a compilation stops the queue and joins the worker from there when that thread is the process's main thread;
//  * a handler registered after every finished compilation (BackgroundCompiler::ExitHook) orders the join ahead of the teardown
//    of everything earlier compilations constructed — for processes whose main thread never called Make;
//  * gdv_shutdown() for embedders that can call it (the Python package does, from atexit).
namespace {
struct MainThreadExitGuard {
  MainThreadExitGuard() : tid(static_cast<long>(syscall(SYS_gettid))) {}
  ~MainThreadExitGuard() {
    if (tid == static_cast<long>(getpid())) Runtime::ShutdownBackgroundCompiler();
  }
  long tid;
};
}  // namespace

bool Runtime::CompileInBackground(const std::string& source, const std::string& kernel_name) {
  thread_local MainThreadExitGuard guard;
  (void)guard.tid;
  return BackgroundCompiler::Get().Push(source, kernel_name);
}
void Runtime::ShutdownBackgroundCompiler() { BackgroundCompiler::Get().Shutdown(); }

Status Runtime::CompileToCodeObject(const std::string& source, const std::string& kernel_name,
                                    std::vector<char>* code, bool* from_cache,
                                    bool ignore_cached) {
  const std::string a = arch();
  if (std::getenv("GDV_DUMP_SOURCE")) {
    const std::string d = cache_dir();
    std::ofstream f((d.empty() ? std::string("/tmp") : d) + "/" + kernel_name + ".hip");
    f << source;
  }
  // every context loads the same code object: compiled (or read from disk) once per process
  const std::string mem_key = kernel_name + "." + a;
  if (!ignore_cached && CachedInMemory(mem_key, code)) {
    if (from_cache) *from_cache = true;
    return Status::OK();
  }
  auto remember = [&]() {
    std::lock_guard<std::mutex> g(CodeCacheMutex());
    std::map<std::string, std::vector<char>>& code_cache = CodeCache();
    if (code_cache.size() > 2000) code_cache.clear();
    code_cache[mem_key] = *code;
  };
  const std::string dir = cache_dir();
  const std::string path = CodeObjectPath(dir, kernel_name, a);
  const bool use_disk = !dir.empty() && std::getenv("GDV_NO_DISK_CACHE") == nullptr;
  if (use_disk && ignore_cached) unlink(path.c_str());  // stale or corrupt: recompiled below
  if (use_disk && !ignore_cached) {
    std::ifstream f(path, std::ios::binary);
    if (f) {
      code->assign(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
      if (!code->empty()) {
        if (from_cache) *from_cache = true;
        remember();
        return Status::OK();
      }
    }
  }
  if (from_cache) *from_cache = false;

  // one compilation at a time: they are rare (cached in memory and on disk) and comgr's
  // temporary-file handling has no need to be exercised concurrently
  static std::mutex& compile_mu = *new std::mutex;  // (leaked on purpose: see CodeCacheMutex)
  std::lock_guard<std::mutex> compile_guard(compile_mu);
  // (another thread — the background compiler of tier 0 — may have produced it while this one waited)
  if (!ignore_cached && CachedInMemory(mem_key, code)) {
    if (from_cache) *from_cache = true;
    return Status::OK();
  }
  hiprtcProgram prog;
  const char* hdr_src[] = {gdv_device_lib_src};
  const char* hdr_name[] = {"gdv_device_lib.hpp"};
  if (hiprtcCreateProgram(&prog, source.c_str(), (kernel_name + ".hip").c_str(), 1, hdr_src,
                          hdr_name) != HIPRTC_SUCCESS)
    return Status::CodeGenError("hiprtcCreateProgram failed");
  std::string arch_opt = "--offload-arch=" + a;
  // -ffp-contract=off is part of the semantics (bit-exact vs separate mul/add)
  std::vector<const char*> opts = {arch_opt.c_str(), "-O3", "-std=c++17", "-ffp-contract=off",
                                   "-fhip-fp32-correctly-rounded-divide-sqrt"};
  // GDV_RTC_OPT: extra compiler options for experiments (e.g. -DGDV_COLD= inlines the cold
  // paths); not part of the cache key, so combine it with GDV_NO_DISK_CACHE=1
  std::vector<std::string> extra_opts;
  if (const char* extra = std::getenv("GDV_RTC_OPT")) {  // blank-separated list
    std::string cur;
    for (const char* c = extra;; c++) {
      if (*c == ' ' || *c == '\0') {
        if (!cur.empty()) extra_opts.push_back(cur);
        cur.clear();
        if (*c == '\0') break;
      } else {
        cur.push_back(*c);
      }
    }
    for (auto& o : extra_opts) opts.push_back(o.c_str());
  }
  hiprtcResult r = hiprtcCompileProgram(prog, static_cast<int>(opts.size()), opts.data());
  if (r != HIPRTC_SUCCESS) {
    size_t n = 0;
    hiprtcGetProgramLogSize(prog, &n);
    std::string log(n, '\0');
    if (n) hiprtcGetProgramLog(prog, &log[0]);
    hiprtcDestroyProgram(&prog);
    return Status::CodeGenError("kernel compilation failed:\n" + log);
  }
  size_t n = 0;
  hiprtcGetCodeSize(prog, &n);
  code->resize(n);
  hiprtcGetCode(prog, code->data());
  hiprtcDestroyProgram(&prog);
  if (use_disk) {
    std::string tmp = path + ".tmp." + std::to_string(getpid());
    std::ofstream f(tmp, std::ios::binary);
    if (f) {
      f.write(code->data(), static_cast<std::streamsize>(code->size()));
      f.close();
      rename(tmp.c_str(), path.c_str());
    }
  }
  remember();
  return Status::OK();
}

}  // namespace gdv
