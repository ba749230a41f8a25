// Host-side plumbing both translation units (pc_engine.hip, pc_kkt.hip) use: HIP errors as exceptions, device and pinned
// buffers that free themselves, and the try / catch around every exported call.
#pragma once
#include <hip/hip_runtime.h>

#include <chrono>
#include <stdexcept>
#include <string>
#include <vector>

#define HIP_OK(expr)                                                                             \
  do {                                                                                           \
    hipError_t e_ = (expr);                                                                      \
    if (e_ != hipSuccess)                                                                        \
      throw std::runtime_error(std::string(#expr) + ": " + hipGetErrorString(e_));              \
  } while (0)

template <class T>
struct DevBuf {
  T* p = nullptr;
  size_t n = 0;
  void alloc(size_t count) {
    free();
    n = count;
    if (count) HIP_OK(hipMalloc(&p, count * sizeof(T)));
  }
  void upload(const T* src, size_t count) {
    if (count != n) alloc(count);   // same size: keep the allocation (pointers held in argument blocks stay valid)
    if (count) HIP_OK(hipMemcpy(p, src, count * sizeof(T), hipMemcpyHostToDevice));
  }
  void upload(const std::vector<T>& v) { upload(v.data(), v.size()); }
  void free() {
    if (p) (void)hipFree(p);
    p = nullptr;
    n = 0;
  }
  ~DevBuf() { free(); }
};

// pinned host staging: the vectors of a call cross the bus from / to page-locked memory (a pageable hipMemcpyAsync is
// staged by the runtime through its own bounce buffer, synchronously: ~0.1 ms per 240 KB vector at config 2, more than
// the KKT solve's kernels)
template <class T>
struct PinBuf {
  T* p = nullptr;
  size_t n = 0;
  void alloc(size_t count) {
    free();
    n = count;
    if (count) HIP_OK(hipHostMalloc(&p, count * sizeof(T), hipHostMallocDefault));
  }
  void free() {
    if (p) (void)hipHostFree(p);
    p = nullptr;
    n = 0;
  }
  ~PinBuf() { free(); }
};

// Wait for a stream or an event.  A blocking wait costs an interrupt and a wake-up (~10 us on the MI355X host, a quarter
// of a 10 k-node callback): `query` is polled for `spin_us` first, which is where a callback completes, then `block`
// is called.  A query error other than "not ready" is thrown.
template <class Query, class Block>
void poll_then_block(Query&& query, Block&& block, int spin_us) {
  if (spin_us > 0) {
    const auto t0 = std::chrono::steady_clock::now();
    for (;;) {
      const hipError_t e = query();
      if (e == hipSuccess) return;
      if (e != hipErrorNotReady) HIP_OK(e);
      if (std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count() > spin_us) break;
    }
  }
  HIP_OK(block());
}
inline void wait_for(hipStream_t st, int spin_us) {
  poll_then_block([&] { return hipStreamQuery(st); }, [&] { return hipStreamSynchronize(st); }, spin_us);
}
inline void wait_for(hipEvent_t ev, int spin_us) {
  poll_then_block([&] { return hipEventQuery(ev); }, [&] { return hipEventSynchronize(ev); }, spin_us);
}

// an exported call's body: 1, or 0 with the exception's text in `err` (the caller's thread-local last-error string)
template <class F>
int guarded(std::string& err, F&& f) {
  try {
    f();
    return 1;
  } catch (const std::exception& e) {
    err = e.what();
    return 0;
  }
}
