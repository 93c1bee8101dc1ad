// hip/hip_runtime.h stand-in for tests/test_device_buffer_on_host.py: the allocation calls of csrc/hmpc_device_buffer.h on host memory, with
// the counters and the injected failures tests/src/device_buffer_on_host.cpp checks the owner types with.  Not a HIP runtime.
#pragma once
#include <cstddef>
#include <cstdlib>
#include <cstring>
typedef int hipError_t;
typedef void *hipStream_t;
enum { hipSuccess = 0, hipErrorOutOfMemory = 2, hipErrorInvalidValue = 1 };
struct ShimState {
  int live = 0;                          // allocations not yet freed
  int mallocs = 0, memsets = 0, frees = 0;
  int stream_syncs = 0, device_syncs = 0;
  int syncs_at_last_free = 0;            // stream_syncs + device_syncs when hipFree was last called
  hipStream_t last_synced = nullptr;
  int fail_malloc = 0, fail_memset = 0;  // N > 0: the N-th call from now fails (once)
};
inline ShimState g_shim;
inline hipError_t hipMalloc(void **p, size_t bytes) {
  ++g_shim.mallocs;
  if (g_shim.fail_malloc > 0 && --g_shim.fail_malloc == 0) return hipErrorOutOfMemory;  // (*p left as it was, as the runtime leaves it)
  *p = malloc(bytes ? bytes : 1);
  ++g_shim.live;
  return hipSuccess;
}
inline hipError_t hipFree(void *p) {
  ++g_shim.frees;
  g_shim.syncs_at_last_free = g_shim.stream_syncs + g_shim.device_syncs;
  if (p) free(p), --g_shim.live;
  return hipSuccess;
}
inline hipError_t hipMemset(void *p, int byte, size_t bytes) {
  ++g_shim.memsets;
  if (g_shim.fail_memset > 0 && --g_shim.fail_memset == 0) return hipErrorInvalidValue;
  memset(p, byte, bytes);
  return hipSuccess;
}
inline hipError_t hipStreamSynchronize(hipStream_t s) {
  ++g_shim.stream_syncs, g_shim.last_synced = s;
  return hipSuccess;
}
inline hipError_t hipDeviceSynchronize() {
  ++g_shim.device_syncs;
  return hipSuccess;
}
