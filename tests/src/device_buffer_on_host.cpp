// The owner types of the handle's device memory (csrc/hmpc_device_buffer.h) on the host: built against tests/src/hip_alloc_shim, whose
// hipMalloc / hipFree / hipMemset are malloc / free / memset with counters and injected failures.  Built with AddressSanitizer and UBSan by
// tests/test_device_buffer_on_host.py, so a double free, a leak of the shim's own memory or a use after free ends the run.
#include <cstdio>
#include <utility>

#include "hmpc_device_buffer.h"

static int g_problems = 0;
#define CHECK(cond)                                                   \
  do {                                                                \
    if (!(cond)) {                                                    \
      printf("line %d: CHECK(%s) failed\n", __LINE__, #cond);         \
      ++g_problems;                                                   \
    }                                                                 \
  } while (0)

static int syncs() { return g_shim.stream_syncs + g_shim.device_syncs; }

int main() {
  // ---- ownership: destruction and moves
  {
    DeviceBuffer<int> a;
    CHECK(a.get() == nullptr && a.bytes() == 0);
    CHECK(a.alloc(10) == hipSuccess && a.get() && a.bytes() == 10 * sizeof(int) && g_shim.live == 1);
    a.get()[9] = 7;  // (the whole size is there: the sanitizer watches)
  }
  CHECK(g_shim.live == 0);
  {
    DeviceBuffer<double> a;
    CHECK(a.alloc(4) == hipSuccess);
    double *p = a.get();
    DeviceBuffer<double> b(std::move(a));
    CHECK(a.get() == nullptr && a.bytes() == 0 && b.get() == p && b.bytes() == 32 && g_shim.live == 1);
    DeviceBuffer<double> c;
    CHECK(c.alloc(2) == hipSuccess && g_shim.live == 2);
    c = std::move(b);  // frees what c held, takes b's
    CHECK(b.get() == nullptr && b.bytes() == 0 && c.get() == p && c.bytes() == 32 && g_shim.live == 1);
    c = std::move(c);  // (self-move: nothing happens)
    CHECK(c.get() == p && g_shim.live == 1);
    c.reset();
    CHECK(c.get() == nullptr && c.bytes() == 0 && g_shim.live == 0);
  }
  CHECK(g_shim.live == 0);
  {
    DeviceBuffer<int> a;
    g_shim.fail_malloc = 1;
    CHECK(a.alloc(3) != hipSuccess && a.get() == nullptr && a.bytes() == 0 && g_shim.live == 0);
  }
  CHECK(g_shim.live == 0);

  // ---- alloc_filled: filled on success; nothing kept, nothing live when either call fails
  {
    DeviceBuffer<int> a;
    CHECK(a.alloc_filled(5, 0xff) == hipSuccess && a.bytes() == 20 && g_shim.live == 1);
    for (int i = 0; i < 5; ++i) CHECK(a.get()[i] == -1);
    DeviceBuffer<unsigned> z;
    CHECK(z.alloc_filled(2, 0) == hipSuccess && z.get()[0] == 0 && z.get()[1] == 0);
    DeviceBuffer<int> b;
    g_shim.fail_memset = 1;
    CHECK(b.alloc_filled(5, 0xff) != hipSuccess && b.get() == nullptr && b.bytes() == 0 && g_shim.live == 2);
    g_shim.fail_malloc = 1;
    const int memsets = g_shim.memsets;
    CHECK(b.alloc_filled(5, 0xff) != hipSuccess && b.get() == nullptr && b.bytes() == 0 && g_shim.live == 2 && g_shim.memsets == memsets);
    // the second allocation / fill of a pair fails: the first, a local, goes with its scope (the both-or-neither commits of hmpc_capi.hip)
    {
      DeviceBuffer<int> first, second;
      g_shim.fail_memset = 2;
      CHECK(first.alloc_filled(4, 0) == hipSuccess && second.alloc_filled(4, 0) != hipSuccess && g_shim.live == 3);
    }
    CHECK(g_shim.live == 2);
  }
  CHECK(g_shim.live == 0);

  // ---- reserve
  {
    DeviceBuffer<unsigned char> a;
    int stream_tag = 0;
    hipStream_t st = &stream_tag;
    int s0 = syncs(), f0 = g_shim.frees;
    CHECK(a.reserve(4096, st, false) == hipSuccess && a.bytes() == 4096 && g_shim.live == 1);
    CHECK(syncs() == s0 && g_shim.frees == f0);  // (nothing to wait for, nothing to free)
    unsigned char *p = a.get();
    const int m0 = g_shim.mallocs;
    CHECK(a.reserve(4096, st, false) == hipSuccess && a.reserve(100, st, true) == hipSuccess);  // large enough: kept
    CHECK(a.get() == p && a.bytes() == 4096 && g_shim.mallocs == m0 && syncs() == s0 && g_shim.frees == f0);
    // grows: the stream is synchronised exactly once, before the free
    CHECK(a.reserve(8192, st, false) == hipSuccess && a.bytes() == 8192 && g_shim.live == 1);
    CHECK(g_shim.stream_syncs == 1 && g_shim.device_syncs == 0 && g_shim.last_synced == st);
    CHECK(g_shim.frees == f0 + 1 && g_shim.syncs_at_last_free == s0 + 1);
    a.get()[8191] = 1;
    // ... or the whole device
    s0 = syncs(), f0 = g_shim.frees;
    CHECK(a.reserve(8193, st, true) == hipSuccess && a.bytes() == 8193 && g_shim.live == 1);
    CHECK(g_shim.stream_syncs == 1 && g_shim.device_syncs == 1 && g_shim.frees == f0 + 1 && g_shim.syncs_at_last_free == s0 + 1);
    // the new allocation fails: empty, size 0, and the next call starts afresh
    g_shim.fail_malloc = 1;
    CHECK(a.reserve(1 << 20, st, false) != hipSuccess && a.get() == nullptr && a.bytes() == 0 && g_shim.live == 0);
    s0 = syncs();
    CHECK(a.reserve(64, st, false) == hipSuccess && a.bytes() == 64 && g_shim.live == 1 && syncs() == s0);
  }
  CHECK(g_shim.live == 0);

  // ---- OutputBuffer
  {
    OutputBuffer<float> o;
    float mine[4] = {0};
    CHECK(o.get() == nullptr);
    o.set_caller(mine);
    const int m0 = g_shim.mallocs;
    CHECK(o.ensure(4) == hipSuccess && g_shim.mallocs == m0 && g_shim.live == 0);  // a caller buffer is set: nothing allocated
    CHECK(o.get() == mine);
    o.set_caller(nullptr);
    CHECK(o.get() == nullptr);  // (the handle's own does not exist yet)
    CHECK(o.ensure(4) == hipSuccess && g_shim.live == 1 && o.get() != nullptr && o.get() != mine);
    float *own = o.get();
    own[3] = 1.f;
    CHECK(o.ensure(4) == hipSuccess && g_shim.live == 1 && o.get() == own);  // first need only
    o.set_caller(mine);
    CHECK(o.get() == mine && o.ensure(4) == hipSuccess && g_shim.live == 1);
    o.set_caller(nullptr);
    CHECK(o.get() == own);  // back to the handle's own, still there
    OutputBuffer<float> failing;
    g_shim.fail_malloc = 1;
    CHECK(failing.ensure(4) != hipSuccess && failing.get() == nullptr && g_shim.live == 1);
    CHECK(failing.ensure(4) == hipSuccess && failing.get() != nullptr && g_shim.live == 2);  // the next need tries again
  }
  CHECK(g_shim.live == 0);

  printf("%d problems\n", g_problems);
  return g_problems ? 1 : 0;
}
