// Library-wide device state: the CUs the persistent grids may occupy, and the note of the last ping-pong NT grid (tests).
// Explicit library state (round 2 read an environment variable ONCE, at the first GEMM launch, so a reducer built after any forward
// was silently ignored): vitssl_set_reserved_cus() takes effect at the next launch of every persistent grid (forward / input-gradient
// / weight-gradient GEMMs, LayerNorm backward).  VITSSL_RESERVE_CUS only provides the initial value.
#include "common.h"

static std::atomic<int> g_reserved_cus{-1};     // -1 = not initialised
static std::atomic<int> g_device_cus{0};
static std::atomic<int> g_last_nt_grid{0};

static int device_cus() {
  int c = g_device_cus.load(std::memory_order_relaxed);
  if (c > 0) return c;
  int dev = 0, cus = 0;
  hipDeviceProp_t prop;
  if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess) cus = prop.multiProcessorCount;
  if (cus <= 0) cus = 256;
  g_device_cus.store(cus, std::memory_order_relaxed);
  return cus;
}

static int clamp_reserve(int n) {
  const int cus = device_cus();
  if (n < 0) n = 0;
  if (n > cus - 8) n = cus - 8;
  return n;
}

extern "C" int vitssl_get_reserved_cus(void) {
  int r = g_reserved_cus.load(std::memory_order_relaxed);
  if (r < 0) {
    const char* e = getenv("VITSSL_RESERVE_CUS");
    r = clamp_reserve(e ? atoi(e) : 0);
    g_reserved_cus.store(r, std::memory_order_relaxed);
  }
  return r;
}

extern "C" int vitssl_set_reserved_cus(int n) {
  if (n < 0) {
    vitssl_set_error("set_reserved_cus: negative count %d", n);
    return VITSSL_ERR_ARG;
  }
  g_reserved_cus.store(clamp_reserve(n), std::memory_order_relaxed);
  return VITSSL_OK;
}

int vitssl_persistent_cus(void) { return device_cus() - vitssl_get_reserved_cus(); }

void vitssl_note_nt_grid(int grid) { g_last_nt_grid.store(grid, std::memory_order_relaxed); }
extern "C" int vitssl_debug_last_nt_grid(void) { return g_last_nt_grid.load(std::memory_order_relaxed); }
