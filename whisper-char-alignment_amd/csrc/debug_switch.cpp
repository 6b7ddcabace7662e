// Process-wide test switches of libwca.so (every default, 0, is the shipped choice, and the parity / bit-identity claims hold for it). They are set
// only through the test entry point wca_test_set_switch; no environment variable selects a kernel.
#include <atomic>
#include <cstring>

#include "kernels.h"

namespace wca {

namespace {
struct Sw {
  const char* name;
  std::atomic<int> value;
};
Sw g_sw[DBG_SWITCH_COUNT] = {
    {"attn_split_variant", {0}},    // 1: the pair attention on the 16x16x32 kernel everywhere
    {"head_stats_general", {0}},    // 1: the general head-statistics kernel
    {"fail_precision_alloc", {0}},  // 1: inject an allocation failure into wca_set_precision
    {"attn_split_drop", {0}},       // pass mask of the encoder's pair attention (wca_test_set_attn_split_drop)
    {"gemm_ring", {0}},             // 1: the pair GEMM on round 4's two-slot rings (default: three A slots + one W slot)
};
}  // namespace

int debug_switch(int id) {
  if (id < 0 || id >= DBG_SWITCH_COUNT) return 0;
  return g_sw[id].value.load(std::memory_order_relaxed);
}

int set_debug_switch(const char* name, int value) {
  for (int i = 0; i < DBG_SWITCH_COUNT; ++i)
    if (std::strcmp(g_sw[i].name, name) == 0) {
      g_sw[i].value.store(value, std::memory_order_relaxed);
      return 0;
    }
  return -1;
}

}  // namespace wca
