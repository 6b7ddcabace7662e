// The one way libwca.so launches a kernel that needs more dynamic LDS than the default 64 KiB.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>

namespace wca {

constexpr int LDS_DEVICE_MAX = 160 * 1024;  // LDS of one gfx950 CU: the most a workgroup can ask for

// Raises the dynamic-LDS limit of `Kernel` to LDS_CAP, then launches it with `shmem` bytes. The limit is a per-device property of the
// kernel SYMBOL, not of a launch, so it is set to the compile-time cap -- never to the launch's own size -- once per (symbol, device)
// and remembered in a per-device bit mask: several engines (one per GPU) in one process and concurrent host threads are served
// correctly, and two threads that race on the first launch set the same value twice. The limit is only a ceiling: occupancy follows
// the size passed to the launch.
template <auto Kernel, int LDS_CAP, class... Args>
hipError_t launch_lds(dim3 grid, dim3 block, size_t shmem, hipStream_t s, const Args&... args) {
  static_assert(LDS_CAP > 0 && LDS_CAP <= LDS_DEVICE_MAX, "the cap is a size one CU has");
  if (shmem > (size_t)LDS_CAP) return hipErrorInvalidValue;
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  static std::atomic<unsigned> attr_mask{0};
  if (!(attr_mask.load(std::memory_order_acquire) & (1u << (dev & 31)))) {
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, LDS_CAP);
    if (e != hipSuccess) return e;
    attr_mask.fetch_or(1u << (dev & 31), std::memory_order_release);
  }
  hipLaunchKernelGGL(Kernel, grid, block, shmem, s, args...);
  return hipGetLastError();
}

}  // namespace wca
