// Launch-side state of libhnr_hip.so, in one place: the HNR_... tuning / probe switches, the per-device CU count, and the launch of a kernel that
// needs more dynamic LDS than the 64 KB a kernel gets without asking.
//
// The first part is plain C++ (no HIP runtime; device indices are arguments): tools/launch_state_check.cpp hammers it from threads under
// -fsanitize=thread.  The second part, for the .hip files, binds it to the HIP runtime.
#pragma once
#include <atomic>
#include <mutex>
#include <stdlib.h>

namespace hnr {

// ---- switches.  Every HNR_... environment variable of the library is read through these two (INTEGRATION.md lists them; tests/test_abi_and_host.py
//      compares that list with the names passed here).  atoi parsing: "abc" and "" read as 0.
// knob_now: reads the environment on every call -- for the switches a tool changes inside one process.
inline int knob_now(const char *name, int dflt)
{
    const char *e = getenv(name);
    return e ? atoi(e) : dflt;
}
inline int knob_now(const char *name, int dflt, int lo, int hi)
{
    const int v = knob_now(name, dflt);
    return v < lo ? lo : v > hi ? hi : v;
}
// knob: a switch read ONCE per process.  The once is the caller's function-local static, which C++11 initialises exactly once under threads:
//     static const int use_ws = knob("HNR_H2LIN_WS", 1);
inline int knob(const char *name, int dflt) { return knob_now(name, dflt); }
inline int knob(const char *name, int dflt, int lo, int hi) { return knob_now(name, dflt, lo, hi); }

constexpr int MAX_DEVICES = 64;

// Per (kernel, device): the dynamic-LDS limit the kernel has been given, -1 = none yet.  raise(dev, bytes, set) returns 0 once the limit is at least
// `bytes`; it calls set(bytes) -- 0 = success, else an error code, which raise returns -- on the first use per device and whenever a call asks for more
// than was set.  The limit is recorded only after set succeeded (a failed set is tried again by the next call), and a second thread waits for the
// first one's set to return instead of launching beside it.  A device index outside 0..63 has no record: set runs every time.
class LdsLimit {
public:
    LdsLimit() { for (auto &b : bytes_) b.store(-1, std::memory_order_relaxed); }
    template <class Set> int raise(int dev, int bytes, Set &&set)
    {
        if (dev < 0 || dev >= MAX_DEVICES) return set(bytes);
        if (bytes_[dev].load(std::memory_order_acquire) >= bytes) return 0;
        std::lock_guard<std::mutex> lock(mu_);
        if (bytes_[dev].load(std::memory_order_relaxed) >= bytes) return 0;
        const int err = set(bytes);
        if (err == 0) bytes_[dev].store(bytes, std::memory_order_release);
        return err;
    }
    int limit(int dev) const { return dev < 0 || dev >= MAX_DEVICES ? -1 : bytes_[dev].load(std::memory_order_acquire); }

private:
    std::atomic<int> bytes_[MAX_DEVICES];
    std::mutex mu_;
};

// Per device: a positive number that is the same every time it is asked for (the CU count).  Two threads may both ask; they store the same value.
class PerDeviceValue {
public:
    template <class Query> int get(int dev, int fallback, Query &&query)
    {
        if (dev < 0 || dev >= MAX_DEVICES) return fallback;
        int v = v_[dev].load(std::memory_order_relaxed);
        if (v == 0) { v = query(dev); if (v <= 0) v = fallback; v_[dev].store(v, std::memory_order_relaxed); }
        return v;
    }

private:
    std::atomic<int> v_[MAX_DEVICES] = {};
};

}  // namespace hnr

#ifdef __HIPCC__
#include "hnr_common.h"

namespace hnr {

// CUs of the current device (256 when it cannot be asked): a process that renders on a second GPU must not reuse the first one's.
inline int device_num_cus()
{
    static PerDeviceValue n_cu;
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess) dev = -1;
    return n_cu.get(dev, 256, [](int d) {
        hipDeviceProp_t prop;
        return hipGetDeviceProperties(&prop, d) == hipSuccess ? prop.multiProcessorCount : 0;
    });
}

// Kernel<<<grid, block, lds_bytes, stream>>>(args...) for a kernel whose dynamic LDS may exceed 64 KB: the kernel's limit on the current device is
// raised to lds_bytes first (LdsLimit: once per kernel and device, again only if a later launch asks for more), so the limit and the launch cannot
// disagree.  HNR_OK, or HNR_ERR_HIP with the error text set.
template <auto Kernel, class... Args>
int launch_lds(dim3 grid, dim3 block, int lds_bytes, hipStream_t stream, const Args &...args)
{
    static LdsLimit limit;
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess) dev = -1;
    HNR_HIP_CHECK((hipError_t)limit.raise(dev, lds_bytes, [](int bytes) {
        return (int)hipFuncSetAttribute(reinterpret_cast<const void *>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    }));
    Kernel<<<grid, block, lds_bytes, stream>>>(args...);
    HNR_LAUNCH_CHECK();
    return HNR_OK;
}

}  // namespace hnr
#endif  // __HIPCC__
