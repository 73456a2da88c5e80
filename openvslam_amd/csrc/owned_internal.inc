// owned_internal.inc -- the one owner of HIP resources on the host side of the C ABI. A handle (or a per-thread work space) acquires its
// device memory, page-locked memory, streams and events through its Owned member; ~Owned gives back exactly those, on every exit path, so a
// create needs no clean-up branch and a destroy no list. (An .inc, not an .h: bench.py fingerprints every .h of this directory into the
// committed counters of the extractor and matcher stages, which host-only code should not age.)
#pragma once
#include <atomic>
#include <cstdint>
#include <utility>
#include <vector>

#include <hip/hip_runtime.h>

#include "ovs_common.h"

namespace ovs {

// resources recorded by any Owned and not yet released, process-wide (ovs_debug_live_resources)
inline std::atomic<int64_t> g_live_resources{0};

// Every acquiring method returns the raw HIP error and records the resource whenever the out-pointer came back non-null -- whatever the
// caller then makes of the error (fault_filter may turn a success into a failure; the resource exists all the same). Owned knows nothing
// of devices: whoever releases on another device than the current one sets it first.
class Owned {
public:
    Owned() = default;
    Owned(const Owned&) = delete;
    Owned& operator=(const Owned&) = delete;
    Owned(Owned&& o) noexcept : items_(std::move(o.items_)) { o.items_.clear(); }   // (a std::vector of owners may grow)
    ~Owned() { clear(); }

    template <class T>
    hipError_t dev(T** p, size_t bytes) {
        *p = nullptr;
        const hipError_t e = hipMalloc(reinterpret_cast<void**>(p), bytes);
        record(*p, kDev);
        return e;
    }
    template <class T>
    hipError_t pinned(T** p, size_t bytes, unsigned flags = hipHostMallocDefault) {
        *p = nullptr;
        const hipError_t e = hipHostMalloc(reinterpret_cast<void**>(p), bytes, flags);
        record(*p, kPinned);
        return e;
    }
    hipError_t stream(hipStream_t* s) {
        *s = nullptr;
        const hipError_t e = hipStreamCreateWithFlags(s, hipStreamNonBlocking);
        record(*s, kStream);
        return e;
    }
    hipError_t event(hipEvent_t* ev, unsigned flags) {
        *ev = nullptr;
        const hipError_t e = hipEventCreateWithFlags(ev, flags);
        record(*ev, kEvent);
        return e;
    }

    // releases one resource now and nulls it (a buffer about to be regrown, a stream of another device); returns what the release reported
    template <class T>
    hipError_t drop(T** p) {
        hipError_t e = hipSuccess;
        for (size_t i = items_.size(); i-- > 0;)
            if (items_[i].p == static_cast<void*>(*p)) {
                e = release(items_[i]);
                items_.erase(items_.begin() + (long)i);
                break;
            }
        *p = nullptr;
        return e;
    }

    // every owned stream drained, then everything released, the latest acquisition first
    void clear() {
        for (const Item& it : items_)
            if (it.kind == kStream) (void)hipStreamSynchronize(static_cast<hipStream_t>(it.p));
        while (!items_.empty()) {
            (void)release(items_.back());
            items_.pop_back();
        }
    }

private:
    enum Kind : uint8_t { kDev, kPinned, kStream, kEvent };
    struct Item {
        void* p;
        Kind kind;
    };
    std::vector<Item> items_;

    void record(void* p, Kind kind) {
        if (!p) return;
        items_.push_back(Item{p, kind});
        g_live_resources.fetch_add(1, std::memory_order_relaxed);
    }
    static hipError_t release(const Item& it) {
        g_live_resources.fetch_sub(1, std::memory_order_relaxed);
        switch (it.kind) {
        case kDev: return hipFree(it.p);
        case kPinned: return hipHostFree(it.p);
        case kStream: return hipStreamDestroy(static_cast<hipStream_t>(it.p));
        default: return hipEventDestroy(static_cast<hipEvent_t>(it.p));
        }
    }
};

}   // namespace ovs

// OVS_HIP_TRY without fault_filter: the creates whose calls the injection tests do not count
#define OVS_HIP_TRY_RAW(expr)                  \
    do {                                       \
        hipError_t _e = (expr);                \
        if (_e != hipSuccess) {                \
            ovs::set_last_error(#expr, _e);    \
            return OVS_ERR_HIP;                \
        }                                      \
    } while (0)
