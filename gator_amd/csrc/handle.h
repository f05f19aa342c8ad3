// What a handle of the auxiliary libraries (gator_renderer, gator_draw2d, gator_smpl) is, stated once: the device it lives on, the
// accounting of its workspace with the one growth rule, the staged host-to-device table, create / destroy, and the checks every entry
// point starts with.  Host code only (DESIGN.md "Handles of the auxiliary libraries").
#pragma once
#include <vector>

#include "image_groups.h"
#include "internal.h"

namespace gator {

// A workspace buffer with the element count it holds; cap is 0 whenever the block is not there.
template <class T, bool Pinned = false> struct WorkBuf : DevBuf<T, Pinned> { size_t cap = 0; };

// A table made on the host at create: the device block (one element when the table is empty) and its blocking copy.
template <class T> int upload(DevBuf<T>& d, const std::vector<T>& h) {
    GATOR_TRY(d.alloc(sizeof(T) * (h.empty() ? 1 : h.size())));
    if (!h.empty()) GATOR_HIP_CHECK(hipMemcpy(d.get(), h.data(), sizeof(T) * h.size(), hipMemcpyHostToDevice));
    return GATOR_OK;
}

struct Handle {
    int device = 0;
    int64_t bytes = 0, allocations = 0;      // held by the grown buffers now; growths since create (gator_*_workspace)
    // The growth rule, `need` in elements of T.  A call that grows nothing synchronises nothing (it may be under graph capture); queued
    // work may still read a block that is replaced, so only then the device is waited for.  alloc() frees the old block before it asks
    // for the new one, so the capacity is 0 from that moment until the new block is there: a failed growth leaves an empty buffer that
    // the next call grows again, never a capacity without a block behind it.
    template <class T, bool Pinned> int grow(WorkBuf<T, Pinned>& buf, size_t need) {
        if (need <= buf.cap) return GATOR_OK;
        if (buf.cap) GATOR_HIP_CHECK(hipDeviceSynchronize());
        bytes -= (int64_t)(buf.cap * sizeof(T));
        buf.cap = 0;
        GATOR_TRY(buf.alloc(need * sizeof(T)));
        bytes += (int64_t)(need * sizeof(T));
        allocations += 1;
        buf.cap = need;
        return GATOR_OK;
    }
};

// Every entry point's first check: there is a handle, and it lives on the current device.  what: "handle", or "ctx" for gator_smpl.
inline int check_handle(const Handle* h, const char* who, const char* what = "handle") {
    if (!h) return fail(GATOR_EINVAL, "%s: null %s", who, what);
    int dev = 0;
    GATOR_HIP_CHECK(hipGetDevice(&dev));
    if (dev != h->device) return fail(GATOR_EINVAL, "%s: the %s lives on device %d, the current device is %d", who, what, h->device, dev);
    return GATOR_OK;
}

inline int handle_workspace(const Handle* h, const char* who, int64_t* bytes, int64_t* allocations) {
    if (!h) return fail(GATOR_EINVAL, "%s: null handle", who);
    if (bytes) *bytes = h->bytes;
    if (allocations) *allocations = h->allocations;
    return GATOR_OK;
}

// new, build(h) on the current device, delete on failure
template <class H, class Build> int create_handle(H** out, Build build) {
    H* h = new H;
    const hipError_t e = hipGetDevice(&h->device);
    const int rc = e == hipSuccess ? build(h) : fail(GATOR_EHIP, "no HIP device available: %s", hipGetErrorString(e));
    if (rc != GATOR_OK) { delete h; return rc; }
    *out = h;
    return GATOR_OK;
}

template <class H> int destroy_handle(H* h) {
    if (!h) return GATOR_OK;
    (void)hipDeviceSynchronize();      // queued work may still use the handle's buffers
    delete h;
    return GATOR_OK;
}

// A table built on the host per call and read by that call's kernels: pinned staging, the device block, and an event recorded behind
// the staging's copy, which the next call waits for before it rewrites the staging.
template <class T>
struct StagedTable {
    WorkBuf<T, true> host;
    WorkBuf<T> dev;
    hipEvent_t copied = nullptr;
    ~StagedTable() { if (copied) (void)hipEventDestroy(copied); }
    int stage(Handle* h, size_t count, T** out) {      // -> the staging, free to be written
        if (!copied) GATOR_HIP_CHECK(hipEventCreateWithFlags(&copied, hipEventDisableTiming));
        GATOR_HIP_CHECK(hipEventSynchronize(copied));
        GATOR_TRY(h->grow(host, count));
        *out = host.get();
        return GATOR_OK;
    }
    int upload(Handle* h, size_t count, hipStream_t st, const T** out) {      // -> the device copy, valid behind this point of the stream
        GATOR_TRY(h->grow(dev, count));
        GATOR_HIP_CHECK(hipMemcpyAsync(dev.get(), host.get(), count * sizeof(T), hipMemcpyHostToDevice, st));
        GATOR_HIP_CHECK(hipEventRecord(copied, st));
        *out = dev.get();
        return GATOR_OK;
    }
};

// A versioned argument struct: `given` is its struct_size field.  accept_larger: a caller built against a later, longer struct is served.
inline int check_struct_size(const char* who, const char* what, int32_t given, size_t expected, bool accept_larger = false) {
    if (given == (int32_t)expected || (accept_larger && given > (int32_t)expected)) return GATOR_OK;
    return fail(GATOR_EINVAL, "%s: struct_size %d, this library's %s has %d bytes", who, given, what, (int)expected);
}

}  // namespace gator
