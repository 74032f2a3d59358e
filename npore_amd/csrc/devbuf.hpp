// devbuf.hpp -- the one grow-only buffer of the HIP side: device memory, page-locked host memory, and page-locked memory
// that turns pageable where the runtime has none left.  A buffer is not copyable and frees itself; ensure() follows the
// convention of everything else here: NPORE_OK, or the code fail() returned (npore_last_error() has the words).
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/npore_amd.h"
#include "hostio.hpp"

#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess)                                                                      \
            return fail(NPORE_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));           \
    } while (0)

namespace npore {

// PinnedOrPageable: the staging of the BAM -> SAM pipeline (the buffers of a batch that cross PCIe), which does not fail
// where the runtime has no page-locked memory left: the buffer is pageable from then on.
enum class Mem { Device, Pinned, PinnedOrPageable };

template <Mem M>
struct GrowBuf {
    char *p = nullptr;
    size_t cap = 0;
    bool pinned = true;        // PinnedOrPageable: false once hipHostMalloc has failed, pageable (RawBuf::alloc) for the rest of its life
    GrowBuf() = default;
    GrowBuf(const GrowBuf &) = delete;
    GrowBuf &operator=(const GrowBuf &) = delete;
    ~GrowBuf() { release(); }
    void release()
    {
        if (!p) return;
        if (M == Mem::Device) (void)hipFree(p);
        else if (pinned) (void)hipHostFree(p);
        else std::free(p);
        p = nullptr;
        cap = 0;
    }
    // (the head-room: the groups and batches of a run differ a little in size)
    int ensure(size_t bytes)
    {
        if (bytes <= cap) return NPORE_OK;
        release();
        const size_t want = M == Mem::PinnedOrPageable ? bytes + bytes / 4 : bytes + bytes / 8 + 256;
        void *q = nullptr;
        if (M == Mem::Device) {
            AllocTrace tr("hipMalloc", want);
            const hipError_t e = hipMalloc(&q, want);
            if (e != hipSuccess) return fail(NPORE_E_NOMEM, "hipMalloc(" + std::to_string(want) + "): " + hipGetErrorString(e));
        } else if (pinned) {
            AllocTrace tr("hipHostMalloc", want);
            const hipError_t e = hipHostMalloc(&q, want, hipHostMallocDefault);
            if (e != hipSuccess && M == Mem::Pinned) return fail(NPORE_E_NOMEM, std::string("hipHostMalloc: ") + hipGetErrorString(e));
            if (e != hipSuccess) {
                (void)hipGetLastError();
                q = nullptr;
                pinned = false;
                if (std::getenv("NPORE_DEBUG")) std::fprintf(stderr, "npore: hipHostMalloc(%zu) failed, pageable staging buffer\n", want);
            }
        }
        if (!pinned) q = RawBuf::alloc(want);
        if (!q) return fail(NPORE_E_NOMEM, "batch buffers");
        p = static_cast<char *>(q);
        cap = want;
        return NPORE_OK;
    }
    // Device, best effort, no head-room: another buffer of the same role already has this capacity (WorkSet::presize_like)
    void match(const GrowBuf &o)
    {
        static_assert(M == Mem::Device, "match() is for device buffers");
        if (o.cap <= cap) return;
        release();
        AllocTrace tr("hipMalloc like", o.cap);
        void *q = nullptr;
        if (hipMalloc(&q, o.cap) == hipSuccess) { p = static_cast<char *>(q); cap = o.cap; }
        else (void)hipGetLastError();
    }
    template <class T> T *as() const { return reinterpret_cast<T *>(p); }
};

using DevBuf = GrowBuf<Mem::Device>;
using HostBuf = GrowBuf<Mem::Pinned>;
using PinnedBuf = GrowBuf<Mem::PinnedOrPageable>;

}  // namespace npore
