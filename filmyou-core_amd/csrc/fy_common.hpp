// fy_common.hpp -- context, stream-ordered HBM buffers, error plumbing shared by the HIP translation units.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <exception>
#include <memory>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "../../include/filmyou.h"
#include "fy_tuning.hpp"   // struct Tuning, ceil_div / round_up

namespace fy {

// ---------------------------------------------------------------- errors
void set_error(const char* fmt, ...);
const char* last_error();
void load_tuning_from_env(Tuning& t);   // fy_api.hip

struct Failure {
    int code;
};

#define FY_HIP(expr)                                                                               \
    do {                                                                                           \
        hipError_t _e = (expr);                                                                    \
        if (_e != hipSuccess) {                                                                    \
            fy::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
            throw fy::Failure{_e == hipErrorOutOfMemory ? FY_ERR_OUT_OF_MEMORY : FY_ERR_HIP};      \
        }                                                                                          \
    } while (0)

#define FY_FAIL(code, ...)            \
    do {                              \
        fy::set_error(__VA_ARGS__);   \
        throw fy::Failure{code};      \
    } while (0)

#define FY_KERNEL_CHECK() FY_HIP(hipGetLastError())

// ---------------------------------------------------------------- context
// One GPU, one stream, and a caching HBM allocator.  Every kernel and copy of a context runs on `stream`, so a block
// released by the host while work is still queued may be handed to a later allocation: the later user is ordered behind
// the earlier one by the stream (the semantics of hipFreeAsync, without the driver's pool: hipMallocAsync re-grew its
// pool at unpredictable steps and stalled whole jobs by 0.3-0.9 s when 14-16 GB buffers were split and re-requested).
// After the first job every request is served from the cache; fy_context_destroy returns the memory.
struct Context {
    int device = -1;
    hipStream_t stream = nullptr;
    int num_cus = 256;
    size_t lds_per_block = 160 * 1024;
    size_t total_mem = 0;
    std::vector<hipStream_t> aux;               // extra streams ("lanes") a multi-cluster job overlaps its clusters on
    std::multimap<size_t, void*> free_blocks;   // capacity -> block
    std::map<void*, size_t> capacity;            // every block ever handed out
    int64_t fail_alloc_in = 0;                   // fault injection (fy_context_inject_alloc_failure): the n-th request from now fails
    Tuning tune;                                 // launch-shape knobs, read from the environment when the context is created

    void* alloc(size_t bytes) {
        const size_t want = (bytes + 255) & ~size_t(255);
        if (fail_alloc_in > 0 && --fail_alloc_in == 0) {
            set_error("HBM allocation of %zu bytes failed: injected fault", want);
            throw Failure{FY_ERR_OUT_OF_MEMORY};
        }
        auto it = free_blocks.lower_bound(want);
        if (it != free_blocks.end() && it->first <= want + want / 4 + (1u << 20)) {
            void* p = it->second;
            free_blocks.erase(it);
            return p;
        }
        void* p = nullptr;
        hipError_t e = hipMalloc(&p, want);
        if (e != hipSuccess) {   // give cached blocks back to the driver and retry once
            (void)hipGetLastError();
            (void)hipStreamSynchronize(stream);
            trim();
            e = hipMalloc(&p, want);
        }
        if (e != hipSuccess) {
            (void)hipGetLastError();
            set_error("HBM allocation of %zu bytes failed: %s", want, hipGetErrorString(e));
            throw Failure{FY_ERR_OUT_OF_MEMORY};
        }
        capacity[p] = want;
        return p;
    }
    void release(void* p) {
        auto it = capacity.find(p);
        if (it != capacity.end()) free_blocks.emplace(it->second, p);
    }
    void trim() {   // the stream must be idle
        for (auto& kv : free_blocks) {
            (void)hipFree(kv.second);
            capacity.erase(kv.second);
        }
        free_blocks.clear();
    }
};

// ---------------------------------------------------------------- HBM buffer (stream-ordered alloc / free)
template <class T>
struct DevBuf {
    T* p = nullptr;
    size_t n = 0;
    Context* ctx = nullptr;
    DevBuf() = default;
    DevBuf(Context* c, size_t count) { alloc(c, count); }
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept { *this = std::move(o); }
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) {
            release();
            p = o.p; n = o.n; ctx = o.ctx;
            o.p = nullptr; o.n = 0;
        }
        return *this;
    }
    ~DevBuf() { release(); }
    void alloc(Context* c, size_t count) {
        release();
        ctx = c;
        n = count;
        size_t bytes = (count ? count : 1) * sizeof(T);
        p = static_cast<T*>(c->alloc(bytes));
    }
    void zero() { FY_HIP(hipMemsetAsync(p, 0, (n ? n : 1) * sizeof(T), ctx->stream)); }
    void release() {
        if (p) ctx->release(p);
        p = nullptr;
        n = 0;
    }
    T* get() const { return p; }
    size_t size() const { return n; }
    size_t bytes() const { return n * sizeof(T); }
};

template <class T>
inline void d2h(Context* c, T* dst, const T* src, size_t count) {
    if (count) FY_HIP(hipMemcpyAsync(dst, src, count * sizeof(T), hipMemcpyDeviceToHost, c->stream));
}
template <class T>
inline void h2d(Context* c, T* dst, const T* src, size_t count) {
    if (count) FY_HIP(hipMemcpyAsync(dst, src, count * sizeof(T), hipMemcpyHostToDevice, c->stream));
}
template <class T>
inline void d2d(Context* c, T* dst, const T* src, size_t count) {
    if (count) FY_HIP(hipMemcpyAsync(dst, src, count * sizeof(T), hipMemcpyDeviceToDevice, c->stream));
}
inline void sync(Context* c) { FY_HIP(hipStreamSynchronize(c->stream)); }

template <class T>
inline T fetch(Context* c, const T* src) {
    T v;
    d2h(c, &v, src, 1);
    sync(c);
    return v;
}

// ---------------------------------------------------------------- HIP-event phase timers on the context's stream
struct EventTimer {
    Context* ctx;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> spans;
    explicit EventTimer(Context* c) : ctx(c) {}
    ~EventTimer() {
        for (auto& s : spans) { (void)hipEventDestroy(s.first); (void)hipEventDestroy(s.second); }
    }
    // a span lives on ONE stream (default: the context's); spans of different lanes may overlap in time
    size_t begin(hipStream_t st = nullptr) {
        hipEvent_t a, b;
        FY_HIP(hipEventCreate(&a));
        FY_HIP(hipEventCreate(&b));
        FY_HIP(hipEventRecord(a, st ? st : ctx->stream));
        spans.emplace_back(a, b);
        return spans.size() - 1;
    }
    void end(size_t i, hipStream_t st = nullptr) { FY_HIP(hipEventRecord(spans[i].second, st ? st : ctx->stream)); }
    // total milliseconds over all spans; the stream must have been synchronised
    double total_ms() {
        double t = 0;
        for (auto& s : spans) {
            float ms = 0;
            if (hipEventElapsedTime(&ms, s.first, s.second) == hipSuccess) t += ms;
        }
        return t;
    }
    size_t count() const { return spans.size(); }
};

// Declared right AFTER the host-side sources (std::vector, stack arrays) of queued hipMemcpyAsync uploads: when an exception unwinds the
// scope, the stream is drained before those sources are destroyed (objects die in reverse order of declaration).  On the normal
// path the scope's own synchronisation has already happened and this does nothing.
struct SyncOnUnwind {
    hipStream_t st;
    int n0;
    explicit SyncOnUnwind(hipStream_t s) : st(s), n0(std::uncaught_exceptions()) {}
    ~SyncOnUnwind() {
        if (std::uncaught_exceptions() > n0) (void)hipStreamSynchronize(st);
    }
};

// ---------------------------------------------------------------- launch grids and the device helpers every translation unit uses
// workgroups of a grid-stride launch over n elements
inline int grid_for(int64_t n, int block = 256, int cap = 256 * 16) {
    int64_t g = ceil_div(n, block);
    return (int)std::max<int64_t>(1, std::min<int64_t>(g, cap));
}

// a ascending over [lo, hi): the first index whose element is not less than key (UPPER: is greater than key), hi when there is none
template <bool UPPER = false, class T, class K>
__device__ __forceinline__ int32_t fy_lower_bound(const T* a, int32_t lo, int32_t hi, K key) {
    while (lo < hi) {
        const int32_t mid = (lo + hi) >> 1;
        if (UPPER ? a[mid] <= key : a[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// 32-bit key that orders like the float (any sign, -0 < +0), and its inverse
__device__ __forceinline__ uint32_t fy_order_key(float f) {
    const uint32_t b = __float_as_uint(f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float fy_order_unkey(uint32_t k) {
    const uint32_t b = (k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k;
    return __uint_as_float(b);
}

// descending bitonic sort of P2 (power of two) 64-bit keys in LDS; every thread of the block calls it
__device__ __forceinline__ void fy_bitonic_desc(uint64_t* v, int P2) {
    for (int k = 2; k <= P2; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = threadIdx.x; i < P2; i += blockDim.x) {
                const int l = i ^ j;
                if (l > i) {
                    const uint64_t x = v[i], y = v[l];
                    const bool desc = (i & k) == 0;
                    if (desc ? (x < y) : (x > y)) { v[i] = y; v[l] = x; }
                }
            }
            __syncthreads();
        }
    }
}

}  // namespace fy

// ---------------------------------------------------------------- opaque ABI objects
struct fy_context {
    fy::Context c;
};

struct fy_ratings {
    fy::Context* ctx = nullptr;
    int64_t nnz = 0;
    fy::DevBuf<int32_t> user, item;
    fy::DevBuf<float> score;
    // largest user / item id over ALL entries (-1: none >= 0), found once when the ratings are put into HBM: the jobs pack
    // their sort keys into the bits these ids need
    int32_t max_user = -1, max_item = -1;
    // every score (of ANY entry; NaN aside) is exactly representable in fp16 -- half stars, integers: found in the same pass; the jobs
    // then carry the rating inside their 64-bit sort keys (fy_prep.hip, packed mode)
    bool scores_fp16_exact = false;
    // what the last RM2 job over these ratings built from them and its clustering alone (fy_rm2.hip: RM2Static): a later job
    // with the same clustering starts from it.  Released with the ratings (before their context), by fy_ratings_drop_cache, and
    // by a caching job whose clustering / share does not match it (BEFORE that job builds its own: never two static sets in HBM).
    // The pointer is read and written under cache_mu; the jobs themselves are single-threaded per ratings object (include/filmyou.h).
    mutable std::shared_ptr<void> rm2_cache;
    mutable std::mutex cache_mu;
};
