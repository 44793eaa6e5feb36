// common.hpp -- error handling and device buffers for the Katana HIP engine.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <utility>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/katana_hip.h"
#include "error.hpp"

namespace ktn {

#define KTN_HIP(expr)                                                                         \
    do {                                                                                       \
        hipError_t e__ = (expr);                                                               \
        if (e__ != hipSuccess) {                                                               \
            throw ::ktn::Error(e__ == hipErrorOutOfMemory ? KTN_E_NOMEM : KTN_E_HIP,          \
                               std::string(#expr) + ": " + hipGetErrorString(e__) + " (" +    \
                                   __FILE__ + ":" + std::to_string(__LINE__) + ")");          \
        }                                                                                      \
    } while (0)

// KTN_POISON (development switch, DevParams in engine.hpp; DESIGN.md "Reproducibility"): every NEW allocation of DBuf::reserve is
// filled over its whole capacity before the old contents are copied in, so that a kernel that reads an element nobody wrote reads
// the same thing in every run -- and, under `nan`, something that shows in the numbers.  mode 1 (`zero`): all bytes 0.  mode 2
// (`nan`): buffers of floating-point element type get a quiet NaN in every element (all bytes 0xFF is one, for float and for
// double), buffers of EVERY integer element type -- and of structs, which may hold indices -- get 0.  Integer buffers are never
// filled with anything but 0, under either value: an uninitialised index must not become an out-of-range address.  The switch
// exists to turn a silent wrong read into a changed number, never to make anything fault.
// The state belongs to a handle; the ABI layer names the handle whose call is running on this thread (PoisonScope), because a
// DBuf does not know its engine.  Unset: no state is named or its mode is 0, and reserve() makes the calls it always made.
// The limit of that: an allocation made while no scope is open -- an entry point of the C ABI that does not go through KTN_TRY,
// a thread of the caller's that the engine did not enter through the ABI -- is not filled and raises no error, and
// `poison_fills > 0` does not notice a partial miss.  Every entry point that allocates goes through KTN_TRY today.
struct PoisonState {
    int mode = 0;         // 0 off, 1 zero, 2 nan
    int64_t fills = 0;    // allocations filled (stat "poison_fills")
};
inline PoisonState*& poison_current() {
    static thread_local PoisonState* cur = nullptr;
    return cur;
}
struct PoisonScope {
    PoisonState* prev;
    explicit PoisonScope(PoisonState* p) : prev(poison_current()) { poison_current() = p; }
    ~PoisonScope() { poison_current() = prev; }
    PoisonScope(const PoisonScope&) = delete;
    PoisonScope& operator=(const PoisonScope&) = delete;
};
template <typename T> struct poison_float : std::false_type {};
template <> struct poison_float<float> : std::true_type {};
template <> struct poison_float<double> : std::true_type {};
template <> struct poison_float<float2> : std::true_type {};
template <> struct poison_float<double2> : std::true_type {};

// Growable device array.  resize() keeps the first min(old,new) elements.
template <typename T>
struct DBuf {
    T* p = nullptr;
    size_t n = 0;    // logical size
    size_t cap = 0;  // allocated elements

    DBuf() = default;
    DBuf(const DBuf&) = delete;
    DBuf& operator=(const DBuf&) = delete;
    ~DBuf() { release(); }

    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        n = cap = 0;
    }
    void reserve(size_t want, hipStream_t s) {
        if (want <= cap) return;
        size_t ncap = cap ? cap : 256;
        while (ncap < want) ncap += ncap / 2 + 256;
        T* q = nullptr;
        KTN_HIP(hipMalloc(&q, ncap * sizeof(T)));
        if (PoisonState* ps = poison_current(); ps && ps->mode) {
            const hipError_t e = hipMemsetAsync(q, (ps->mode == 2 && poison_float<T>::value) ? 0xFF : 0, ncap * sizeof(T), s);
            if (e != hipSuccess) (void)hipFree(q);
            KTN_HIP(e);
            ++ps->fills;
        }
        if (p && n) KTN_HIP(hipMemcpyAsync(q, p, n * sizeof(T), hipMemcpyDeviceToDevice, s));
        if (p) {
            KTN_HIP(hipStreamSynchronize(s));
            (void)hipFree(p);
        }
        p = q;
        cap = ncap;
    }
    void resize(size_t want, hipStream_t s) {
        reserve(want, s);
        n = want;
    }
    void swap(DBuf& o) {
        std::swap(p, o.p);
        std::swap(n, o.n);
        std::swap(cap, o.cap);
    }
    void zero(hipStream_t s) {
        if (n) KTN_HIP(hipMemsetAsync(p, 0, n * sizeof(T), s));
    }
    void upload(const T* host, size_t count, hipStream_t s) {
        resize(count, s);
        if (count) KTN_HIP(hipMemcpyAsync(p, host, count * sizeof(T), hipMemcpyHostToDevice, s));
    }
    void upload(const std::vector<T>& v, hipStream_t s) { upload(v.data(), v.size(), s); }
    void download(T* host, size_t count, hipStream_t s) const {
        if (count) KTN_HIP(hipMemcpyAsync(host, p, count * sizeof(T), hipMemcpyDeviceToHost, s));
        KTN_HIP(hipStreamSynchronize(s));
    }
    std::vector<T> to_host(hipStream_t s) const {
        std::vector<T> v(n);
        download(v.data(), n, s);
        return v;
    }
};

inline int ceil_div(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }

}  // namespace ktn
