// device_buf.h -- the grow-only buffer record of the encoder's and the decoder's host side.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>

namespace lacx {

// A failing HIP call, by name.
struct DevErr {
    const char* what = "";
    hipError_t e = hipSuccess;
    explicit operator bool() const { return e != hipSuccess; }
};
inline DevErr chk(hipError_t e, const char* what) { return DevErr{what, e}; }

// Up to three allocations that share one grow-only capacity, counted in elements: device or pinned, each with its element
// size and the name a failing allocation is reported under.
struct Buf {
    struct Part {
        bool pinned;
        uint32_t elem;  // 0: unused
        const char* what;
        void* p = nullptr;
    } part[3];
    uint64_t cap = 0;
    template <class T>
    T* as(int i = 0) const { return static_cast<T*>(part[i].p); }
};
inline void buf_free(Buf& b) {
    for (Buf::Part& x : b.part) {
        if (x.p) (void)(x.pinned ? hipHostFree(x.p) : hipFree(x.p));
        x.p = nullptr;
    }
    b.cap = 0;
}
// need elements, or need + slack where it has to grow (or a part is missing)
inline DevErr buf_grow(Buf& b, uint64_t need, uint64_t slack) {
    bool have = need <= b.cap;
    for (const Buf::Part& x : b.part) have = have && (x.p || !x.elem);
    if (have) return DevErr{};
    buf_free(b);
    for (Buf::Part& x : b.part) {
        if (!x.elem) continue;
        const size_t bytes = (size_t)(need + slack) * x.elem;
        if (DevErr e = chk(x.pinned ? hipHostMalloc(&x.p, bytes, 0) : hipMalloc(&x.p, bytes), x.what)) return e;
    }
    b.cap = need + slack;
    return DevErr{};
}

}  // namespace lacx
