// What every unit that reads or writes a fitted leaf-space posterior agrees on (included from common.h): how areas are carved
// out of a buffer, the layout of the state, and the limits that the stateless driver (leafsystem.hip) and the driver of the
// calls on a state (fitted.hip) both check.  Plain host C++ with no HIP in it, so a host-only program can include it alone.
#pragma once
#include <cstddef>
#include <cstdint>

namespace bark {

inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }  // workspace areas start on 256-byte boundaries

// 256-byte aligned areas handed out front to back; base == nullptr: sizes only
struct Carve {
    char *base;
    size_t o = 0;
    template <class T> T *take(size_t n) {
        T *p = base ? reinterpret_cast<T *>(base + o) : nullptr;
        o = align256(o + n * sizeof(T));
        return p;
    }
};

constexpr int ACQ_MAX_TREES = 64;      // trees per forest that the scan, score and conditioning kernels (acquire.hip) stage in LDS
constexpr int64_t ACQ_SLAB = 1 << 16;  // candidates walked and scanned per launch pair: bounds the code buffer (Bc, W, slab)
constexpr int64_t ACQ_MAX_PENDING = 64, ACQ_MAX_SKIP = 64, ACQ_MAX_TARGETS = 1024;

// body(s0, n) for the slabs of C candidates, n <= ACQ_SLAB of them from s0 on, until one fails
template <class F> int for_slabs(int64_t C, F &&body) {
    for (int64_t s0 = 0; s0 < C; s0 += ACQ_SLAB) {
        const int rc = body(s0, C - s0 < ACQ_SLAB ? C - s0 : ACQ_SLAB);
        if (rc) return rc;
    }
    return 0;
}

// A fitted posterior in a buffer of the caller's: M^-1 (B, R, R), w (B, R), then the sweep's status per forest, each area
// 256-byte aligned.  bark_leaf_posterior_bytes and every entry point that takes a state get sizes and pointers here.
// base == nullptr: sizes only.  (The Python front end reads the status words by the same arithmetic: LeafPosterior.info.)
struct PosteriorState {
    double *Minv, *w;
    int32_t *info;
    size_t total;
};
inline PosteriorState posterior_state(void *base, int64_t R, int64_t B) {
    Carve cv{static_cast<char *>(base)};
    PosteriorState st;
    st.Minv = cv.take<double>((size_t)B * R * R);
    st.w = cv.take<double>((size_t)B * R);
    st.info = cv.take<int32_t>((size_t)B);
    st.total = cv.o;
    return st;
}
inline bool posterior_shape_ok(int64_t R, int64_t m, int64_t B) { return R >= 1 && R <= 8192 && m >= 1 && m <= ACQ_MAX_TREES && B >= 1; }

}  // namespace bark
