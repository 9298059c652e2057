// The bump allocator the workspace layouts are written with.  A layout's size is the layout run on a null base, so the two cannot disagree.
#pragma once
#include "common.h"

namespace mnf {

struct Carver {
    char *base;          // NULL: size only, every take() returns NULL
    size_t off = 0;
    explicit Carver(void *b) : base(static_cast<char *>(b)) {}
    template <typename T = char>
    T *take(size_t count) {      // `count` elements of T on the next 256-byte granule
        char *p = base ? base + off : nullptr;
        off += (count * sizeof(T) + 255) & ~(size_t)255;
        return reinterpret_cast<T *>(p);
    }
    int64_t bytes() const { return (int64_t)off; }
};

inline int check_workspace(const char *who, const void *workspace, int64_t have, int64_t need) {
    if (!workspace || have < need) { set_error("%s: workspace too small (%lld < %lld bytes)", who, (long long)have, (long long)need); return MNF_ERR_WORKSPACE; }
    return MNF_OK;
}

}  // namespace mnf
