// The bump allocator the workspace layouts are written with.  A layout's size is the layout run on a null base, so the two cannot disagree.
#pragma once
#include "common.h"

namespace mnf {

struct Carver {
    char *base;          // NULL: size only, every take() returns NULL
    size_t granule;      // a power of two; the base is aligned to it by the caller (the map units carve at 8)
    size_t off = 0;
    explicit Carver(void *b, size_t g = 256) : base(static_cast<char *>(b)), granule(g) {}
    template <typename T = char>
    T *take(size_t count) {      // `count` elements of T on the next granule
        char *p = base ? base + off : nullptr;
        off += (count * sizeof(T) + granule - 1) & ~(granule - 1);
        return reinterpret_cast<T *>(p);
    }
    int64_t bytes() const { return (int64_t)off; }
};

// bytes of mnf_exclusive_scan_i64's own workspace for a scan of n elements (a scan of none still takes one's)
inline int64_t scan_bytes(int64_t n) { return mnf_scan_workspace_bytes(n > 0 ? n : 1); }

inline int check_workspace(const char *who, const void *workspace, int64_t have, int64_t need) {
    if (!workspace || have < need) { set_error("%s: workspace too small (%lld < %lld bytes)", who, (long long)have, (long long)need); return MNF_ERR_WORKSPACE; }
    return MNF_OK;
}

}  // namespace mnf
