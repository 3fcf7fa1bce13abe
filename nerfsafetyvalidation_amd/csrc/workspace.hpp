// workspace.hpp -- caller-owned scratch memory: one way to bump, align and refuse.  Every entry point that takes a workspace has ONE
// layout function, `static FooWs foo_layout(Carver&, dims...)`, which its ngp_foo_workspace() runs over a measuring Carver (no base)
// and the entry point, after check_workspace(), over the caller's pointer -- so the size reported and the bytes touched come from
// the same lines.  (A layout may be one braced initialiser in field order: its takes are evaluated left to right.)  The two behaviours
// a caller sees are in include/ngp_hip.h, "Caller-owned workspaces": too small is NGP_EWORKSPACE from every such entry point (four of
// them said NGP_EINVAL before ABI 102), and ngp_mark_untrained_grid has a size function of its own.
// Host only and free of HIP headers: tests/test_workspace_cpu.py builds it with a plain C++ compiler.
#ifndef NGP_WORKSPACE_HPP
#define NGP_WORKSPACE_HPP
#include <stddef.h>
#include <stdint.h>

#include "../../include/ngp_hip.h"

namespace ngp {

void set_error(const char* fmt, ...);      // capi.hip

// Bump allocator over `base`; nullptr measures.  Offsets are size_t and saturate at SIZE_MAX, which no buffer satisfies.
class Carver {
public:
    explicit Carver(void* base = nullptr) : base_(static_cast<char*>(base)) {}

    // `count` objects of T at the next multiple of `align` (a power of two; relative to the base, which check_workspace() aligns)
    template <typename T>
    T* take(size_t count, size_t align = alignof(T)) {
        off_ = off_ > SIZE_MAX - (align - 1) ? SIZE_MAX : (off_ + align - 1) & ~(align - 1);
        T* p = base_ ? reinterpret_cast<T*>(base_ + off_) : nullptr;
        pad(count > SIZE_MAX / sizeof(T) ? SIZE_MAX : count * sizeof(T));
        return p;
    }
    // slack that belongs to no region; every call site says who uses it
    void pad(size_t bytes) { off_ = bytes > SIZE_MAX - off_ ? SIZE_MAX : off_ + bytes; }
    size_t bytes() const { return off_; }

private:
    char* base_;
    size_t off_ = 0;
};

// The one refusal.  Nothing needed: NGP_OK whatever was given.  Fewer bytes than needed (a NULL workspace of 0 bytes included):
// NGP_EWORKSPACE, the message naming both sizes.  Enough bytes claimed behind a NULL pointer or one not `align`-byte aligned: NGP_EINVAL.
inline int check_workspace(const char* what, const void* workspace, size_t given, size_t need, size_t align) {
    if (need == 0) return NGP_OK;
    if (given < need) {
        set_error("%s: workspace too small (%zu < %zu bytes)", what, given, need);
        return NGP_EWORKSPACE;
    }
    if (!workspace || ((uintptr_t)workspace & (align - 1))) {
        set_error("%s: workspace is NULL or not %zu-byte aligned", what, align);
        return NGP_EINVAL;
    }
    return NGP_OK;
}

}  // namespace ngp
#endif
