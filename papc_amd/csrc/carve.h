// carve.h -- a caller-provided workspace is laid out once: a family's xx_layout(shape..., base, ptrs) walks its pieces with a WsCarver and
// returns `off`, the bytes carved.  papc_*_workspace() is that walk over a null base; the entry point takes its pointers, and the size it
// refuses a smaller workspace_bytes against, from the same walk over the caller's buffer.  (sa_mlp.hip's Carver with the alignment as a member.)
// A family whose caller's buffer may start anywhere walks WsCarver::over(base), the base rounded up to 256, and returns bytes().
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace papc {

struct WsCarver {      // hands out pieces of one buffer, each `align` bytes aligned from base; base == nullptr: sizes only
    char *base;
    size_t off, align = 256;
    static WsCarver over(void *base) { return WsCarver{reinterpret_cast<char *>((reinterpret_cast<uintptr_t>(base) + 255) & ~(uintptr_t)255), 0}; }
    template <class T> T *take(size_t n)
    {
        off = (off + align - 1) & ~(align - 1);
        T *p = base ? reinterpret_cast<T *>(base + off) : nullptr;
        off += n * sizeof(T);
        return p;
    }
    size_t bytes() const { return ((off + 255) & ~(size_t)255) + 256; }      // over()'s families: rounded up, plus the 256 the rounded base may eat
};

}  // namespace papc
