// carve.h -- a caller-provided workspace is laid out once: a family's xx_layout(shape..., base, ptrs) walks its pieces with a WsCarver and
// returns `off`, the bytes carved.  papc_*_workspace() is that walk over a null base; the entry point takes its pointers, and the size it
// refuses a smaller workspace_bytes against, from the same walk over the caller's buffer.  (sa_mlp.hip's Carver with the alignment as a member.)
#pragma once
#include <stddef.h>

namespace papc {

struct WsCarver {      // hands out pieces of one buffer, each `align` bytes aligned from base; base == nullptr: sizes only
    char *base;
    size_t off, align = 256;
    template <class T> T *take(size_t n)
    {
        off = (off + align - 1) & ~(align - 1);
        T *p = base ? reinterpret_cast<T *>(base + off) : nullptr;
        off += n * sizeof(T);
        return p;
    }
};

}  // namespace papc
