// The bump allocator the entry points carve their workspaces with (handle.hpp: carve()); on its
// own so that a kernel file can lay out its workspace without the rest of the handle.
#pragma once
#include <stddef.h>

namespace pbbss {
// Bump allocator over a slab (256-byte aligned pieces).  Without a base it only measures: take()
// counts the bytes and hands out null.
struct Carver {
  char* base;
  size_t off = 0;
  explicit Carver(void* b = nullptr) : base(static_cast<char*>(b)) {}
  template <typename T>
  T* take(size_t count) {
    T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
    off += (count * sizeof(T) + 255) & ~(size_t)255;
    return p;
  }
};
}  // namespace pbbss
