// Stand-in for tbb/scalable_allocator.h: std::allocator under TBB's name.
#pragma once
#include <memory>

namespace tbb {

template <typename T>
class scalable_allocator : public std::allocator<T> {
public:
    scalable_allocator() = default;
    template <typename U>
    scalable_allocator(const scalable_allocator<U>&) {}
    template <typename U>
    struct rebind { using other = scalable_allocator<U>; };
};

}  // namespace tbb
