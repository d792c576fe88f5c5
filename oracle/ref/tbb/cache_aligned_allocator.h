// Stand-in for tbb/cache_aligned_allocator.h: std::allocator under TBB's name
// (alignment changes no arithmetic).
#pragma once
#include <memory>

namespace tbb {

template <typename T>
class cache_aligned_allocator : public std::allocator<T> {
public:
    cache_aligned_allocator() = default;
    template <typename U>
    cache_aligned_allocator(const cache_aligned_allocator<U>&) {}
    template <typename U>
    struct rebind { using other = cache_aligned_allocator<U>; };
};

}  // namespace tbb
