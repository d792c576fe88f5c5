// Stand-in for tbb/blocked_range.h (test infrastructure, oracle/ref/Makefile):
// the half-open range the reference hands to parallel_for, nothing else.
#pragma once
#include <cstddef>

namespace tbb {

template <typename Value>
class blocked_range {
public:
    blocked_range(Value begin, Value end, std::size_t grain = 1) : m_begin(begin), m_end(end), m_grain(grain) {}
    Value begin() const { return m_begin; }
    Value end() const { return m_end; }
    std::size_t grainsize() const { return m_grain; }

private:
    Value m_begin, m_end;
    std::size_t m_grain;
};

}  // namespace tbb
