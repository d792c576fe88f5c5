// Stand-in for tbb/parallel_for.h: the body runs once over the whole range, on
// the calling thread.  Each image row seeds its own RNG, so the frame does not
// depend on how the rows are split among threads.
#pragma once
#include "blocked_range.h"

namespace tbb {

template <typename Range, typename Body>
void parallel_for(const Range& range, const Body& body)
{
    body(range);
}

}  // namespace tbb
