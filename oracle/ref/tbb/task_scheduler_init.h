// Stand-in for tbb/task_scheduler_init.h: one thread, nothing to set up.
#pragma once

namespace tbb {

class task_scheduler_init {
public:
    explicit task_scheduler_init(int = 1) {}
    static int default_num_threads() { return 1; }
};

}  // namespace tbb
