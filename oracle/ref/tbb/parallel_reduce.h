// Stand-in for tbb/parallel_reduce.h: included by the reference, never called.
#pragma once
