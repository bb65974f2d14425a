// profile.h - per-family launch timing of the executor (HIP events on the launch stream; icd_profile_enable / _read / _dump).
// The records, the event pool and the switches live in profile.hip and nowhere else.
#pragma once
#include "common.h"

// One timed launch: records an event on `st` at construction and at destruction when profiling is on and family `kind` is selected;
// otherwise it does nothing.  flops: the algorithmic count of the operator as the reference computes it.
struct __attribute__((visibility("hidden"))) ProfScope {
    ProfScope(hipStream_t st, int kind, double flops, double bytes, int M = 0, int N = 0, int K = 0, int aux = 0);
    ~ProfScope();
    ProfScope(const ProfScope&) = delete;
    void executed(double xflops);           // flops issued to the matrix cores when they differ from the algorithmic count
    void plan(const icd_gemm_desc& d);      // which tile the planner takes for this launch (tests assert the code path)
private:
    bool on; hipStream_t st; size_t idx;
};
