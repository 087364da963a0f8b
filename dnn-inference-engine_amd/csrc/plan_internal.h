// Host-side pieces plan.hip and host_ops.hip share (no device code, not part of the ABI).
#pragma once
#include <cstddef>

namespace dnnhip {

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// the checks dnn_plan_add_spp and dnn_spp_host make of their window sizes (0, or -2 with the error set)
int spp_sizes_ok(const char* who, int n_sizes, const int* sizes);

}  // namespace dnnhip
