// What hint_householder.hip offers hint_householder_many.hip: the single op's limits and workspace size, and the launches of the
// batched op on the single op's device code.  Declarations only.
#pragma once
#include <cstddef>
#include <cstdint>
#include <hip/hip_runtime.h>

namespace hint {

struct HhLimits { int max_d, max_n, max_b; };
HhLimits hh_limits();
size_t hh_grad_workspace_bytes(int B, int d);           // a single grad run's workspace: one slot of the batched op
int hh_many_build(const float* Vs, int64_t vs_stride, float* W, int64_t w_stride, int m, int d, int n, hipStream_t s);
int hh_many_rows(const float* x, const float* g_y, const float* W, float* g_x, void* slot, int B, int d, hipStream_t s);
int hh_many_finish(void* ws, int64_t ws_stride, const float* W, int64_t w_stride, const float* Vs, int64_t vs_stride, float* g_W,
                   int64_t gw_stride, float* g_V, int64_t gv_stride, int m, int B, int d, int n, hipStream_t s);

}  // namespace hint
