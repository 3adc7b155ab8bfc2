// task_rows.hpp — what the task layers of the three-launch tasks share (reach_task.hpp, anymal_task.hpp, amp_task.hpp,
// quadcopter_task.hpp): the reset draw, torch_rand_float, row staging between memory and LDS, and the
// VecTask.step tail of a *_post kernel.  Every caller runs blocks of one 64-lane wave; how lanes map to envs is
// each task's own business, and nothing below knows which task calls it.  Included by those four headers only: the
// step kernels' translation units (inst.hip) never see it.  fp32 with FMA contraction off, as task.hpp.
#pragma once
#include "../../include/migym.h"
#include "device_math.hpp"
#include "task.hpp"

namespace mgt {

constexpr int kLanes = 64;   // lanes per block

#pragma clang fp contract(off)

// draw `col` of env e: its row of the (N, width) injected noise tensor, or the counter RNG keyed by the global env id
__device__ __forceinline__ float noise_draw(const mg_task_buffers& tb, int e, int col, int width) {
  return tb.noise ? tb.noise[(size_t)width * e + col]
                  : mg::uniform01(tb.seed, (uint64_t)(tb.env_offset + e), tb.step_counter, (uint32_t)col);
}

// torch_rand_float(lower, upper): (upper - lower) * u + lower, the span a Python float
__device__ __forceinline__ float rand_float(float span, float lo, float u) { return span * u + lo; }

// the block's `rows` rows of `w` floats of a tensor, between memory and LDS, over consecutive addresses
__device__ __forceinline__ void rows_load(float* s, const float* g, int rows, int w) {
  for (int i = threadIdx.x; i < rows * w; i += kLanes) s[i] = g[i];
}
__device__ __forceinline__ void rows_store(float* g, const float* s, int rows, int w) {
  for (int i = threadIdx.x; i < rows * w; i += kLanes) g[i] = s[i];
}

// the per-row outputs of VecTask.step; time_out is the caller's own comparison
__device__ __forceinline__ void tail_store(const mg_task_buffers& tb, int row, float rew, long long reset,
                                           long long progress, bool time_out) {
  tb.rew[row] = rew;
  tb.reset[row] = reset;
  tb.progress[row] = progress;
  tb.timeout[row] = (uint8_t)(time_out && reset != 0);
}

// The block's rows leave LDS as one contiguous range of the output tensors: s_obs holds `rows` packed rows of `no`
// floats, s_rew / s_rst one reward and one reset flag per packed row; row0 is the block's first output row.  Writes
// obs, obs_clamped if bound, and the gather's message rows [clamped obs | rew | reset] if bound.  Call after a
// __syncthreads(); with a constant `no` the row / column split is a constant division.
__device__ __forceinline__ void block_tail(const mg_task_buffers& tb, const float* s_obs, const float* s_rew,
                                           const float* s_rst, size_t row0, int rows, int no, float clip_obs) {
  for (int i = threadIdx.x; i < rows * no; i += kLanes) {
    const float x = s_obs[i];
    tb.obs[row0 * no + i] = x;
    if (tb.obs_clamped) tb.obs_clamped[row0 * no + i] = mg::clampf(x, clip_obs);
  }
  if (tb.out_pack) {
    const int w = no + 2;
    for (int i = threadIdx.x; i < rows * w; i += kLanes) {
      const int r = i / w, c = i - r * w;
      const float x = c < no ? mg::clampf(s_obs[r * no + c], clip_obs) : (c == no ? s_rew[r] : s_rst[r]);
      tb.out_pack[row0 * w + i] = x;
    }
  }
}

#pragma clang fp contract(fast)

}  // namespace mgt
