// The stand-alone network kernel's template, shared by its two units: net.hip instantiates the float32 mode,
// net_bf16.hip the plain-bf16 mode.  (Two units: the float32 kernels' code is then the same whether or not the other
// mode's kernels exist -- the compiler's output for one kernel shifts with what else its module holds.)
#pragma once
#include "net_dev.hpp"

namespace nz {
namespace {

// x as the plain-bf16 mode holds it: rounded to nearest even, widened again
__device__ __forceinline__ float bf16_round(float x) { return bf16_lo(pack_rne16(x, 0.0f)); }

// PREC: the arithmetic mode (net_dev.hpp); `W` and `prog` are that mode's.  Plain-bf16 rounds the raw input planes here,
// where the kernel reads them.
template <bool STAMPS, int PREC = PREC_F32>
__global__ __launch_bounds__(NET_THREADS) void net_kernel(const NetProgram* __restrict__ prog, int n_layers,
                                                          const float* __restrict__ W,
                                                          const uint32_t* __restrict__ boards,
                                                          const float* __restrict__ states, int in_channels,
                                                          const int32_t* __restrict__ count_ptr, int max_positions,
                                                          int policy_channels, float* __restrict__ logits,
                                                          float* __restrict__ value,
                                                          unsigned long long* __restrict__ stamps) {
  __shared__ __attribute__((aligned(16))) float lds[NET_LDS_FLOATS];
  float* const inp = lds + NET_BUFFERS * ACT_FLOATS;

  int count = max_positions;
  if (count_ptr != nullptr) {
    const int c = *count_ptr;
    count = c < count ? c : count;
  }
  const int tile0 = blockIdx.x * POS;
  if (tile0 >= count) return;

  // K groups may reach past a narrow layer's channels (their weights are zero): no NaN bit patterns in LDS
  for (int idx = threadIdx.x; idx < NET_BUFFERS * ACT_FLOATS; idx += NET_THREADS) lds[idx] = 0.0f;
  for (int idx = threadIdx.x; idx < STRIP_FLOATS; idx += NET_THREADS) lds[NET_LDS_FLOATS - STRIP_FLOATS + idx] = 0.0f;
  // input planes -> inp[cell][pos][4]
  for (int idx = threadIdx.x; idx < CELLS * POS * 4; idx += NET_THREADS) {
    const int c = idx & 3, pp = (idx >> 2) & 15, cell = idx >> 6;
    const int gp = tile0 + pp;
    float v = 0.0f;
    if (gp < count && c < in_channels) {
      if (boards != nullptr) v = (float)((boards[gp] >> (cell + 16 * c)) & 1u);
      else v = states[((size_t)gp * in_channels + c) * CELLS + cell];
    }
    if constexpr (PREC == PREC_BF16) v = bf16_round(v);
    inp[idx] = v;
  }
  __syncthreads();
  net_tile<STAMPS, false, PREC>(prog, W, lds, inp, policy_channels, count - tile0,
                                logits + (size_t)tile0 * policy_channels * CELLS, value + tile0,
                                STAMPS ? stamps + blockIdx.x * 4 : nullptr);
}

}  // namespace
}  // namespace nz
