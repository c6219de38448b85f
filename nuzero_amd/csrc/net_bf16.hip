// The stand-alone network kernel in plain-bf16 mode (nz_engine_precision; the arithmetic: net_dev.hpp), and its test
// hook, the dump kernel.  The float32 instantiations are net.hip's.
#include "net_dev.hpp"
#include "net_kernel.hpp"

namespace nz {
namespace {

// The test hook of the plain-bf16 mode (nz_net_forward_dump): net_kernel<false, PREC_BF16> on `states`, and what the
// device itself held, widened to float32, for all 16 rows of every tile (`padded` = 16 * tiles rows per array):
// planes [padded][9 cells][4], acts [stage][padded][NZ_NET_DUMP_ROW] = after each stage piece plane 0 of buffer 0, of
// buffer 1 ([cell][64 ch] each) and of the strip ([cell][16 ch]), vcells [padded][9].  The copy after a stage's barrier
// needs a barrier of its own before the next stage writes; the plain instantiation carries neither.
struct DumpStage {
  const unsigned char* lds;
  float* acts;
  int tile0, padded, max_stages;
  __device__ __forceinline__ void operator()(int stage) const {
    if (stage < max_stages) {
      for (int idx = threadIdx.x; idx < POS * NZ_NET_DUMP_ROW; idx += NET_THREADS) {
        const int pos = idx / NZ_NET_DUMP_ROW, e = idx % NZ_NET_DUMP_ROW;
        int byte;
        if (e < NET_BUFFERS * CELLS * ROW) {
          const int b = e / (CELLS * ROW), cell = (e / ROW) % CELLS, ch = e % ROW;
          byte = b * ACT_BYTES + slot_addr(cell, pos, ch >> 3) + (ch & 7) * 2;
        } else {
          const int r = e - NET_BUFFERS * CELLS * ROW, cell = r / 16, ch = r % 16;
          byte = (NET_BUFFERS * ACT_FLOATS + INP_FLOATS + VAL_FLOATS) * 4 + strip_addr(cell, pos, ch >> 3) + (ch & 7) * 2;
        }
        const uint32_t h = *reinterpret_cast<const uint16_t*>(lds + byte);
        acts[((size_t)stage * padded + tile0 + pos) * NZ_NET_DUMP_ROW + e] = bf16_lo(h);
      }
    }
    __syncthreads();
  }
};
static_assert(NZ_NET_DUMP_ROW == NET_BUFFERS * CELLS * ROW + CELLS * 16, "two buffers and the strip");
__global__ __launch_bounds__(NET_THREADS) void net_dump_kernel(const NetProgram* __restrict__ prog,
                                                               const float* __restrict__ W,
                                                               const float* __restrict__ states, int in_channels,
                                                               int count, int policy_channels, float* __restrict__ logits,
                                                               float* __restrict__ value, float* __restrict__ planes,
                                                               float* __restrict__ acts, int max_stages,
                                                               float* __restrict__ vcells_out) {
  __shared__ __attribute__((aligned(16))) float lds[NET_LDS_FLOATS];
  float* const inp = lds + NET_BUFFERS * ACT_FLOATS;
  const int tile0 = blockIdx.x * POS, padded = gridDim.x * POS;
  if (tile0 >= count) return;
  for (int idx = threadIdx.x; idx < NET_BUFFERS * ACT_FLOATS; idx += NET_THREADS) lds[idx] = 0.0f;
  for (int idx = threadIdx.x; idx < STRIP_FLOATS; idx += NET_THREADS) lds[NET_LDS_FLOATS - STRIP_FLOATS + idx] = 0.0f;
  for (int idx = threadIdx.x; idx < CELLS * POS * 4; idx += NET_THREADS) {
    const int c = idx & 3, pp = (idx >> 2) & 15, cell = idx >> 6;
    const int gp = tile0 + pp;
    float v = 0.0f;
    if (gp < count && c < in_channels) v = states[((size_t)gp * in_channels + c) * CELLS + cell];
    inp[idx] = bf16_round(v);
  }
  __syncthreads();
  for (int idx = threadIdx.x; idx < CELLS * POS * 4; idx += NET_THREADS) {      // what the input-plane step will read
    const int c = idx & 3, pp = (idx >> 2) & 15, cell = idx >> 6;
    planes[((size_t)(tile0 + pp) * CELLS + cell) * 4 + c] = inp[idx];
  }
  const DumpStage hook{reinterpret_cast<const unsigned char*>(lds), acts, tile0, padded, max_stages};
  net_tile<false, false, PREC_BF16, DumpStage>(prog, W, lds, inp, policy_channels, count - tile0,
                                               logits + (size_t)tile0 * policy_channels * CELLS, value + tile0, nullptr, 0, hook);
  const float* const vcells = inp + INP_FLOATS;                                  // the per-cell staging, before the mean
  for (int idx = threadIdx.x; idx < CELLS * POS; idx += NET_THREADS)
    vcells_out[(size_t)(tile0 + (idx & 15)) * CELLS + (idx >> 4)] = vcells[idx];
}

}  // namespace

// launch_net's kernel for NZ_PREC_BF16 (launch_net adds the softmax)
void launch_net_bf16(const NetProgram* prog_dev, const float* bf16_weights, const uint32_t* boards, const float* states,
                     const int32_t* count_dev, int max_positions, float* logits, float* value, unsigned long long* stamps,
                     hipStream_t s) {
  const int blocks = (max_positions + POS - 1) / POS;
  if (stamps != nullptr)
    hipLaunchKernelGGL((net_kernel<true, PREC_BF16>), dim3(blocks), dim3(NET_THREADS), 0, s, prog_dev, 0, bf16_weights, boards,
                       states, 2, count_dev, max_positions, 1, logits, value, stamps);
  else
    hipLaunchKernelGGL((net_kernel<false, PREC_BF16>), dim3(blocks), dim3(NET_THREADS), 0, s, prog_dev, 0, bf16_weights, boards,
                       states, 2, count_dev, max_positions, 1, logits, value, stamps);
}

void launch_net_dump(const NetProgram* prog_dev, const float* bf16_weights, const float* states, int batch, float* logits,
                     float* value, float* probs, float* planes, float* acts, int max_stages, float* vcells, hipStream_t s) {
  const int blocks = (batch + POS - 1) / POS;
  if (blocks <= 0) return;
  hipLaunchKernelGGL(net_dump_kernel, dim3(blocks), dim3(NET_THREADS), 0, s, prog_dev, bf16_weights, states, 2, batch, 1,
                     logits, value, planes, acts, max_stages, vcells);
  if (probs != nullptr) launch_softmax9(logits, probs, batch, s);
}

}  // namespace nz
