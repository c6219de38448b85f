// The scripted evaluation agents of nz_scs_agent_match_play: the bare policy and the random mover (SURVEY.md section
// 3.4; their rules are harness rules).  One wavefront per live match acts for the side that is
// not an MCTS agent, on the search handle's own games:
//   * policy agent: agent_image_kernel writes the current position's planes straight into the input rows of the
//     agent's board net (scs_state_image_wave), the host enqueues nz_boardnet_forward_rows on the device-side count,
//     agent_act_kernel takes the masked argmax of the match's row -- the lowest flat action index wins a tie (np.argmax);
//   * random agent: the match's MT19937 state stays in HBM between its decisions; agent_act_kernel draws
//     k = randint(n_legal) (scs_mt.hpp: numpy's legacy masked rejection, n == 1 draws nothing) and takes the k-th set bit
//     of the legal mask in ascending flat action index.
// The legal mask, the planes and the step are scs_dev.hpp's, the legal set and the copies scs_wave.hpp's, the stream in
// HBM scs_mt.hpp's.  Every loop is bounded; a rejection cap, a position without a legal action and a game past the
// records' bound set the match's error word.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/nuzero_amd.h"
#include "scs_agents.hpp"
#include "scs_mt.hpp"
#include "scs_wave.hpp"

namespace nz {
namespace {

// the side that decides in this position: agent 1 moves for player index 1
__device__ __forceinline__ int mover_of(const ScsState& s) { return s.player == 1 ? 0 : 1; }

__global__ __launch_bounds__(64) void agent_seed_kernel(const uint32_t* __restrict__ seeds, uint32_t* __restrict__ mt_keys,
                                                        int32_t* __restrict__ mt_pos, int n) {
  __shared__ __align__(16) uint32_t key[MT_N];
  const int lane = threadIdx.x, g = blockIdx.x;
  if (g >= n) return;
  mt_seed(key, seeds[g], lane);
  __syncthreads();
  mt_store_keys(mt_keys, g, key, lane);
  if (lane == 0) mt_pos[g] = MT_N;                       // as after RandomState(seed): the first draw twists
}

__global__ void agent_live_kernel(const ScsState* __restrict__ real, int n, const int32_t* __restrict__ error_flag,
                                  const int32_t* __restrict__ err, int32_t* __restrict__ out3) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  const bool in = g < n;
  const bool live = in && !real[g].terminal;
  const int e = in ? err[g] : 0;
  const int n_live = __popcll(__ballot(live));
  if ((threadIdx.x & 63) == 0 && n_live) atomicAdd(&out3[0], n_live);
  if (e) atomicOr(&out3[2], e);                          // (never in a sound round)
  if (g == 0) atomicOr(&out3[1], *error_flag);
}

// One launch per policy side: the positions `side` decides.  Two policy sides may share one network, whose input rows
// hold one side's positions at a time (the host runs image and forward side by side on one stream).  A match takes one
// slot per decision, so the slots stay below n_games, the rows the network holds.
__global__ __launch_bounds__(64) void agent_image_kernel(AgentArgs a, int side) {
  __shared__ __align__(16) ScsRules R;
  __shared__ ScsState sc;
  __shared__ int s_slot;
  const int lane = threadIdx.x, g = blockIdx.x;
  if (g >= a.n_games) return;
  const ScsState& real = a.real[g];
  if (real.terminal || real.length >= a.max_moves) return;           // (wave-uniform)
  if (mover_of(real) != side) return;
  const AgentSide& me = a.side[side];
  wave_copy<uint64_t>(&R, rules_of(a.rules, a.rules_row, g), lane);
  wave_copy<uint16_t>(&sc, &real, lane);
  if (lane == 0) s_slot = atomicAdd(me.count, 1);
  __syncthreads();
  const int slot = s_slot;
  // straight into the network's input rows: group of 16 slots, then cell, then slot
  float* const img = me.net_rows + ((size_t)(slot >> 4) * R.tiles * 16 + (slot & 15)) * me.row_stride;
  scs_state_image_wave<true>(R, sc, img, me.row_stride, lane);
  if (lane == 0) a.slot[g] = slot;
  if (me.hook_slot && me.hook_slot[g] >= 0) {
    // the digest of the planes just written, read back behind a fence (this wavefront's own stores)
    __threadfence();
    const int stride = me.row_stride;
    uint64_t hi, lo;
    scs_image_digest_wave(
        [&](int c, int t) { return __hip_atomic_load(img + (size_t)t * 16 * stride + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); },
        R.channels, R.tiles, lane, hi, lo);
    if (lane == 0) { a.digest[2 * g] = hi; a.digest[2 * g + 1] = lo; }
  }
}

__global__ __launch_bounds__(64) void agent_act_kernel(AgentArgs a) {
  __shared__ __align__(16) ScsRules R;
  __shared__ ScsState sc;
  __shared__ uint32_t smask[SCS_MASK_WORDS];
  __shared__ __align__(16) uint32_t key[MT_N];
  const int lane = threadIdx.x, g = blockIdx.x;
  if (g >= a.n_games) return;
  if (lane == 0) a.forced[g] = -1;
  const ScsState& real = a.real[g];
  if (real.terminal) return;                                          // (wave-uniform, as every return below)
  const int move = real.length, who = mover_of(real);
  const AgentSide& me = a.side[who];
  if (me.kind == NZ_AGENT_MCTS) return;                               // the search's own choice stands
  if (move >= a.max_moves) {
    if (lane == 0) atomicOr(&a.err[g], AGENT_ERR_LENGTH);
    return;
  }
  wave_copy<uint64_t>(&R, rules_of(a.rules, a.rules_row, g), lane);
  wave_copy<uint16_t>(&sc, &real, lane);
  __syncthreads();
  const WaveLegal legal = wave_legal(R, sc, smask, lane);
  const int n_legal = legal.count;
  if (n_legal == 0) {
    if (lane == 0) atomicOr(&a.err[g], AGENT_ERR_NO_LEGAL);
    return;
  }
  const int A = a.num_actions;
  int action = -1;
  float won = 0.0f;
  const float* row = nullptr;
  int slot = -1;
  if (me.kind == NZ_AGENT_POLICY) {
    slot = a.slot[g];                                                 // (agent_image_kernel's, under the same conditions)
    row = me.probs + (size_t)slot * A;
    // masked argmax: lane l looks at actions l, l + 64, ... in ascending order, so `>` keeps the lowest index of a tie
    float best = 0.0f;
    int at = -1;
    for (int i = lane; i < A; i += 64) {
      if (!((smask[i >> 5] >> (i & 31)) & 1u)) continue;
      const float p = row[i];
      if (at < 0 || p > best) { best = p; at = i; }
    }
    for (int o = 32; o; o >>= 1) {                                    // ds_bpermute butterfly over (probability, index)
      const float ob = __shfl_xor(best, o, 64);
      const int oa = __shfl_xor(at, o, 64);
      if (oa >= 0 && (at < 0 || ob > best || (ob == best && oa < at))) { best = ob; at = oa; }
    }
    action = at;
    won = best;
  } else {
    const int k = mt_stream_randint(key, me.mt_keys, me.mt_pos, g, n_legal, lane);
    if (k < 0) {
      if (lane == 0) atomicOr(&a.err[g], AGENT_ERR_CAP);
      return;
    }
    action = legal.kth(k, lane);
  }
  if (action < 0 || action >= A) {                                    // (cannot happen: k < n_legal, the mask has n_legal bits)
    if (lane == 0) atomicOr(&a.err[g], AGENT_ERR_NO_LEGAL);
    return;
  }
  const size_t gm = (size_t)g * a.max_moves + move;
  if (lane == 0) {
    a.forced[g] = action;
    me.rec_action[gm] = action;
    me.rec_n_legal[gm] = n_legal;
    me.rec_prob[gm] = won;
  }
  if (row && me.hook_slot && me.hook_slot[g] >= 0) {
    const int h = me.hook_slot[g], n = me.hook_count[h];
    if (n < me.hook_cap) {
      const size_t hat = (size_t)h * me.hook_cap + n;
      for (int i = lane; i < A; i += 64) me.hook_probs[hat * A + i] = row[i];
      if (lane == 0) {
        me.hook_value[hat] = me.value[slot];
        me.hook_digest[2 * hat] = a.digest[2 * g];
        me.hook_digest[2 * hat + 1] = a.digest[2 * g + 1];
      }
    }
    if (lane == 0) me.hook_count[h] = n + 1;
  }
  if (a.step) {
    // no engine searches: the games step here, and the handle's tree stays the unexpanded root of its reset -- the
    // right tree for whatever position the game is in
    scs_step_wave<true>(R, sc, action, lane);
    wave_copy<uint16_t>(&a.real[g], &sc, lane);
    if (lane == 0) a.rec_action[gm] = action;
  }
}

}  // namespace

hipError_t agent_seed_launch(const uint32_t* seeds, uint32_t* mt_keys, int32_t* mt_pos, int n, hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(agent_seed_kernel, dim3(n), dim3(64), 0, stream, seeds, mt_keys, mt_pos, n);
  return hipGetLastError();
}

hipError_t agent_live_launch(const ScsState* real, int n, const int32_t* error_flag, const int32_t* err, int32_t* out3,
                             hipStream_t stream) {
  hipLaunchKernelGGL(agent_live_kernel, dim3((n + 127) / 128), dim3(128), 0, stream, real, n, error_flag, err, out3);
  return hipGetLastError();
}

hipError_t agent_image_launch(const AgentArgs& a, int side, hipStream_t stream) {
  hipLaunchKernelGGL(agent_image_kernel, dim3(a.n_games), dim3(64), 0, stream, a, side);
  return hipGetLastError();
}

hipError_t agent_act_launch(const AgentArgs& a, hipStream_t stream) {
  hipLaunchKernelGGL(agent_act_kernel, dim3(a.n_games), dim3(64), 0, stream, a);
  return hipGetLastError();
}

}  // namespace nz
