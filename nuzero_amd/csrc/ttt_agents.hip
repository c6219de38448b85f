// The scripted evaluation agents of nz_engine_match_play on Tic-Tac-Toe -- the bare policy and the random mover -- and the
// match's own bookkeeping (reset, state images, step, tally).  Their rules are the harness rules of scs_agents.hip
// (parity unpinned):
//   * policy agent: the masked argmax of the side's nine softmax probabilities (its network's output for the match's
//     state image, or its table's row of the position), the lowest cell index winning a tie (np.argmax);
//   * random agent: the match's MT19937 state stays in HBM between its decisions; k = randint(n_legal) (scs_mt.hpp:
//     numpy's legacy masked rejection, n == 1 draws nothing), then the k-th empty cell in ascending index.
// All matches of a round are at the same ply, so the host knows which side moves and of which kind: a launch serves one
// side.  ttt_agent_move_kernel runs one wavefront per match (the MT19937 twist of scs_mt.hpp meets at __syncthreads:
// one wavefront per workgroup); every branch around a barrier is uniform over the workgroup.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/nuzero_amd.h"
#include "scs_mt.hpp"
#include "tree_dev.hpp"
#include "ttt_agents.hpp"

namespace nz {
namespace {

__global__ void ttt_match_reset_kernel(TttMatchArgs a, const uint32_t* __restrict__ start) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;          // over n * 9
  if (idx >= a.n * TTT_MAX_MOVES) return;
  a.actions[idx] = -1;
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    a.agent_actions[s][idx] = -1;
    a.agent_n_legal[s][idx] = 0;
  }
  if (idx < a.n) {
    const uint32_t board = start ? start[idx] : 0u;
    a.board[idx] = board;
    a.alive[idx] = 1;
    a.length[idx] = ttt_length(board);                            // the record is by absolute ply
    a.outcome[idx] = 0;
    a.forced[idx] = -1;
    a.err[idx] = 0;
  }
}

// tic_tac_toe.py:135-159: (player-one stones, player-two stones), no side-to-move plane
__global__ void ttt_state_image_kernel(TttMatchArgs a) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;          // over n * 18
  if (idx >= a.n * 18) return;
  const int cell = idx % 9, plane = (idx / 9) % 2, i = idx / 18;
  a.states[idx] = a.alive[i] ? (float)((a.board[i] >> (cell + 16 * plane)) & 1u) : 0.0f;
}

__global__ __launch_bounds__(64) void ttt_agent_move_kernel(TttMatchArgs a, int side, int kind,
                                                            const float* __restrict__ table) {
  __shared__ __align__(16) uint32_t key[MT_N];
  const int lane = threadIdx.x, i = blockIdx.x;
  if (i >= a.n) return;                                           // (uniform over the workgroup, as every return below)
  if (lane == 0) a.forced[i] = -1;
  if (!a.alive[i]) return;
  const uint32_t board = a.board[i];
  const uint32_t legal = ttt_empty(board);
  const int n_legal = __popc(legal), ply = a.length[i];
  if (n_legal == 0 || ply >= TTT_MAX_MOVES) {
    if (lane == 0) atomicOr(&a.err[i], TTT_AGENT_ERR_NO_LEGAL);
    return;
  }
  int action;
  if (kind == NZ_AGENT_POLICY) {
    const float* row = table ? table + (size_t)ttt_code(board) * 10 : a.probs + (size_t)i * TTT_ACTIONS;
    const bool mine = lane < TTT_ACTIONS && ((legal >> lane) & 1u);
    float best = mine ? row[lane] : 0.0f;
    int at = mine ? lane : -1;
    for (int o = 8; o; o >>= 1) {                                 // butterfly over (probability, index) in the first row
      const float ob = __shfl_xor(best, o, 16);
      const int oa = __shfl_xor(at, o, 16);
      if (oa >= 0 && (at < 0 || ob > best || (ob == best && oa < at))) { best = ob; at = oa; }
    }
    action = __shfl(at, 0, 64);
  } else {
    const int k = mt_stream_randint(key, a.mt_keys[side], a.mt_pos[side], i, n_legal, lane);
    if (k < 0) {
      if (lane == 0) atomicOr(&a.err[i], TTT_AGENT_ERR_CAP);
      return;
    }
    uint32_t x = legal;
    for (int j = 0; j < k; ++j) x &= x - 1u;                      // (k < n_legal <= 9)
    action = __ffs((int)x) - 1;
  }
  if (action < 0 || action >= TTT_ACTIONS || !((legal >> action) & 1u)) {   // (cannot happen: the mask has n_legal bits)
    if (lane == 0) atomicOr(&a.err[i], TTT_AGENT_ERR_NO_LEGAL);
    return;
  }
  if (lane == 0) {
    a.forced[i] = action;
    a.agent_actions[side][i * TTT_MAX_MOVES + ply] = action;
    a.agent_n_legal[side][i * TTT_MAX_MOVES + ply] = n_legal;
  }
}

__global__ void ttt_match_step_kernel(TttMatchArgs a) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.n || !a.alive[i]) return;
  const uint32_t board = a.board[i];
  const int action = a.forced[i], ply = a.length[i];
  if (action < 0 || action >= TTT_ACTIONS || !((ttt_empty(board) >> action) & 1u) || ply >= TTT_MAX_MOVES) {
    atomicOr(&a.err[i], TTT_AGENT_ERR_ACTION);
    a.alive[i] = 0;                                               // counted as unfinished: its length stays short
    return;
  }
  const uint32_t next = ttt_step(board, action);
  a.actions[i * TTT_MAX_MOVES + ply] = action;
  a.board[i] = next;
  a.length[i] = ply + 1;
  const int term = ttt_terminal(next);
  if (term != 0) {
    a.alive[i] = 0;
    a.outcome[i] = term_value(term);
  }
}

// (The SCS tally, scs_search.hip match_tally_kernel, reads ScsState records and two engines' action records; what is
// shared with it is the shape: ballots, then one vector atomic per wavefront and category.)
__global__ void ttt_match_tally_kernel(TttMatchArgs a, const int32_t* __restrict__ flag1, const int32_t* __restrict__ flag2,
                                       unsigned long long* __restrict__ tally) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const bool in = i < a.n;
  bool done = false;
  int value = 0, e = 0;
  if (in) {
    done = ttt_terminal(a.board[i]) != 0;
    value = a.outcome[i];
    e = a.err[i];
  }
  const int n_p1 = __popcll(__ballot(in && done && value > 0)), n_p2 = __popcll(__ballot(in && done && value < 0)),
            n_draw = __popcll(__ballot(in && done && value == 0)), n_open = __popcll(__ballot(in && !done));
  if ((threadIdx.x & 63) == 0) {
    if (n_p1) atomicAdd(&tally[0], (unsigned long long)n_p1);
    if (n_p2) atomicAdd(&tally[1], (unsigned long long)n_p2);
    if (n_draw) atomicAdd(&tally[2], (unsigned long long)n_draw);
    if (n_open) atomicAdd(&tally[3], (unsigned long long)n_open);
  }
  if (e) atomicOr(&tally[4], (unsigned long long)e);              // (never in a sound round)
  if (i == 0) {
    if (flag1) tally[5] = (unsigned long long)*flag1;
    if (flag2) tally[6] = (unsigned long long)*flag2;
  }
}

}  // namespace

void ttt_match_reset_launch(const TttMatchArgs& a, const uint32_t* start, hipStream_t s) {
  const int total = a.n * TTT_MAX_MOVES;
  hipLaunchKernelGGL(ttt_match_reset_kernel, dim3((total + 255) / 256), dim3(256), 0, s, a, start);
}
void ttt_state_image_launch(const TttMatchArgs& a, hipStream_t s) {
  const int total = a.n * 18;
  hipLaunchKernelGGL(ttt_state_image_kernel, dim3((total + 255) / 256), dim3(256), 0, s, a);
}
void ttt_agent_move_launch(const TttMatchArgs& a, int side, int kind, const float* table, hipStream_t s) {
  hipLaunchKernelGGL(ttt_agent_move_kernel, dim3(a.n), dim3(64), 0, s, a, side, kind, table);
}
void ttt_match_step_launch(const TttMatchArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(ttt_match_step_kernel, dim3((a.n + 255) / 256), dim3(256), 0, s, a);
}
void ttt_match_tally_launch(const TttMatchArgs& a, const int32_t* flag1, const int32_t* flag2, unsigned long long* tally,
                            hipStream_t s) {
  hipLaunchKernelGGL(ttt_match_tally_kernel, dim3((a.n + 255) / 256), dim3(256), 0, s, a, flag1, flag2, tally);
}

}  // namespace nz
