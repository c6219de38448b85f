// Evaluation matches from opening positions (nz_scs_search_reset_to, nz_scs_openings_draw, nz_scs_openings_expand;
// DESIGN.md section 5b).  Evaluation agents are deterministic, so the matches of a round on one map are copies of one
// game unless they start at different positions.  Three kernels, one wavefront per match or prefix, the rules row and the
// game in LDS (scs_wave.hpp):
//   * apply: after the slot's reset, replay the match's prefix through the legal mask and the step; the tree stays the
//     unexpanded root (MctsAgent.new_game, then choose_action, on a game stepped to the position);
//   * draw: the random agent's rule from the start, on the stream RandomState(opening_seeds[g]);
//   * expand: a frontier of prefixes one ply deeper, in ascending action order, with each child position's key -- the
//     128-bit digest of the child's planes (scs_image_digest_wave, what the leaf records of the persistent route hold).
//     The inference cache's state hash would not do: it tells two units of one type apart, so the two orders of placing
//     them on two tiles -- one position to the network and to the rules -- would count twice.
// Every loop is bounded (plies, mask words, 32 bits a word); an action indexes the mask only after its range check; the
// first violation stops the wavefront and is reported in the match's error word.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/nuzero_amd.h"
#include "scs_mt.hpp"
#include "scs_openings.hpp"
#include "scs_wave.hpp"

namespace nz {
namespace {

// Replays acts[0 .. n) on the game `sc` (LDS): 0, or the error word of the first violation, at which `sc` stays where the
// sound part of the prefix left it.  Wave-uniform: every lane returns the same word.
__device__ __forceinline__ int32_t replay_prefix(const ScsRules& R, ScsState& sc, uint32_t* smask, const int32_t* acts, int n,
                                                 int num_actions, int max_moves, int lane) {
  for (int ply = 0; ply < n; ++ply) {
    const int a = acts[ply];
    const int refused = scs_admit_wave(R, sc, smask, a, num_actions, lane);
    // the records' bound is reported behind a game that is over and ahead of what is wrong with the action itself
    if (refused == SCS_ADMIT_GAME_OVER) return (ply << 8) | OPENING_ERR_GAME_OVER;
    if (sc.length >= max_moves) return (ply << 8) | OPENING_ERR_LENGTH;
    if (refused) return (ply << 8) | OPENING_ERR_ILLEGAL;
    scs_step_wave<true>(R, sc, a, lane);
  }
  return 0;
}

__global__ __launch_bounds__(64) void opening_apply_kernel(OpeningGames og, int n, const int32_t* __restrict__ actions,
                                                           const int32_t* __restrict__ n_plies, int max_plies, ScsState* real,
                                                           int32_t* __restrict__ rec_action, int max_moves,
                                                           int32_t* __restrict__ err) {
  __shared__ __align__(16) ScsRules R;
  __shared__ ScsState sc;
  __shared__ uint32_t smask[SCS_MASK_WORDS];
  const int lane = threadIdx.x, g = blockIdx.x;
  if (g >= n) return;
  wave_copy<uint64_t>(&R, rules_of(og.rules, og.rules_row, g), lane);
  wave_copy<uint16_t>(&sc, &real[g], lane);
  __syncthreads();
  int np = n_plies ? n_plies[g] : max_plies;
  np = np < 0 ? 0 : np > max_plies ? max_plies : np;                  // (the host refused anything else)
  const int32_t* const mine = actions + (size_t)g * max_plies;
  const int first = sc.length;                                        // (0: the slot was just reset)
  int32_t e = replay_prefix(R, sc, smask, mine, np, og.num_actions, max_moves, lane);
  if (!e && first + np > max_moves) e = (np << 8) | OPENING_ERR_LENGTH;
  if (lane == 0) err[g] = e;
  if (e) return;                                                      // (wave-uniform) the match stays at its reset state
  wave_copy<uint16_t>(&real[g], &sc, lane);
  // records stay indexed by the game's decision number; rec_children / rec_tree_size stay 0: nobody searched these plies
  for (int ply = lane; ply < np; ply += 64) rec_action[(size_t)g * max_moves + first + ply] = mine[ply];
}

__global__ __launch_bounds__(64) void opening_draw_kernel(OpeningGames og, int n, const uint32_t* __restrict__ seeds, int plies,
                                                          int32_t* __restrict__ actions_out, int32_t* __restrict__ n_plies_out,
                                                          int32_t* __restrict__ err) {
  __shared__ __align__(16) ScsRules R;
  __shared__ ScsState sc;
  __shared__ uint32_t smask[SCS_MASK_WORDS];
  __shared__ __align__(16) uint32_t key[MT_N];
  const int lane = threadIdx.x, g = blockIdx.x;
  if (g >= n) return;
  wave_copy<uint64_t>(&R, rules_of(og.rules, og.rules_row, g), lane);
  mt_seed(key, seeds[g], lane);
  __syncthreads();
  if (lane == 0) Scs(R, sc).reset();
  __syncthreads();
  Mt m{key, MT_N, lane};                                              // as after RandomState(seed): the first draw twists
  int32_t e = 0;
  int ply = 0;
  for (; ply < plies; ++ply) {
    if (sc.terminal) break;                                           // (wave-uniform, as every exit below)
    const WaveLegal legal = wave_legal(R, sc, smask, lane);
    const int n_legal = legal.count;
    if (n_legal == 0) { e = (ply << 8) | OPENING_ERR_NO_LEGAL; break; }
    const int k = mt_randint(m, n_legal);
    if (k < 0) { e = (ply << 8) | OPENING_ERR_CAP; break; }
    const int action = legal.kth(k, lane);
    if (action < 0 || action >= og.num_actions) { e = (ply << 8) | OPENING_ERR_NO_LEGAL; break; }   // (cannot happen: k < n_legal)
    if (lane == 0) actions_out[(size_t)g * plies + ply] = action;
    scs_step_wave<true>(R, sc, action, lane);
  }
  for (int i = ply + lane; i < plies; i += 64) actions_out[(size_t)g * plies + i] = -1;
  if (lane == 0) {
    n_plies_out[g] = ply;
    err[g] = e;
  }
}

__global__ __launch_bounds__(64) void opening_expand_kernel(OpeningGames og, int n, const int32_t* __restrict__ frontier,
                                                            int depth, int max_moves, int32_t* __restrict__ counts,
                                                            const int32_t* __restrict__ offsets, int total,
                                                            int32_t* __restrict__ children, uint64_t* __restrict__ keys,
                                                            float* __restrict__ planes, int32_t* __restrict__ err) {
  __shared__ __align__(16) ScsRules R;
  __shared__ ScsState sc, child;
  __shared__ uint32_t smask[SCS_MASK_WORDS];
  const int lane = threadIdx.x, f = blockIdx.x;
  if (f >= n) return;
  wave_copy<uint64_t>(&R, rules_of(og.rules, og.rules_row, f), lane);
  __syncthreads();
  if (lane == 0) Scs(R, sc).reset();
  __syncthreads();
  const int32_t* const mine = frontier + (size_t)f * depth;
  const int32_t e = replay_prefix(R, sc, smask, mine, depth, og.num_actions, max_moves, lane);
  if (lane == 0) err[f] = e;
  int n_legal = 0;
  if (!e && !sc.terminal && sc.length < max_moves)                    // a terminal prefix has no children
    n_legal = wave_legal(R, sc, smask, lane).count;
  if (!children) {
    if (lane == 0) counts[f] = n_legal;
    return;
  }
  const int base = offsets[f];
  if (base < 0 || base > total) return;                               // (the host's scan; kept as the bound of the stores)
  const int room = n_legal < total - base ? n_legal : total - base;
  float* const img = planes + (size_t)f * R.channels * R.tiles;       // this wavefront's own [channels][tiles]
  const int tiles = R.tiles;
  int j = 0;
  for (int w = 0; w < SCS_MASK_WORDS && j < room; ++w) {
    uint32_t bits = smask[w];
    while (bits && j < room) {                                        // (at most 32 rounds, ascending)
      const int a = w * 32 + __ffs((int)bits) - 1;
      bits &= bits - 1;
      wave_copy<uint16_t>(&child, &sc, lane);
      __syncthreads();
      scs_step_wave<true>(R, child, a, lane);
      // the digest of the planes just written, read back behind a fence (this wavefront's own stores)
      scs_state_image_wave<false>(R, child, img, 0, lane);
      __threadfence();
      uint64_t hi, lo;
      scs_image_digest_wave(
          [&](int c, int t) { return __hip_atomic_load(img + c * tiles + t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); },
          R.channels, tiles, lane, hi, lo);
      const size_t at = (size_t)(base + j);
      for (int i = lane; i < depth; i += 64) children[at * (depth + 1) + i] = mine[i];
      if (lane == 0) {
        children[at * (depth + 1) + depth] = a;
        keys[2 * at] = hi;
        keys[2 * at + 1] = lo;
      }
      ++j;
      __syncthreads();                                                // the image's reads of `child` before the next copy
    }
  }
}

}  // namespace

hipError_t opening_apply_launch(const OpeningGames& og, int n, const int32_t* actions, const int32_t* n_plies, int max_plies,
                                ScsState* real, int32_t* rec_action, int max_moves, int32_t* err, hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(opening_apply_kernel, dim3(n), dim3(64), 0, stream, og, n, actions, n_plies, max_plies, real, rec_action,
                     max_moves, err);
  return hipGetLastError();
}

hipError_t opening_draw_launch(const OpeningGames& og, int n, const uint32_t* seeds, int plies, int32_t* actions_out,
                               int32_t* n_plies_out, int32_t* err, hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(opening_draw_kernel, dim3(n), dim3(64), 0, stream, og, n, seeds, plies, actions_out, n_plies_out, err);
  return hipGetLastError();
}

hipError_t opening_expand_launch(const OpeningGames& og, int n, const int32_t* frontier, int depth, int max_moves,
                                 int32_t* counts, const int32_t* offsets, int total, int32_t* children, uint64_t* keys,
                                 float* planes, int32_t* err, hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(opening_expand_kernel, dim3(n), dim3(64), 0, stream, og, n, frontier, depth, max_moves, counts, offsets, total,
                     children, keys, planes, err);
  return hipGetLastError();
}

}  // namespace nz
