// Per-game "Randomized" SCS maps drawn on the device, one wavefront per game.
//
// Restates what SCS_Game.load_game_from_config draws (SCS_Game.py:1678-1738) when numpy's global stream was seeded
// with the game's seed just before (Training/Gamer.py:52), i.e. nuzero_amd.scs.randomized_map with RandomState(seed):
//   * MT19937 as numpy's legacy RandomState (scs_mt.hpp, shared with the random evaluation agent): init_genrand for an
//     integer seed, the twist, tempering, random_sample = the 53-bit double;
//   * a tile's terrain: choice(len(types), p=dist) = searchsorted(cdf, random_sample(), side='right') on the float64
//     cdf the host computed with numpy itself (cdf = p.cumsum(); cdf /= cdf[-1]);
//   * a victory point: (choice(range(rows)), choice(range of the side's columns)), redrawn while it repeats one already
//     on that side's list; choice(range(n)) without p is the legacy randint(0, n): masked rejection on 32-bit words,
//     n == 1 consumes nothing;
//   * the sections in the config file's order.
// Every lane runs the same (wave-uniform) draw sequence on the state in LDS; the twist is spread over the lanes.  The
// game's rules row is built in the same pass with the host's scs_apply_map and digested with scs_map_digest.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/nuzero_amd.h"
#include "scs_mt.hpp"
#include "scs_wave.hpp"

namespace nz {
namespace {

// Bound of the redraw loop: the host refuses more victory points than a side has cells, so a valid config never reaches
// it (nor MT_RANDINT_TRIES, scs_mt.hpp); reaching one sets SCS_DRAW_ERR_CAP for the game instead of spinning.
constexpr int VP_REDRAWS = 1 << 16;

__global__ __launch_bounds__(64) void scs_draw_kernel(ScsDrawSpec sp, const ScsRules* __restrict__ tmpl, int64_t n,
                                                      const uint32_t* __restrict__ seeds, ScsRules* __restrict__ rows,
                                                      uint64_t* __restrict__ rules_key, float* __restrict__ terrain_out,
                                                      int32_t* __restrict__ vp_out, uint32_t* __restrict__ mt_keys,
                                                      int32_t* __restrict__ mt_pos, int32_t* __restrict__ err_out) {
  __shared__ __align__(16) uint32_t key[MT_N];
  __shared__ __align__(16) ScsRules row;
  __shared__ float terr[SCS_MAX_TILES * 3];
  __shared__ int32_t vp[2 * SCS_MAX_TILES * 2];
  const int lane = threadIdx.x;
  const int64_t g = blockIdx.x;
  if (g >= n) return;

  // the engine's template row; init_genrand (a serial recurrence: one lane)
  wave_copy<uint64_t>(&row, tmpl, lane);
  mt_seed(key, seeds[g], lane);
  __syncthreads();
  // the template's map: what the sections the config gives in "Detailed" form stay
  const int T = row.tiles, cols = row.cols, nv0 = row.n_vp[0], nv = row.n_vp[0] + row.n_vp[1];
  for (int t = lane; t < T; t += 64)
    for (int k = 0; k < 3; ++k) terr[t * 3 + k] = row.terrain_f[t][k];
  for (int i = lane; i < nv; i += 64) {
    const int tile = i < nv0 ? row.vp[0][i] : row.vp[1][i - nv0];
    vp[i * 2] = tile / cols;
    vp[i * 2 + 1] = tile % cols;
  }
  __syncthreads();

  Mt m{key, MT_N, lane};
  int err = 0;
  for (int s = 0; s < 2 && !err; ++s) {
    if (sp.order[s] == NZ_SCS_DRAW_MAP) {
      for (int t = 0; t < T; ++t) {                       // row by row: tile index order
        const double u = mt_double(m);
        int idx = 0;                                      // searchsorted(cdf, u, 'right'): entries <= u
        while (idx < sp.n_types - 1 && sp.cdf[idx] <= u) ++idx;
        if (lane == 0)
          for (int k = 0; k < 3; ++k) terr[t * 3 + k] = sp.types[idx][k];
      }
    } else if (sp.order[s] == NZ_SCS_DRAW_VP) {
      for (int side = 0; side < 2 && !err; ++side) {
        const int first = sp.side_cols[side][0], width = sp.side_cols[side][1] - first, base = side ? nv0 : 0;
        for (int i = 0; i < sp.number_vp[side] && !err; ++i) {
          bool placed = false;
          for (int redraw = 0; redraw < VP_REDRAWS && !placed && !err; ++redraw) {
            const int r = mt_randint(m, row.rows);
            const int c = r < 0 ? -1 : mt_randint(m, width);
            if (r < 0 || c < 0) { err = SCS_DRAW_ERR_CAP; break; }
            bool dup = false;
            for (int j = 0; j < i; ++j) dup |= vp[(base + j) * 2] == r && vp[(base + j) * 2 + 1] == first + c;
            if (!dup) {
              if (lane == 0) { vp[(base + i) * 2] = r; vp[(base + i) * 2 + 1] = first + c; }
              placed = true;
            }
            __syncthreads();                              // the point is on the list before the next is checked
          }
          if (!placed) err = SCS_DRAW_ERR_CAP;
        }
      }
    }
  }
  __syncthreads();

  // the game's rules row and its digest (one lane: the host functions as they are)
  if (lane == 0) {
    scs_apply_map(&row, terr, vp);
    for (int t = 0; t < T; ++t)
      if (row.cost[t] < 1 && !err) err = SCS_DRAW_ERR_COST;
    uint64_t d[2];
    scs_map_digest(row, d);
    rules_key[2 * g] = d[0];
    rules_key[2 * g + 1] = d[1];
    mt_pos[g] = m.pos;
    err_out[g] = err;
  }
  __syncthreads();

  wave_copy<uint64_t>(rows + g, &row, lane);
  mt_store_keys(mt_keys, g, key, lane);
  for (int i = lane; i < T * 3; i += 64) terrain_out[(size_t)g * T * 3 + i] = terr[i];
  for (int i = lane; i < nv * 2; i += 64) vp_out[(size_t)g * nv * 2 + i] = vp[i];
}

}  // namespace

hipError_t scs_draw_launch(const ScsDrawSpec& spec, const ScsRules* tmpl, int64_t n, const uint32_t* seeds,
                           ScsRules* rows, uint64_t* rules_key, float* terrain, int32_t* vp, uint32_t* mt_keys,
                           int32_t* mt_pos, int32_t* err, hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(scs_draw_kernel, dim3((unsigned)n), dim3(64), 0, stream, spec, tmpl, n, seeds, rows, rules_key,
                     terrain, vp, mt_keys, mt_pos, err);
  return hipGetLastError();
}

}  // namespace nz
